"""Hard targets for the two fit stages with entry points of their own — one rotation pass (smplfit_part_rotations_f32 /
BodyFitter._part_rotations) and one shape solve (smplfit_shape_solve_ex_f32 / BodyFitter._shape_solve) — and the criteria
that compare them with the fp64 oracle of the same operation (OracleFitter.fit_global_rotations / fit_shape).  Plain numpy;
used by tests/test_gpu_stages_hard.py and, for the rotation pass of the host build, by tests/test_hostemu.py.

Targets come from the fp64 oracle forward (util.forward64), rounded to fp32: never from the kernels under test."""

import numpy as np

import prim_util as P
import util

B = 8
GAP_MIN = 1e-2        # a part's rotation is compared entry by entry where (s2 + d s3) / s1 exceeds this
BONE_MIN = 1e-3       # bone parts: both bones longer than this (m) and no closer than this (rad) to antiparallel
# A bone part's twist is atan2(s, c) of two contractions of its covariance A: an error delta in (s, c) / |A|_F turns the
# part by delta / kappa, kappa = hypot(s, c) / |A|_F (the fp64 oracle's).  The 5e-4 stage gate was set on small poses,
# where kappa >= 0.1 on every bone pair (the oracle alone: >= 0.09 on 'hard_pose', 0.15 on 'far', median 0.33), i.e. it
# admits delta = 5e-5.  A mirrored target pushes kappa down to 3e-3 (median 3e-2), and two fp32 evaluations of the same
# pair then scatter by delta / kappa >> 5e-4 in the reference's arithmetic too.  Bone pairs are therefore held to the
# same delta: |G - G64| * min(kappa / 0.1, 1) <= max(2 x the fp32 oracle's (same factor), gate) — unchanged for
# kappa >= 0.1, and the bone-part analogue of the conditioned distance of proj_so3 (prim_util.PROJ_DIST_TOL).
KAPPA_REF = 0.1
DEFICIT_FLOOR = 1e-6  # optimality deficit relative to s1
MIN_GATED = 0.9       # unmasked families: share of the (instance, part) pairs that must fall under a distance gate
MESH_GATE, BETA_GATE, TRANS_GATE = 1e-4, 3e-4, 1e-5  # the gates of test_fit_vs_oracle
UNMASKED = ('hard_pose', 'pose1', 'mirror', 'betas5', 'far')
MASKED = ('part_off', 'part_two', 'mask01', 'joint_off')
FAR_ROW = util.FWD_FAR


def dist_gate(name):
    """The existing stage gate on the iteration-0 rotations (test_stage_goldens)."""
    return 2e-3 if name.startswith('smplx') else 5e-4


def families(om64, of64, seed=0):
    """name -> dict(tv, tj, vw, jw): float32 targets (B instances) and weights (None where the family has none).

    hard_pose  util.forward_inputs: per joint zero, tiny, ordinary, large (3 rad a component) and near-pi rotations
    pose1      rotation vectors of 1 rad a component, 5 mm of noise on the vertices
    mirror     the x-mirrored mesh: every part covariance has a negative determinant
    betas5     betas at the +-5 corners
    far        instance FAR_ROW translated by 1000 m (the centring identity cancels there)
    part_off   vertex weights with one whole part at 0          part_two   one part reduced to two vertices
    mask01     random 0/1 vertex weights                          joint_off  joint weights with one joint at 0"""
    rs = np.random.RandomState(seed)
    J, S, V = om64.J, om64.S, om64.V
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731

    def fwd(pose, betas, trans, noise=0.0):
        fw = util.forward64(om64, pose_rotvecs=f32(pose), shape_betas=f32(betas), trans=f32(trans))
        return dict(tv=f32(fw['vertices'] + noise * rs.randn(B, V, 3)), tj=f32(fw['joints']), vw=None, jw=None)

    betas, trans = rs.randn(B, S) * 0.5, rs.randn(B, 3)
    out = {}
    fi = util.forward_inputs(B, J, S, seed=seed + 1)
    out['hard_pose'] = fwd(fi['pose_rotvecs'], betas, trans)
    out['pose1'] = fwd(rs.randn(B, 3 * J), betas, trans, noise=0.005)
    base = fwd(rs.randn(B, 3 * J) * 0.3, betas, trans, noise=0.005)
    mir = np.array([-1.0, 1, 1], np.float32)
    out['mirror'] = dict(base, tv=f32(base['tv'] * mir), tj=f32(base['tj'] * mir))
    out['betas5'] = fwd(rs.randn(B, 3 * J) * 0.3, rs.choice([-5.0, 5.0], (B, S)), trans)
    far = trans.copy()
    far[FAR_ROW] += (1000.0, -1000.0, 1000.0)
    out['far'] = fwd(rs.randn(B, 3 * J) * 0.3, betas, far)
    leaf, bone = of64.leaf[len(of64.leaf) // 2], of64.bone[len(of64.bone) // 2]
    vw = np.ones((B, V), np.float32)
    vw[:, of64.sel[leaf]] = 0
    vw[B // 2:, of64.sel[bone]] = 0  # (a bone part too, on half of the instances)
    out['part_off'] = dict(base, vw=vw, jw=np.ones((B, J), np.float32))
    vw = np.ones((B, V), np.float32)
    for p in (leaf, bone):
        vw[:, of64.sel[p][2:]] = 0
    out['part_two'] = dict(base, vw=vw, jw=np.ones((B, J), np.float32))
    out['mask01'] = dict(base, vw=f32(rs.rand(B, V) < 0.5), jw=np.ones((B, J), np.float32))
    jw = np.ones((B, J), np.float32)
    jw[:, of64.multi[-1]] = 0
    jw[B // 2:, of64.cas[of64.multi[0]][1]] = 0
    out['joint_off'] = dict(base, vw=np.ones((B, V), np.float32), jw=jw)
    return out


def centred(dtype, tv, tj):
    """The targets in ``dtype`` minus their mean, as every entry point centres them (pt/bodyfitter.py:355-361)."""
    tv = np.asarray(tv, dtype)
    tj = None if tj is None else np.asarray(tj, dtype)
    mean = tv.mean(1) if tj is None else np.concatenate([tv, tj], 1).mean(1)
    return tv - mean[:, None], None if tj is None else tj - mean[:, None], mean


def oracle_rotations(of, fam):
    """(G, info) of the oracle's first rotation pass on a family, in the oracle's dtype."""
    dt = of.m.dtype
    tv, tj, _ = centred(dt, fam['tv'], fam['tj'])
    w = lambda a: None if a is None else np.asarray(a, dt)  # noqa: E731
    return of.fit_global_rotations(tv, tj, of.default_mesh[None], of.m.J_template[None], w(fam['vw']), w(fam['jw']),
                                   return_cov=True)


_setups = {}


def host_setup(name, model_root, golden):
    """Oracles, families and the oracles' first rotation passes of one model kind: computed once, shared, read only."""
    if name not in _setups:
        kind, md = util.load_md(model_root, name, golden(name))
        om64, of64 = util.make_oracle(md, kind, np.float64)
        om32, of32 = util.make_oracle(md, kind, np.float32)
        fams = families(om64, of64)
        rot = {k: (oracle_rotations(of64, fam), oracle_rotations(of32, fam)[0]) for k, fam in fams.items()}
        _setups[name] = dict(om64=om64, om32=om32, of64=of64, of32=of32, fams=fams, rot=rot)
    return _setups[name]


def rotation_figures(G, G32, G64, info, gate, prev=None):
    """A rotation pass ``G`` (B, J, 3, 3) against the fp64 oracle's ``G64`` with its covariances ``info``, PAIR BY PAIR
    (instance, part); the fp32 oracle's ``G32`` gives each pair's floor.  Returns the family maxima (recorded figures)
    and the pairs that miss a gate: ``bad_deficit`` (Kabsch parts: deficit > max(4 x the fp32 oracle's on that pair,
    1e-6)), ``bad_dist`` (pairs under a distance gate: |G - G64| > max(2 x |G32 - G64| on that pair, ``gate``)), each
    as (instance, part, ours, fp32 oracle).  Distances of bone pairs carry the factor min(kappa / KAPPA_REF, 1) (above)
    on both sides.

    ``prev`` (B, J, 3, 3): the pass composed a DELTA rotation with these previous ones (a later pass of a fit, the
    refinement) — ``info['cov']`` is the delta's covariance, so the deficit and the gap are evaluated on ``R prev^T``
    while the distance stays on the composed rotation.  ``info['toes']``: the parts that copy part - 3 (default: every
    part without a rotation of its own); the refinement, where kind -1 is 'not adjusted', names them itself."""
    kind = info['kind']
    own = kind >= 0
    G, G32, G64 = (np.asarray(x, np.float64) for x in (G, G32, G64))
    A = info['cov'].astype(np.float64)
    U, s, Vt = np.linalg.svd(A)
    d = np.sign(np.linalg.det(U @ Vt))
    s1 = np.where(s[..., 0] > 0, s[..., 0], 1.0)
    best = s[..., 0] + s[..., 1] + d * s[..., 2]
    delta = (lambda R: R) if prev is None else (lambda R: R @ np.swapaxes(np.asarray(prev, np.float64), -1, -2))  # noqa: E731
    deficit = lambda R: (best - np.einsum('bjrc,bjrc->bj', delta(R), A)) / s1  # noqa: E731
    gap = (s[..., 1] + d * s[..., 2]) / s1
    kab = ((kind == 0) | (kind == 1))[None] & np.ones_like(gap, bool)
    cosang = (info['bone_ref'] * info['bone_tgt']).sum(-1)
    bone_ok = (kind == 2) & (info['bone_ref_len'] > BONE_MIN) & (info['bone_tgt_len'] > BONE_MIN) & \
        (np.arccos(np.clip(cosang, -1, 1)) < np.pi - BONE_MIN)
    gated = (kab & (gap > GAP_MIN)) | bone_ok
    kappa = np.hypot(info['twist_sc'][..., 0], info['twist_sc'][..., 1]) / np.maximum(np.linalg.norm(A, axis=(-1, -2)), 1e-300)
    cond = np.where(kind == 2, np.minimum(kappa / KAPPA_REF, 1.0), 1.0)  # (Kabsch pairs: 1 — they are selected by gap)
    err = lambda R: np.abs(R - G64).max((-1, -2)) * cond  # noqa: E731
    e, e32, df, df32 = err(G), err(G32), deficit(G), deficit(G32)
    sel = lambda x, m: float(np.where(m, x, 0).max())  # noqa: E731
    pairs = lambda m, x, y: [(int(b), int(j), float(x[b, j]), float(y[b, j])) for b, j in zip(*np.nonzero(m))]  # noqa: E731
    Go = G[:, own]
    # the SMPL toes (no rotation of their own, kind -1) take the feet's: parts 10 / 11 <- 7 / 8, copied bit for bit
    toes_copied = all(np.array_equal(G[:, j], G[:, j - 3]) for j in info.get('toes', np.nonzero(~own)[0]))
    return dict(
        finite=bool(np.isfinite(G).all()),
        proper=max(float(np.abs(Go @ np.swapaxes(Go, -1, -2) - np.eye(3)).max()), float(np.abs(np.linalg.det(Go) - 1).max())),
        deficit=sel(df, kab), deficit32=sel(df32, kab), dist=sel(e, gated), dist32=sel(e32, gated),
        gated_share=float(gated[:, own].mean()),
        bad_deficit=pairs(kab & (df > np.maximum(4 * df32, DEFICIT_FLOOR)), df, df32),
        bad_dist=pairs(gated & (e > np.maximum(2 * e32, gate)), e, e32), toes_copied=toes_copied,
    )


def check_rotations(name, family, fig, label, share_exempt=False):
    """Every part a proper rotation.  Per (instance, part): Kabsch parts (leaf, multi) — optimality deficit in the fp64
    covariance <= max(4 x the fp32 oracle's deficit on that pair, 1e-6 s1), and where gap > 1e-2 |G - G64| <=
    max(2 x |G32 - G64| on that pair, the stage gate); bone parts with both bones longer than 1e-3 m and no closer than
    1e-3 rad to antiparallel: the same distance gate, pair by pair, scaled by the twist's conditioning where that is
    below KAPPA_REF (see there: bone parts need this, Kabsch parts have gap > 1e-2).  Unmasked families: at least 90 % of the pairs under
    a distance gate (``share_exempt``: a combination stage_chain_util.SHARE_EXEMPT names, with its measured share;
    every other gate holds for it pair by pair).  The printed family maxima are records, not gates."""
    print(f'[rotations {label}] {name:8s} {family:9s} proper {fig["proper"]:.1e} deficit {fig["deficit"]:.2e} (fp32 oracle '
          f'{fig["deficit32"]:.2e}) |G - G64| {fig["dist"]:.2e} (fp32 oracle {fig["dist32"]:.2e}) gated {fig["gated_share"]:.3f}'
          f' misses {len(fig["bad_deficit"])} / {len(fig["bad_dist"])}')
    assert fig['finite'], (name, family)
    assert fig['proper'] < P.PROPER_TOL, (name, family, fig)
    assert not fig['bad_deficit'], (name, family, fig['bad_deficit'])
    assert not fig['bad_dist'], (name, family, fig['bad_dist'])
    assert fig['toes_copied'], (name, family)
    if family in UNMASKED and not share_exempt:
        assert fig['gated_share'] >= MIN_GATED, (name, family, fig)


# ---- the shape solve --------------------------------------------------------------------------------------------------
SOLVE_CASES = (  # (tag, beta_regularizer, weights, add_mean)
    ('reg1', 1.0, False, False), ('reg0', 0.0, False, False), ('reg1_w', 1.0, True, False), ('reg0_w_mean', 0.0, True, True))


def solve_weights(fam, V, J, seed=7):
    """The family's own weights, else random 0/1 vertex masks times [0.5, 1.5) with one joint at 0."""
    if fam['vw'] is not None:
        return fam['vw'], fam['jw']
    rs = np.random.RandomState(seed)
    jw = (rs.rand(B, J) + 0.5).astype(np.float32)
    jw[:, J // 2] = 0
    return ((rs.rand(B, V) < 0.7) * (rs.rand(B, V) + 0.5)).astype(np.float32), jw


def oracle_solve(of, fam, G, reg, vw, jw):
    dt = of.m.dtype
    tv, tj, mean = centred(dt, fam['tv'], fam['tj'])
    w = lambda a: None if a is None else np.asarray(a, dt)  # noqa: E731
    r = of.fit_shape(np.asarray(G, dt), tv, tj, w(vw), w(jw), reg, 0.0)
    return {k: np.asarray(r[k], np.float64) for k in ('shape_betas', 'trans', 'vertices', 'joints')}, mean.astype(np.float64)


def check_solve(name, family, tag, ours, r32, r64, mean64, add_mean, label, rows=None):
    """Row by row against the fp64 solve: the mesh and the joints as ``vertices - trans`` / ``joints - trans`` (which do
    not depend on the mean the entry point centred with) 1e-4 m, betas 3e-4, trans 1e-5 — the gates of
    test_fit_vs_oracle, each max(gate, 2 x the fp32 oracle's distance on that row).  One relaxation: the translation of
    the instance 1000 m away (family 'far', row FAR_ROW) is judged relative to max(1, |target mean|) — the fp32 mean it is
    measured from, and with add_mean the translation itself, round at 6e-8 |mean| a coordinate.  ``add_mean`` adds the
    target mean to trans alone (smplfit.h).  ``rows``: the row of the references each of our rows is compared with
    (default: the same row)."""
    o = {k: np.asarray(v, np.float64) for k, v in ours.items()}
    assert all(np.isfinite(v).all() for v in o.values()), (name, family, tag)
    rows = np.arange(B) if rows is None else np.asarray(rows)
    a32, a64 = ({k: v[rows] for k, v in r.items()} for r in (r32, r64))
    mean = mean64[rows]
    scale = np.where((rows == FAR_ROW) & (family == 'far'), np.maximum(1.0, np.abs(mean).max(-1)), 1.0)
    o_trans = o['trans'] - (mean if add_mean else 0)  # back in the centred frame
    # with add_mean the far row's vertices stay relative to the fp32 mean the kernel centred with while its trans is
    # absolute: their difference carries that mean's rounding (6e-5 m at 1000 m), so that one row is anchored at its own
    # root joint instead (equally independent of the mean); its trans is judged by the trans gate
    far = (scale > 1) & bool(add_mean)
    anchor = lambda r, tr: np.where(far[:, None], r['joints'][:, 0], tr)  # noqa: E731
    rel_pos = lambda r, k, tr: r[k] - anchor(r, tr)[:, None]  # noqa: E731
    l2 = lambda a, b: np.linalg.norm(a - b, axis=-1).max(1)  # noqa: E731
    per_row = dict(
        mesh=(l2(rel_pos(o, 'vertices', o_trans), rel_pos(a64, 'vertices', a64['trans'])),
              l2(rel_pos(a32, 'vertices', a32['trans']), rel_pos(a64, 'vertices', a64['trans'])), MESH_GATE),
        joints=(l2(rel_pos(o, 'joints', o_trans), rel_pos(a64, 'joints', a64['trans'])),
                l2(rel_pos(a32, 'joints', a32['trans']), rel_pos(a64, 'joints', a64['trans'])), MESH_GATE),
        betas=(np.abs(o['shape_betas'] - a64['shape_betas']).max(1), np.abs(a32['shape_betas'] - a64['shape_betas']).max(1), BETA_GATE),
        trans=(np.abs(o_trans - a64['trans']).max(1) / scale, np.abs(a32['trans'] - a64['trans']).max(1) / scale, TRANS_GATE),
    )
    fig = {k: float(v[0].max()) for k, v in per_row.items()}
    fig.update({k + '32': float(v[1].max()) for k, v in per_row.items()})
    print(f'[solve {label}] {name:8s} {family:9s} {tag:11s} ' +
          ' '.join(f'{k} {fig[k]:.2e} ({fig[k + "32"]:.2e})' for k in ('mesh', 'joints', 'betas', 'trans')))
    for k, (e, e32, gate) in per_row.items():
        bad = np.nonzero(e > np.maximum(gate, 2 * e32))[0]
        assert not len(bad), (name, family, tag, k, [(int(i), float(e[i]), float(e32[i])) for i in bad])
    return fig
