"""The stages of BodyFitter.fit_with_known_shape, one at a time, against the fp64 oracle of that stage alone — the
counterpart of tests/stage_chain_util.py for the entry point whose kernels no fit reaches: k_fill_shape, the posed pass
from a rest or warm pose, k_regress_joints(_bm) into ws.rjreg, the alignment (k_scale_trans; k_align_partial_bm<1|2, W> +
k_align_finish with its substitution reference <- scale * reference + trans) and the refinement with RefineArgs::scaled.
Plain numpy; used by tests/test_known_shape_chain_host.py (the host emulation standing in for the device) and
tests/test_gpu_known_shape_chain.py.

Three calls expose every stage, each made with and without scale_fit:
  K1   num_iter=1, final_adjust_rots=False   orientations = the first rotation pass (R1); trans / scale_corr = the
                                             alignment at it (T1)
  K1F  num_iter=1, final_adjust_rots=True    adds exactly the refinement (F); trans / scale_corr stay K1's bits
  K2   num_iter=2, final_adjust_rots=False   adds exactly the second rotation pass (R2) and the alignment at it (T2)
and each stage is compared with the oracle function of that stage (fit_global_rotations, fit_scale_and_translation,
fit_global_rotations_dependent, called as OracleFitter.fit_with_known_shape calls them) evaluated AT THE OUTPUT OF THE
STAGE BEFORE of the build under test: nothing is amplified across stages.  The model is posed there by the oracle's
forward in the reference's own dtype with the given betas and kid factor.

Rotations are judged by the gates of stage_util / stage_chain_util unchanged (properness, optimality deficit in the fp64
covariance, distance under max(2 x the fp32 oracle on that pair, dist_gate) with the bone factor, F and R2 as delta
rotations, toes as bit copies; the share condition under the exemptions listed HERE).  The alignment is judged row by
row: trans (with the target mean, as the entry point returns it) and scale_corr each under max(ALIGN_GATE, 2 x the fp32
oracle on that row) — 1e-5 is the project's gate on a fit's translation (stage_util.TRANS_GATE) and on scale_corr
(util.check_known_shape); the row 1000 m away relative to max(1, |target mean|), as stage_util.check_solve judges it."""

import numpy as np

import stage_chain_util as C
import stage_util as S
import util

O = util.O
CALLS = (dict(num_iter=1, final_adjust_rots=False), dict(num_iter=1, final_adjust_rots=True),
         dict(num_iter=2, final_adjust_rots=False))
ALIGN_GATE = 1e-5
TARGET_SCALES = np.linspace(0.6, 1.6, S.B).astype(np.float32)  # per source row, vertices and joints alike
KID = np.linspace(0.0, 1.0, S.B).astype(np.float32)            # per source row

# (model, family, step) -> the share of (instance, part) pairs the fp64 oracle ALONE puts under a distance gate, where
# that is below stage_util.MIN_GATED: exempt from the share condition and from nothing else.  By name only: the plain
# case, the scaled refinement and every option of a family stand under one entry.  Measured by
# tests/test_known_shape_chain_host.py, which fails when a combination not listed here falls below the cap or a listed
# one no longer does.  'mirror' at the refinement: as stage_chain_util.SHARE_EXEMPT — the delta covariance of an
# adjustable part of the reflected target is itself close to a reflection.
SHARE_EXEMPT = {
    ('smpl', 'mirror', 'F'): 0.5375,
    ('smplxfat', 'mirror', 'F'): 0.4125,
    ('smpl_w6', 'mirror', 'F'): 0.55,
}


def family_betas(om64, fams, seed=0):
    """name -> the (B, S) betas each family of stage_util.families(seed) was posed with: the known shape of its
    targets.  families() does not return them, so its draws are replayed here; the replay is pinned by posing 'betas5'
    (the last draw that matters) again, bit for bit."""
    rs = np.random.RandomState(seed)
    B, J, Sn, V = S.B, om64.J, om64.S, om64.V
    betas, trans = rs.randn(B, Sn) * 0.5, rs.randn(B, 3)
    rs.randn(B, V, 3)                                   # hard_pose: its (zero) noise
    for _ in range(2):                                  # pose1, the base of mirror and the masked families
        rs.randn(B, 3 * J), rs.randn(B, V, 3)
    pose5, betas5 = rs.randn(B, 3 * J) * 0.3, rs.choice([-5.0, 5.0], (B, Sn))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    fw = util.forward64(om64, pose_rotvecs=f32(pose5), shape_betas=f32(betas5), trans=f32(trans))
    assert np.array_equal(f32(fw['vertices']), fams['betas5']['tv']), 'the draws of stage_util.families have moved'
    out = {k: f32(betas) for k in fams}
    out['betas5'] = f32(betas5)
    return out


class Case(C.Case):
    """One family with the options of the three calls.  ``weights``: None, 'vj' (both: weighted in the rotations and in
    the alignment), 'v' (vertex weights alone: with target joints weighted in the rotations and UNWEIGHTED in the
    alignment, without them weighted in both) or 'j' (joint weights alone: the same); ``warm``: initial_pose_rotvecs of
    stage_chain_util.warm_start; ``kid``: the per-row kid factor KID; ``scaled``: the family's target scaled per source
    row by TARGET_SCALES, so that scale_corr is gated at something other than 1."""

    def __init__(self, family, joints=True, weights=None, warm=False, kid=False, scaled=False):
        super().__init__(family, joints=joints, weights=weights)
        self.warm, self.kid, self.scaled = bool(warm), bool(kid), bool(scaled)

    def inputs(self, fam):
        w = self.weights or ''
        s = TARGET_SCALES[:, None, None] if self.scaled else np.float32(1.0)
        return dict(tv=np.ascontiguousarray(fam['tv'] * s, np.float32),
                    tj=np.ascontiguousarray(fam['tj'] * s, np.float32) if self.joints else None,
                    vw=fam['vw'] if 'v' in w else None, jw=fam['jw'] if 'j' in w else None)

    @property
    def tag(self):
        return (('j' if self.joints else 'nj') + (f' w={self.weights}' if self.weights else '') +
                (' warm' if self.warm else '') + (' kid' if self.kid else '') + (' x0.6-1.6' if self.scaled else ''))

    @property
    def id(self):
        return f'{self.family}-{self.tag.replace(" ", "_")}'


def cases(name):
    """Every family and option of the chain on one model: the unmasked families plain; the masked ones under the three
    weight settings; joints omitted (the regressed path) plain and with 'mask01' vertex weights; a warm start; scaled
    targets with joints, without them and with both weights; the kid factor (not on smpl_w6: the host emulation has no
    instance for 11 shape unknowns with KW = 8, and the case is the same on host and device)."""
    return ([Case(f) for f in S.UNMASKED] + [Case(f, weights=w) for f in S.MASKED for w in ('vj', 'v', 'j')] +
            [Case('pose1', joints=False), Case('mask01', joints=False, weights='v'), Case('pose1', warm=True),
             Case('pose1', scaled=True), Case('hard_pose', joints=False, scaled=True),
             Case('part_off', weights='vj', scaled=True)] + ([Case('betas5', kid=True)] if name != 'smpl_w6' else []))


def known(c, case):
    """dict(betas, kid, pose0) of a case: the known shape of its family, KID or None, the warm start's pose or None
    (``c``: a stage_util.host_setup dict; computed once, shared, read only)."""
    if 'ks_betas' not in c:
        c['ks_betas'] = family_betas(c['om64'], c['fams'])
    if case.warm and ('ks_warm', case.family) not in c:
        c['ks_warm', case.family] = C.warm_start(c['of64'], c['fams'][case.family])['initial_pose_rotvecs']
    return dict(betas=c['ks_betas'][case.family], kid=KID if case.kid else None,
                pose0=c['ks_warm', case.family] if case.warm else None)


class Refs(C.Refs):
    """The references of one (model, case) in one dtype, memoised per state as stage_chain_util.Refs memoises them."""

    def __init__(self, of, fam, case, betas, kid=None, pose0=None):
        self.of, self.dt, self.case = of, of.m.dtype, case
        inp = case.inputs(fam)
        self.tv, self.tj, self.mean = S.centred(self.dt, inp['tv'], inp['tj'])
        w = lambda a: None if a is None else np.asarray(a, self.dt)  # noqa: E731
        self.vw, self.jw, self.betas, self.kid, self.pose0 = w(inp['vw']), w(inp['jw']), w(betas), w(kid), w(pose0)
        self._memo = {}

    def _R1(self):
        """(G, info, prev): the first pass at the rest pose or at the warm start, whose orientations it is composed with."""
        of, m = self.of, self.of.m
        pose0 = np.zeros((self.tv.shape[0], 3 * m.J), self.dt) if self.pose0 is None else self.pose0
        f = m.forward(pose_rotvecs=pose0, shape_betas=self.betas, kid_factor=self.kid)
        R, info = of.fit_global_rotations(self.tv, self.tj, f['vertices'], f['joints'], self.vw, self.jw, return_cov=True)
        return R @ f['orientations'], info, None if self.pose0 is None else f['orientations']

    def posed(self, G):
        """The oracle's forward at the rotations ``G`` with the known shape, zero translation."""
        return self._once('posed', (G,), lambda: self.of.m.forward(glob_rotmats=np.asarray(G, self.dt),
                                                                   shape_betas=self.betas, kid_factor=self.kid))

    def T(self, G, scale):
        """(scale_corr (B,) or None, trans + mean (B, 3)) of the alignment at ``G``, rounded as the oracle returns them."""
        return self._once('T', (G, np.array(scale)), lambda: self._T(G, scale))

    def _T(self, G, scale):
        f = self.posed(G)
        sc, tr = O.fit_scale_and_translation(self.tv, f['vertices'], self.tj, f['joints'], self.vw, self.jw, scale)
        return (None if sc is None else np.asarray(sc, np.float64)), np.asarray((tr + self.mean).astype(self.dt), np.float64)

    def F(self, G, trans, scale):
        """(G, info, prev) of the refinement at the state (``G``, ``trans`` WITH the mean, ``scale`` (B,) or None)."""
        state = (G, trans) + (() if scale is None else (scale,))
        return self._once('F', state, lambda: self._F(G, trans, scale))

    def _F(self, G, trans, scale):
        m, dt = self.of.m, self.dt
        G, f = np.asarray(G, dt), self.posed(G)
        tr = (np.asarray(trans, dt) - self.mean).astype(dt)
        nb = min(self.betas.shape[1], m.S)
        rest = m.J_template + np.einsum('jcs,bs->bjc', m.J_shapedirs[:, :, :nb], self.betas[:, :nb])
        if self.kid is not None:
            rest = rest + m.kid_J_shapedir[None] * self.kid.reshape(-1, 1, 1)
        sc = None if scale is None else np.asarray(scale, dt)[:, None, None]
        sv, sj = (f['vertices'], f['joints']) if sc is None else (sc * f['vertices'], sc * f['joints'])
        R, info = self.of.fit_global_rotations_dependent(
            self.tv, self.tj, (sv + tr[:, None]).astype(dt), (sj + tr[:, None]).astype(dt), self.vw, self.jw, G, None, tr,
            rest_joints=rest.astype(dt), scale_corr=sc, return_cov=True)
        return R, info, G

    def R2(self, G):
        """(G, info, prev) of the second rotation pass at ``G``."""
        return self._once('R2', (G,), lambda: self._R2(G))

    def _R2(self, G):
        G, f = np.asarray(G, self.dt), self.posed(G)
        R, info = self.of.fit_global_rotations(self.tv, self.tj, f['vertices'], f['joints'] if self.tj is not None else None,
                                               self.vw, self.jw, return_cov=True)
        return R @ G, info, G


def refs(c, case):
    """(fp64, fp32) Refs of a case, kept in ``c``: every build, route and batch under test shares their memo."""
    key = ('ks_refs', case.id)
    if key not in c:
        k = known(c, case)
        c[key] = tuple(Refs(of, c['fams'][case.family], case, k['betas'], k['kid'], k['pose0']) for of in (c['of64'], c['of32']))
    return c[key]


def check_align(name, case, step, out, a32, a64, mean64, label, rows):
    """The alignment of one call (``out``: its result dict) row by row against (scale, trans + mean) of both oracles."""
    far = (rows == S.FAR_ROW) & (case.family == 'far')
    rel = np.where(far, np.maximum(1.0, np.abs(mean64[rows]).max(-1)), 1.0)
    e = np.abs(np.asarray(out['trans'], np.float64) - a64[1][rows]).max(1) / rel
    e32 = np.abs(a32[1] - a64[1]).max(1)[rows] / rel
    fig = dict(trans=float(e.max()), trans32=float(e32.max()))
    per_row = dict(trans=(e, e32))
    assert ('scale_corr' in out) == (a64[0] is not None), (name, case.family, step)
    if a64[0] is not None:
        es, es32 = np.abs(np.asarray(out['scale_corr'], np.float64) - a64[0][rows]), np.abs(a32[0] - a64[0])[rows]
        fig.update(scale=float(es.max()), scale32=float(es32.max()))
        per_row['scale_corr'] = (es, es32)
    print(f'[alignment {label} {step} {case.tag}] {name:8s} {case.family:9s} ' +
          ' '.join(f'{k} {v[0].max():.2e} ({v[1].max():.2e})' for k, v in per_row.items()))
    for k, (x, x32) in per_row.items():
        assert np.isfinite(x).all(), (name, case.family, step, k)
        bad = np.nonzero(x > np.maximum(ALIGN_GATE, 2 * x32))[0]
        assert not len(bad), (name, case.family, case.tag, step, k, [(int(i), float(x[i]), float(x32[i])) for i in bad])
    return fig


def check_rotations(name, case, step, ours, r32, r64, label, rows):
    """One rotation stage as stage_chain_util.check_step_rotations judges it (same figures, same gates, the parts a
    refinement does not own keep their bits), with the share condition under THIS chain's exemptions.  A failing gate
    carries the step's figures on the AssertionError (``.fig``)."""
    (G64, info, prev), G32 = r64, r32[0]
    info = {k: (v[rows] if isinstance(v, np.ndarray) and v.ndim > 1 else v) for k, v in info.items()}
    if step == 'F':
        adj = info['kind'] >= 0
        info['toes'] = [j for j in (10, 11) if j < len(adj) and not adj[j] and adj[j - 3]]
        kept = [j for j in np.nonzero(~adj)[0] if j not in info['toes']]
        assert np.array_equal(ours[:, kept], np.asarray(prev[rows][:, kept], ours.dtype)), (name, case.family, 'unadjusted parts changed')
    fig = S.rotation_figures(ours, G32[rows], G64[rows], info, S.dist_gate(name), prev=None if prev is None else prev[rows])
    try:
        S.check_rotations(name, case.family, fig, f'{label} {step} {case.tag}', share_exempt=(name, case.family, step) in SHARE_EXEMPT)
    except AssertionError as e:
        e.fig = fig
        raise
    return fig


def check_chain(name, c, case, outs, label, rows=None, defer=()):
    """The five stages of the six calls ``outs`` — {scale_fit: (K1, K1F, K2)}, result dicts as numpy arrays — under the
    criteria above.  ``c``: stage_util.host_setup(name); ``rows``: the source row (of the family's B) of each row of the
    batch — every source row must occur, and the references are built at the state of its first occurrence.  Returns
    step -> figures; the steps of the scale_fit calls carry the suffix '/s' (R1 / R2 do not depend on scale_fit: the
    orientations of K1 and K2 must be the same bits with and without it).  ``defer``: steps whose AssertionError is not
    raised here but returned under figs['deferred'][step], as stage_chain_util.check_chain defers them — every other gate
    of the case still holds, and the caller raises the deferred one in a test of its own."""
    r64, r32 = refs(c, case)
    rows = np.arange(len(outs[False][0]['trans'])) if rows is None else np.asarray(rows)
    first = [int(np.nonzero(rows == k)[0][0]) for k in range(S.B)]
    figs = {'deferred': {}}

    def step(key, check, *a):
        try:
            figs[key] = check(name, case, key.split('/')[0], *a)
        except AssertionError as e:
            if key not in defer:
                raise
            figs['deferred'][key] = e
            if hasattr(e, 'fig'):
                figs[key] = e.fig

    for i in (0, 2):
        assert np.array_equal(outs[False][i]['orientations'], outs[True][i]['orientations']), (name, case.family, CALLS[i])
    k1, _, k2 = outs[False]
    G1, G2 = k1['orientations'][first], k2['orientations'][first]
    step('R1', check_rotations, k1['orientations'], r32.R1(), r64.R1(), label, rows)
    step('R2', check_rotations, k2['orientations'], r32.R2(G1), r64.R2(G1), label, rows)
    for sf in (False, True):
        o1, o2, o3 = outs[sf]
        sfx, lab = ('/s', label + ' scale_fit') if sf else ('', label)
        step('T1' + sfx, check_align, o1, r32.T(G1, sf), r64.T(G1, sf), r64.mean, lab, rows)
        for k in ('trans', 'scale_corr'):  # the refinement changes rotations only
            assert (k in o1) == (k in o2) and (k not in o1 or np.array_equal(o1[k], o2[k])), (name, case.family, k)
        state = (G1, o1['trans'][first], o1['scale_corr'][first] if sf else None)
        step('F' + sfx, check_rotations, o2['orientations'], r32.F(*state), r64.F(*state), lab, rows)
        step('T2' + sfx, check_align, o3, r32.T(G2, sf), r64.T(G2, sf), r64.mean, lab, rows)
    return figs


def gated_shares(name, case, figs):
    """(model, family, step) -> the lowest share of the case's rotation steps (the plain and the scale_fit refinement
    stand under one name)."""
    out = {}
    for k, fig in figs.items():
        if k[0] in 'RF' and k != 'deferred':
            key = (name, case.family, k.split('/')[0])
            out[key] = min(out.get(key, 1.0), fig['gated_share'])
    return out


def host_chain(md, kind, c, case, H):
    """The six calls of a case through the host emulation ``H`` (tests/hostemu_util.py), B = stage_util.B."""
    inp, k = case.inputs(c['fams'][case.family]), known(c, case)
    keys = ('orientations', 'trans', 'scale_corr')
    call = lambda sf, o: {kk: v for kk, v in H.fit_known_shape(  # noqa: E731
        md, kind, k['betas'], inp['tv'], inp['tj'], inp['vw'], inp['jw'], kid_factor=k['kid'],
        initial_pose_rotvecs=k['pose0'], scale_fit=sf, **o).items() if kk in keys}
    return {sf: tuple(call(sf, o) for o in CALLS) for sf in (False, True)}
