"""The general path (kernels_gen.inc) at every launch shape: which branch a count of unknowns reaches, the models and
fp64 / fp32 oracles of a case, and the references of one shape solve with the kid and the scale unknowns.  Plain numpy;
used by tests/test_gpu_general_shapes.py and, for the branch tables and the oracle's own gated shares, by
tests/test_general_shapes_host.py.  Targets and criteria are stage_util's, unchanged.

``launch_rules`` restates the host-side launch rules of kernels_gen.inc in Python (they are plain integer arithmetic):
the library reports no per-call route, so this table is what the tests can know about the instantiation a count takes;
the CPU test pins it at the thresholds the source states, the GPU tests show by the bits that SMPLFIT_GEN_MFMA switched
the accumulate form."""

import numpy as np

import stage_util as S
import util
from smplfitter_amd import modelio

# name (directory under the model root) -> (model kind, joints); all with four skinning weights per vertex (KW = 4)
MODELS = {'smpl_b400': ('smpl', 24), 'smpl_b100': ('smpl', 24), 'smplx_fat_b300': ('smplx', 55)}
KW = 4

SWEEP_LISTED = (17, 27, 30, 59, 60, 88, 89, 128, 129, 155, 156, 176, 177, 252, 253, 315, 316)
SWEEP_STAGING = (20, 21, 28, 392, 393, 400)  # both sides of the staging flips the listed counts miss (sweep_branches)
SWEEP = tuple(sorted(SWEEP_LISTED + SWEEP_STAGING))
ENTRY_COUNTS = (30, 156)              # the three ways weights enter a solve
SCALE_COUNTS = (27, 30, 60, 156, 316)  # the scale unknown: column t straddles or fills a block of the matrix-core form
ROWS = 4                              # instances of a sweep case, and of every case of 300 unknowns or more
# the stage harness — (model, betas) -> families of stage_util: every family up to 64 unknowns, 'pose1' and one masked
# family at 300 (four rows: an fp64 solve of 300 unknowns on eight rows of the 55-joint model takes ten seconds)
ALL_FAMILIES = S.UNMASKED + S.MASKED
STAGE_MODELS = {('smpl_b400', 32): ALL_FAMILIES, ('smpl_b400', 300): ('pose1', 'part_off'),
                ('smplx_fat_b300', 20): ALL_FAMILIES, ('smplx_fat_b300', 64): ALL_FAMILIES,
                ('smplx_fat_b300', 300): ('pose1', 'part_off')}


def _jd_row(n):
    return (n + 3) // 4 * 4


def _jd_stride(n):  # sf_stages.h:22-24
    x = 12 + 3 * _jd_row(n)
    return x if x % 8 == 4 else x + 4


def launch_rules(n, J, B=1, kw=KW):
    """The branches ``n`` shape unknowns (betas + kid) reach on a model of ``J`` joints at batch ``B``.

    accum_*  k_gen_accum (SMPLFIT_GEN_MFMA=0): threads (gen_accum_threads, kernels_gen.inc:29), vertices per tile
             (gen_tile_vertices, :25), passes over the 4 x 4 block pairs (:82-83), joint rows staged in LDS
             (gen_accum_stage_joints, :39-42)
    mfma_*   k_gen_accum_mfma: 32-column blocks nb of the n + 5 columns (gen2_nb, :460), waves x blocks per wave
             (gen2_nw / gen2_nbw, :465-466), workgroups per instance (gen2_groups, :469-472), staged joint rows
             (gen2_stage_joints, :484-487), and where the five columns b | 1x 1y 1z | t sit: 'inside' one block, 'fill'
             (its last five columns: n % 32 == 27) or 'straddle' (n % 32 in 28..31: store_entry, :665-685); waves
             without a block (nblk == 0, :619) and waves with fewer than their NBW blocks, whose spare accumulators
             repeat the last one (:539-553)
    lbs_ni   instances per workgroup of k_gen_lbs (gen_lbs_ni, :267) and its dynamic LDS in bytes (gen_lbs_lds, :268-271)"""
    s4 = (n + 3) & ~3
    tile = 32 if n <= 128 else 8
    threads = 64 if n <= 88 else 256
    rows = 3 * tile
    jrows = J * _jd_stride(n) * 4
    accum_base = (rows * s4 + 2 * rows + tile * 12 + 2 * tile * kw) * 4
    nb4 = s4 // 4
    npair = nb4 * (nb4 + 1) // 2
    nb = (n + 5 + 31) // 32
    nw = 4 if nb <= 2 else 16 if nb <= 5 else 8
    nbw = 1 if nb <= 5 else 7
    tv2 = 8 if nbw >= 4 else 32
    sv2 = 64 if tv2 == 8 else 128
    mfma_base = (3 * tv2 * 32 * (nb | 1) + sv2 * 21 + 2 * sv2 * kw) * 4
    ni = 4 if n >= 48 and B >= 2048 else 1
    tri = nb * (nb + 1) // 2
    groups = -(-tri // (nw * nbw))
    per_wg = -(-tri // groups)
    per_wave = -(-per_wg // nw)
    first = [g * per_wg + w * per_wave for g in range(groups) for w in range(nw)]  # :524-527
    end = [min((g + 1) * per_wg, tri) for g in range(groups) for w in range(nw)]
    nblk = [max(0, min(min(f + per_wave, e) - f, nbw)) for f, e in zip(first, end)]
    r = n % 32
    return dict(
        accum_threads=threads, accum_tile=tile, accum_passes=-(-npair // (threads * 4)),
        accum_staged=accum_base + jrows <= (20 if threads == 64 else 150) * 1024,
        mfma_nb=nb, mfma_waves=nw, mfma_blocks_per_wave=nbw, mfma_groups=groups,
        mfma_idle_waves=sum(k == 0 for k in nblk), mfma_short_waves=sum(0 < k < nbw for k in nblk),
        mfma_blocks_covered=sum(nblk) == tri,
        mfma_staged=mfma_base + jrows <= (160 if nw >= 8 else 52) * 1024,
        mfma_extra='fill' if r == 27 else 'straddle' if r > 27 else 'inside',
        lbs_ni=ni, lbs_lds=ni * (n + J * 12 + 4 * J * 16 + 4) * 4)


def sweep_branches():
    """count -> launch_rules on the SMPL skeleton (J = 24, KW = 4) for every count of SWEEP and its kid neighbour n + 1.

    What each listed count is there for (kernels_gen.inc; 'kid' is the same count with the kid unknown, n + 1):
      17         one block of 32 (n + 5 = 22), 4 waves x 1; both forms stage the joint rows
      20 | 21    k_gen_accum's one-wave form stops staging the joint rows (20 KB limit, :41)             [added]
      27         b | 1 | t fill the first block exactly (n % 32 == 27); kid: 28, they straddle into a second block
      27 | 28    k_gen_accum_mfma stops staging (52 KB limit of the 4-wave shape, :486): nb 1 -> 2       [28 added]
      30         the extra columns straddle blocks 0 and 1 (30, 31 | 32, 33, 34)
      59 | 60    nb 2 -> 3: 4 waves -> 16 waves x 1 block (:465), staged again (160 KB limit); 59 = 32 + 27 fills, 60 straddles
      88 | 89    k_gen_accum 64 -> 256 threads (:29), staged again (150 KB limit)
      128 | 129  k_gen_accum tile of 32 -> 8 vertices (:25)
      155 | 156  nb 5 -> 6: 16 x 1 -> 8 waves x 7 blocks, tile 32 -> 8 vertices (:465-467); 155 = 4 * 32 + 27 fills, 156 straddles
      176 | 177  k_gen_accum 1 -> 2 passes (:82-83: 1035 block pairs > 1024)
      252 | 253  k_gen_accum 2 -> 3 passes; 252 % 32 == 28 and 253 % 32 == 29 straddle
      315 | 316  nb 10 -> 11: 66 blocks > 56, gridDim.y 1 -> 2 (:469-472); 315 = 9 * 32 + 27 fills, 316 straddles;
                 k_gen_accum in 4 passes (since 309)
      392 | 393  k_gen_accum stops staging the joint rows (150 KB limit)                                  [added]
      400 | kid  k_gen_accum_mfma stops staging (160 KB limit) at 401 unknowns: the kid fitter at 400; 6 passes  [added]
    Waves without a block (nblk == 0) at every count up to 177 (one block on four waves at 17..27, three at 28..59, six
    on sixteen waves at 60..91, fifteen at 124..155, 21 as 7 x 3 on eight waves from 156) and at 316 (two groups of 33
    blocks as 6 x 5 + 3: the last wave of each is idle); waves with fewer than seven blocks, whose spare accumulators
    repeat their last block, at every count of the 8 x 7 shape (launch_rules: mfma_idle_waves / mfma_short_waves)."""
    return {n: dict(plain=launch_rules(n, 24), kid=launch_rules(n + 1, 24)) for n in SWEEP}


# ---- models and oracles ------------------------------------------------------------------------------------------
_cache = {}


def load_md(root, name, nb):
    return modelio.load_model(MODELS[name][0], 'neutral', model_root=f'{root}/{name}', num_betas=nb)


def setup(root, name, nb, transient=False):
    """Oracles (fp64 / fp32, plain and with the kid unknown), the families of stage_util and a cache of references for
    ``name`` at ``nb`` betas: computed once, shared, read only.  ``transient``: keep one such entry at a time (the sweep:
    an fp64 copy of 400 shape directions is 66 MB)."""
    key = (name, nb)
    if key not in _cache:
        if transient:
            for k in [k for k, v in _cache.items() if v['transient']]:
                del _cache[k]
        kind = MODELS[name][0]
        md = load_md(root, name, nb)
        om64, of64 = util.make_oracle(md, kind, np.float64)
        om32, of32 = util.make_oracle(md, kind, np.float32)
        _cache[key] = dict(name=name, nb=nb, kind=kind, md=md, om64=om64, of64=of64, om32=om32, of32=of32, transient=transient,
                           kid64=util.O.OracleFitter(om64, enable_kid=True), kid32=util.O.OracleFitter(om32, enable_kid=True),
                           fams=S.families(om64, of64), refs={})
    return _cache[key]


def rotations(c, family):
    """((G64, info), G32): the oracles' first rotation pass on a family (stage_util.oracle_rotations), cached."""
    key = ('rot', family)
    if key not in c['refs']:
        fam = c['fams'][family]
        c['refs'][key] = (S.oracle_rotations(c['of64'], fam), S.oracle_rotations(c['of32'], fam)[0])
    return c['refs'][key]


def head(fam, rows):
    """The first ``rows`` instances of a family."""
    return {k: (None if v is None else v[:rows]) for k, v in fam.items()}


def scaled_targets(fam, factor=1.1):
    """The family with its targets scaled (a target that really is a scaled body, as util.scale_inputs)."""
    f = np.float32(factor)
    return dict(fam, tv=fam['tv'] * f, tj=None if fam['tj'] is None else fam['tj'] * f)


def _mesh(om64, G, x, kid, scale_mode):
    """vertices / joints of a scaled solve's unknowns: no entry point returns a mesh with a scale (smplfit.h), so every
    side is evaluated by the fp64 forward at the given rotations — linear in the unknowns, as the solve's own mesh
    (scale_fit: at shape / scale, oracle fit_shape)."""
    nb = om64.S
    betas = np.asarray(x['shape_betas'], np.float64)[:, :nb]
    k = np.asarray(x['kid_factor'], np.float64) if kid else None
    if scale_mode == 2:
        sc = np.asarray(x['scale_corr'], np.float64)
        betas, k = betas / sc[:, None], (None if k is None else k / sc)
    fw = util.forward64(om64, glob_rotmats=np.asarray(G, np.float64), shape_betas=betas, trans=np.asarray(x['trans'], np.float64),
                        kid_factor=k)
    return fw['vertices'], fw['joints']


def solve_view(c, x, G, kid=False, scale_mode=0):
    """A solve's result (ours or an oracle's) in the form stage_util.check_solve judges: the kid factor and the scale
    correction are further columns of 'shape_betas' — they are unknowns of the same system, held to the same gate —
    and a scaled solve gets its mesh from ``_mesh``."""
    cols = [np.asarray(x['shape_betas'], np.float64)]
    if kid:
        cols.append(np.asarray(x['kid_factor'], np.float64).reshape(-1, 1))
    if scale_mode:
        cols.append(np.asarray(x['scale_corr'], np.float64).reshape(-1, 1))
        v, j = _mesh(c['om64'], G, x, kid, scale_mode)
    else:
        v, j = x['vertices'], x['joints']
    return dict(shape_betas=np.concatenate(cols, 1), trans=np.asarray(x['trans'], np.float64), vertices=np.asarray(v, np.float64),
                joints=np.asarray(j, np.float64))


def oracle_solve(c, fam, G, reg, vw, jw, kid=False, scale_mode=0, key=None):
    """(r64, r32, mean64) of one solve in the form of ``solve_view``: OracleFitter.fit_shape in fp64 and in fp32 on the
    same rotations (kid_regularizer = beta_regularizer, scale_regularizer 0, as BodyFitter._shape_solve's defaults).
    ``key``: cache the result under it."""
    if key is not None and key in c['refs']:
        return c['refs'][key]
    out = []
    for of in ((c['kid64'], c['kid32']) if kid else (c['of64'], c['of32'])):
        dt = of.m.dtype
        tv, tj, mean = S.centred(dt, fam['tv'], fam['tj'])
        w = lambda a: None if a is None else np.asarray(a, dt)  # noqa: E731
        r = of.fit_shape(np.asarray(G, dt), tv, tj, w(vw), w(jw), reg, 0.0, scale_mode=scale_mode)
        out.append(solve_view(c, r, G, kid, scale_mode))
        if dt == np.float64:
            mean64 = mean.astype(np.float64)
    res = (out[0], out[1], mean64)
    if key is not None:
        c['refs'][key] = res
    return res


def entry_weights(fam, V, J):
    """tag -> (target joints, vertex weights, joint weights): the three ways weights enter a solve (solve_weights of the
    library; reference pt/bodyfitter.py:1018-1028) — both kinds; vertex weights with the joints omitted; vertex weights
    beside joints without weights, which the reference then IGNORES in the solve (the oracle does the same)."""
    vw, jw = S.solve_weights(fam, V, J)
    return dict(vw_jw=(fam['tj'], vw, jw), vw_nojoints=(None, vw, None), vw_only=(fam['tj'], vw, None))


def oracle_gated_share(c, family):
    """The share of (instance, part) pairs under a distance gate, from the fp64 oracle alone (rotation_figures)."""
    (G64, info), G32 = rotations(c, family)
    return S.rotation_figures(G64, G32, G64, info, S.dist_gate(c['kind']))['gated_share']


def forward_floors(c, fin, fw64):
    """(vertices, joints): what fp32 alone costs a forward on the inputs ``fin`` (keyword arguments of util.forward64, whose
    fp64 result is ``fw64``), as util.forward_excess measures it.  The fp32 oracle's own excess; for the vertices also the
    rounding of the shape blend summed one term after the other in fp32 — the order any kernel with a run-time loop over
    the unknowns uses, where numpy's fp32 product sums pairwise: max over the vertices of |sum_fp32 - sum_fp64|_2 (the
    blended rotation that follows is a convex combination of rotations and does not enlarge it).  The figure
    tests/test_gpu_forward.py quotes for smpl_b300 (2.4e-6 m at 300 terms)."""
    fv, fj, _ = util.forward_errors(util.forward64(c['om32'], **fin), fw64)
    sd, betas = c['om32'].shapedirs, np.asarray(fin['shape_betas'], np.float32)
    acc = np.zeros((betas.shape[0],) + sd.shape[:2], np.float32)
    for s in range(sd.shape[2]):
        acc += sd[None, :, :, s] * betas[:, None, None, s]
    exact = np.einsum('vcs,bs->bvc', sd.astype(np.float64), betas.astype(np.float64))
    return max(fv, float(np.linalg.norm(acc - exact, axis=-1).max())), fj
