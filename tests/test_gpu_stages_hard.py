"""-m gpu: the two fit stages with entry points of their own — one rotation pass (BodyFitter._part_rotations) and one shape
solve (BodyFitter._shape_solve) — on the hard targets of tests/stage_util.py, each against the fp64 oracle of the same
operation (OracleFitter.fit_global_rotations / fit_shape) with the fp32 oracle as the floor.  One stage at a time, so that
nothing is amplified over iterations: large and near-pi part rotations, a mirrored mesh (every part covariance reflected),
betas of +-5, an instance 1000 m away, parts masked to zero weight or to two vertices, random masks, a joint at zero
weight; and a non-finite instance beside good ones.

Routes.  The rotation-pass entry point always runs the wave-per-instance kernels (route_of: rotations_only is never
batch-major), on the fine or the coarse cell tables; the shape-solve entry point runs k_gram_combine + k_shape_solve on
the fine tables and the lane = instance k_solve_bm on the coarse ones (forced at a small batch with SMPLFIT_FINE_B=0),
the accumulate kernel with weights.  k_rotations_bm / k_prologue_bm / k_refine_bm only run inside a whole fit: they are
held to the same oracles, stage by stage and on the same families, by tests/test_gpu_stage_chain.py.  Which solve
kernels ran is read from the library's launch counters (smplfit_stage_launches)."""

import numpy as np
import pytest
import torch

import stage_util as S
from smplfitter_amd import _lib
from test_gpu_parity import get_model, t, to_np

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def setup(name, model_root, golden, dev):
    """Model, oracles, families and the oracles' rotation passes of one model kind: computed once, shared, read only."""
    if name not in _cache:
        m, f = get_model(model_root, name, golden(name), dev)
        _cache[name] = dict(S.host_setup(name, model_root, golden), m=m, f=f)
    return _cache[name]


def dev_weights(fam, dev):
    return t(fam['vw'], dev), t(fam['jw'], dev)


@pytest.mark.parametrize('fine_b', [None, '0'])
@pytest.mark.parametrize('name', ['smpl', 'smplxfat', 'smpl_w6'])
def test_part_rotations_hard(name, fine_b, model_root, golden, dev, smplfit_env, capsys):
    """Every family through smplfit_part_rotations_f32 on the fine and on the coarse cell tables (SMPL, the fat-part
    SMPL-X, and smpl_w6: the KW = 8 kernels), under stage_util.check_rotations.
    Gated pair by pair; the printed family maxima are records.
    (deficit <= 7.0e-8 observed; largest distance, with the bone factor: 1.8e-3 on smplxfat 'mirror', the fp32 oracle's
    6.2e-3; 6.6e-4 on smpl_w6 'mirror' (2.7e-3), 4.3e-4 on smpl 'mirror' (2.3e-3); <= 1.1e-4 off the mirrored family; the
    same on both tables)"""
    c = setup(name, model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', fine_b)
    with capsys.disabled():
        print()
        for family in S.UNMASKED + S.MASKED:
            fam = c['fams'][family]
            vw, jw = dev_weights(fam, dev)
            G = c['f']._part_rotations(t(fam['tv'], dev), t(fam['tj'], dev), vw, jw).cpu().numpy()
            (G64, info), G32 = c['rot'][family]
            S.check_rotations(name, family, S.rotation_figures(G, G32, G64, info, S.dist_gate(name)), f'device fine_b={fine_b}')


# the rotation pass and the solve see one set of families; a masked family is solved with its own weights only
SOLVE_FAMILIES = [(name, k) for name in ('smpl', 'smplxfat', 'smpl_w6') for k in S.UNMASKED + S.MASKED]


def solve_refs(c, name, family, tag, G, reg, vw, jw):
    """The fp64 and the fp32 oracle's solve of one case: computed once, shared by the routes."""
    key = ('solve', name, family, tag)
    if key not in _cache:
        r64, mean64 = S.oracle_solve(c['of64'], c['fams'][family], G, reg, vw, jw)
        _cache[key] = (r64, S.oracle_solve(c['of32'], c['fams'][family], G, reg, vw, jw)[0], mean64)
    return _cache[key]


@pytest.mark.parametrize('fine_b', [None, '0'])
@pytest.mark.parametrize('name,family', SOLVE_FAMILIES)
def test_shape_solve_hard(name, family, fine_b, model_root, golden, dev, smplfit_env, capsys):
    """One shape solve at the fp64 oracle's rotations rounded to fp32, against fit_shape in fp64 on the same rotations:
    beta_regularizer 1 and 0, without and with weights, add_mean; on the fine tables and on the coarse ones (unweighted:
    k_solve_bm).  Every family of the rotation pass on every model kind: an unmasked family runs the four
    stage_util.SOLVE_CASES, the weighted ones with random 0/1 masks and a joint at 0 (stage_util.solve_weights); a masked
    family (a part at 0, a part cut to two vertices, a 0/1 mask, a joint at 0) runs the two weighted cases with its own
    weights — without them it is the unmasked target it was cut from.  Gates of stage_util.check_solve.
    (worst case observed, all on smplxfat: mesh 1.6e-6 m, joints 5.3e-7 m, betas 4.8e-5, trans 3.9e-7; the fp32 oracle:
    3.2e-5 m, 6.9e-6 m, 1.4e-3, 3.9e-5)"""
    c = setup(name, model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', fine_b)
    m, fam = c['m'], c['fams'][family]
    G = c['rot'][family][0][0].astype(np.float32)
    with capsys.disabled():
        print()
        for tag, reg, weights, add_mean in S.SOLVE_CASES:
            if fam['vw'] is not None and not weights:
                continue
            vw, jw = S.solve_weights(fam, m.num_vertices, m.num_joints) if weights else (None, None)
            r = to_np(c['f']._shape_solve(t(G, dev), t(fam['tv'], dev), t(fam['tj'], dev), t(vw, dev), t(jw, dev),
                                          beta_regularizer=reg, add_mean=add_mean))
            r64, r32, mean64 = solve_refs(c, name, family, tag, G, reg, vw, jw)
            S.check_solve(name, family, tag, r, r32, r64, mean64, add_mean, f'device fine_b={fine_b}')


@pytest.mark.parametrize('Bn', [63, 65])
def test_solve_bm_rows_vs_oracle(Bn, model_root, golden, dev, smplfit_env, capsys):
    """The lane = instance k_solve_bm (coarse tables forced with SMPLFIT_FINE_B=0; 64 instances a workgroup) on both
    sides of 64: a wave short of one lane, and a second workgroup of one lane.  The batch tiles the 8 targets of a
    family, every row is compared with the fp64 solve of its source row under stage_util.check_solve, and rows of the
    same source must agree bit for bit whatever their lane or workgroup.  That the coarse route was taken is shown by the
    bits: the fine tables sum in another order, so the same call without SMPLFIT_FINE_B=0 must differ somewhere; with
    SMPLFIT_SOLVE_BM=0 (k_gram_combine_bm + k_shape_solve on the same tables, sums in k_solve_bm's order by design,
    test_solve_bm_matches_two_kernels) it must not.  Which kernels solved is read from the launch counters: k_solve_bm
    and neither k_gram_combine_bm nor k_shape_solve in the 'coarse' variant, the reverse in 'coarse_two_kernels'."""
    c = setup('smpl', model_root, golden, dev)
    rows = np.arange(Bn) % S.B
    with capsys.disabled():
        print()
        for family in ('pose1', 'far'):
            fam = c['fams'][family]
            G = c['rot'][family][0][0].astype(np.float32)
            args = (t(G[rows], dev), t(fam['tv'][rows], dev), t(fam['tj'][rows], dev))
            out = {}
            for tag, env in (('fine', {}), ('coarse', dict(SMPLFIT_FINE_B='0')),
                             ('coarse_two_kernels', dict(SMPLFIT_FINE_B='0', SMPLFIT_SOLVE_BM='0'))):
                for k in ('SMPLFIT_FINE_B', 'SMPLFIT_SOLVE_BM'):
                    smplfit_env(k, env.get(k))
                torch.cuda.synchronize()
                before = _lib.stage_launches()
                out[tag] = to_np(c['f']._shape_solve(*args, beta_regularizer=1.0))
                torch.cuda.synchronize()
                ran = {k: v - before[k] for k, v in _lib.stage_launches().items()}
                if tag == 'coarse':
                    assert ran['solve_bm'] == 1 and ran['gram_combine'] == 0 and ran['shape_solve'] == 0, (tag, ran)
                elif tag == 'coarse_two_kernels':
                    assert ran['solve_bm'] == 0 and ran['gram_combine'] == 1 and ran['shape_solve'] == 1, (tag, ran)
            r64, r32, mean64 = solve_refs(c, 'smpl', family, 'reg1', G, 1.0, None, None)
            for tag in out:
                S.check_solve('smpl', family, 'reg1', out[tag], r32, r64, mean64, False, f'device B={Bn} {tag}', rows=rows)
            for k, v in out['coarse'].items():
                for src in range(S.B):
                    same = v[rows == src]
                    assert all(np.array_equal(same[0], x) for x in same[1:]), (family, k, src)
                assert np.array_equal(v, out['coarse_two_kernels'][k]), (family, k)
            differs = any(not np.array_equal(out['coarse'][k], out['fine'][k]) for k in out['coarse'])
            print(f'[route B={Bn}] {family}: coarse differs from fine in bits: {differs}')
            assert differs, (family, 'SMPLFIT_FINE_B=0 changed nothing: the coarse route (k_solve_bm) did not run')


@pytest.mark.parametrize('Bn,rows,fine_b', [(8, (3,), None), (65, (5, 63, 64), '0'), (63, (62,), '0')])
@pytest.mark.parametrize('poison', [float('nan'), float('inf')])
def test_poisoned_row(poison, Bn, rows, fine_b, model_root, golden, dev, smplfit_env):
    """One instance with NaN (or Inf) targets — inside a wave, at both sides of a wave edge, the last lane of a partly
    filled wave — beside good ones: every other row of both stages is bit-identical to the clean run, no part of the
    poisoned row is a finite matrix and its solve is non-finite.  B = 8 on the fine tables; B = 63 / 65 on the coarse
    ones, where the solve is the lane = instance k_solve_bm (64 instances a workgroup)."""
    c = setup('smpl', model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', fine_b)
    f, fam = c['f'], c['fams']['pose1']
    rep = (Bn + S.B - 1) // S.B
    tv = t(np.tile(fam['tv'], (rep, 1, 1))[:Bn], dev)
    tj = t(np.tile(fam['tj'], (rep, 1, 1))[:Bn], dev)
    G0 = f._part_rotations(tv, tj)
    s0 = f._shape_solve(G0, tv, tj, beta_regularizer=1.0)
    assert torch.isfinite(G0).all() and all(torch.isfinite(v).all() for v in s0.values())
    s0 = {k: v.clone() for k, v in s0.items()}
    for row in rows:
        tvp, tjp = tv.clone(), tj.clone()
        tvp[row], tjp[row] = poison, poison
        G = f._part_rotations(tvp, tjp)
        s = f._shape_solve(G0, tvp, tjp, beta_regularizer=1.0)
        keep = torch.arange(Bn, device=dev) != row
        assert torch.equal(G[keep], G0[keep]), row
        assert not torch.isfinite(G[row]).all(-1).all(-1).any(), row  # no joint's matrix is finite
        for k in s0:
            assert torch.equal(s[k][keep], s0[k][keep]), (row, k)
        assert not torch.isfinite(s['shape_betas'][row]).any() and not torch.isfinite(s['trans'][row]).any(), row
