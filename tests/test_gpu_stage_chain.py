"""-m gpu: the stage kernels that only run inside a whole fit — the lane = instance k_rotations_bm /
k_rotations_bm_rounds, k_prologue_bm, k_solve_bm, k_refine_bm, and k_refine_epilogue behind k_gt_to_g — one stage at a
time against the fp64 oracle of that stage, on the hard families of tests/stage_util.py (tests/stage_chain_util.py: three
fits expose the five stages R1, S1, F, R2, S2; each is compared with the oracle function of that stage at the device's own
output of the stage before, under the criteria of stage_util).

The coarse cell tables are forced with SMPLFIT_FINE_B=0 (as tests/test_gpu_stages_hard.py and test_gpu_gemm_planes.py
do), the 8 source rows of a family are tiled over the batch, rows of one source must agree bit for bit whatever their lane
or workgroup, and EVERY call asserts its route through the library's launch counters (smplfit_stage_launches): on SMPL
k_rotations_bm, k_prologue_bm<10 / 11>, k_solve_bm once per iteration and k_refine_bm once, no wave counterpart; on the
fat-part SMPL-X (55 joints) k_rotations_bm_rounds, and k_gt_to_g + k_refine_epilogue for the refinement.  Where a build
or model does not take the route the case skips with the counts in the message.

Batches: 63 (a wave short of one lane), 65 (a second workgroup of one lane and 63 pad lanes), 129 (Mp = 256: the pad
columns of the GEMM planes).  Models: smpl (24 joints), smplxfat (55: two rounds, the toe slots), smpl_w6 (KW = 8)."""

import os

import numpy as np
import pytest
import torch

import stage_chain_util as C
import stage_util as S
from smplfitter_amd import _lib
from test_gpu_parity import t, to_np
from test_gpu_stages_hard import setup

pytestmark = pytest.mark.gpu

KEYS = ('orientations', 'shape_betas', 'trans', 'kid_factor')
CALLS = (dict(num_iter=1, final_adjust_rots=False), dict(num_iter=1), dict(num_iter=2, final_adjust_rots=False))
MODELS = ('smpl', 'smplxfat', 'smpl_w6')
FAMILY_CASES = ([C.Case(f) for f in S.UNMASKED] + [C.Case(f, weights='v') for f in ('part_off', 'part_two', 'mask01')] +
                [C.Case('joint_off', weights='j')])
# One pair misses its distance gate, deterministically: smpl_w6 'mirror', the right hand (part 23, a leaf part whose
# reflected covariance has s = (1, 0.41, 0.39) s1, gap (s2 - s3) / s1 = 0.02), source row 0.  With target joints at R2:
# |G - G64| 2.13e-3 where the fp32 oracle is at 3.1e-4 (gate 5e-4); without them at R1: 1.21e-3 against 4.7e-4.  Both
# deficits are <= 1.0e-7, i.e. the device's rotation is an optimum of the fp64 covariance to rounding, and on the same
# part the fp32 oracle itself is 3.0e-3 off on source row 7 where the device is 1.1e-4 off: the pair is loose in fp32
# (the hand's part sums cancel by (0.8 m / 0.05 m)^2 before a gap of 0.02 divides them), which of two fp32 evaluations
# lands closer is chance, and the floor of 2 x the fp32 oracle ON THAT PAIR does not cover the other.  Suspected cause and
# what would fix it (part sums about a local origin): DESIGN.md §5.  The two cases defer the assertion of those steps
# (KNOWN_MISS) and gate everything else; test_known_miss raises it, expected to fail, strictly.
# (without joints the second pass misses too, on the hands again: (row 2, part 22) 1.39e-3 against 2.4e-4, (row 7, part 23)
# 1.60e-3 against 2.6e-4)
KNOWN_MISS = {('smpl_w6', 'mirror', True, 65): ('R2',), ('smpl_w6', 'mirror', False, 129): ('R1', 'R2')}
W6_MIRROR = pytest.mark.xfail(strict=True, reason="smpl_w6 'mirror', (row 0, part 23): 2.1e-3 / 1.2e-3 against 2 x the fp32 "
                                                  "oracle's 3.1e-4 / 4.7e-4 on a pair with gap 0.02 (DESIGN.md §5)")
_checked = {}  # (model, family, case tag, kid, batch) -> check_chain's figures
_fits = {}  # (model, case tag, family, kid, batch, environment) -> the three clean fits: computed once, shared, read only


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def fitter(c, kid):
    if kid and 'f_kid' not in c:
        from smplfitter_amd.pt import BodyFitter

        c['f_kid'] = BodyFitter(c['m'], enable_kid=True)
    return c['f_kid'] if kid else c['f']


def expected_route(c, kid, call):
    """The launches of one call on the lane = instance route (module docstring)."""
    n, final, small = call['num_iter'], call.get('final_adjust_rots', True), c['m'].num_joints <= 32
    e = dict.fromkeys(_lib.STAGE_IDS, 0)
    e['rotations_bm' if small else 'rotations_bm_rounds'] = n
    e['prologue_bm_s11' if kid else 'prologue_bm_s10'] = n
    e['solve_bm'] = n
    if small:
        e['refine_bm'] = 1
    else:  # (the part sums of the last pass, which only a final adjustment reads, are combined for k_refine_epilogue)
        e.update(gt_to_g=1, refine_epilogue=1, psum_combine=1 if final else 0)
    return e


def run_fits(c, case, rows, dev, kid=False, poison_row=None, check_route=True):
    """The three fits of one case on the batch ``rows`` (source row of each instance); each with its counter differences.
    Returns the result dicts (torch).  The in-tree build must take the lane = instance route on the three models here; a
    build loaded through SMPLFIT_LIB that does not take it skips with the counts."""
    fam = c['fams'][case.family]
    inp = case.inputs(fam)
    args = [t(None if a is None else a[rows], dev) for a in (inp['tv'], inp['tj'], inp['vw'], inp['jw'])]
    if poison_row is not None:
        args[0] = args[0].clone()
        args[0][poison_row] = float('nan')
        if args[1] is not None:
            args[1] = args[1].clone()
            args[1][poison_row] = float('nan')
    kw = {k: (t(v[rows], dev) if isinstance(v, np.ndarray) else v) for k, v in case.fit_kwargs().items()}
    outs = []
    for call in CALLS:
        torch.cuda.synchronize()
        before = _lib.stage_launches()
        r = fitter(c, kid).fit(*args, **kw, **call, requested_keys=[])
        torch.cuda.synchronize()
        got = {k: v - before[k] for k, v in _lib.stage_launches().items()}
        if check_route:
            # (another build loaded through SMPLFIT_LIB may lack the route; the in-tree build must take it on these models)
            if os.environ.get('SMPLFIT_LIB') and (got['solve_bm'] == 0 or got['prologue_bm_s10'] + got['prologue_bm_s11'] == 0):
                pytest.skip(f'the lane = instance stage kernels are not taken on this build / model: {got}')
            assert got == expected_route(c, kid, call), (call, got)
        outs.append({k: v for k, v in r.items() if k in KEYS})
    return outs


def clean_fits(name, c, case, rows, dev, kid=False, env=''):
    key = (name, case.family, case.tag, kid, len(rows), env)
    if key not in _fits:
        _fits[key] = run_fits(c, case, rows, dev, kid)
    return _fits[key]


def check_case(name, c, case, Bn, dev, kid=False):
    key = (name, case.family, case.tag, kid, Bn)
    if key not in _checked:
        _checked[key] = _check_case(name, c, case, Bn, dev, kid)
    return _checked[key]


def _check_case(name, c, case, Bn, dev, kid):
    rows = np.arange(Bn) % S.B
    outs = clean_fits(name, c, case, rows, dev, kid)
    for k in ('shape_betas', 'trans', 'kid_factor'):  # the refinement changes rotations only
        if k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), (name, case.family, k)
    outs = [to_np(o) for o in outs]
    for i, o in enumerate(outs):
        for k, v in o.items():
            for src in range(S.B):
                same = v[rows == src]
                assert all(np.array_equal(same[0], x) for x in same[1:]), (name, case.family, i, k, src)
    defer = KNOWN_MISS.get((name, case.family, case.joints, Bn), ())
    return C.check_chain(name, c, case, outs, f'device B={Bn}' + (' kid' if kid else ''), rows=rows, kid=kid,
                         defer=defer if not case.weights and not kid else ())


@pytest.mark.parametrize('name,case', [pytest.param(name, case, id=f'{name}-{case.family}') for name in MODELS for case in FAMILY_CASES])
def test_chain_families(name, case, model_root, golden, dev, smplfit_env, capsys):
    """Every unmasked family; 'part_off', 'part_two', 'mask01' with their vertex weights alone (they enter the part sums,
    not the solve, so the route keeps k_solve_bm and k_prologue_bm); 'joint_off' with its joint weights alone (the Kabsch
    of the multi-joint parts, the weighted joint block).  B = 65.
    (observed maxima per step — R1 / F / R2 |G - G64| with the bone factor, S1 / S2 mesh and betas — with the fp32
    oracle's in brackets: DESIGN.md §5)"""
    c = setup(name, model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', '0')
    with capsys.disabled():
        print()
        check_case(name, c, case, 65, dev)


def option_cases(c):
    warm = C.warm_start(c['of64'], c['fams']['pose1'])
    return {
        'no_joints': (C.Case('pose1', joints=False), False),        # tables kShareLbsAll, regressed target joints
        'no_joints_hard': (C.Case('hard_pose', joints=False), False),
        'reg0': (C.Case('hard_pose', reg=0.0), False),
        'kid': (C.Case('betas5'), True),                              # k_prologue_bm<11>, k_refine_bm<11>
        'kid_reg0_no_joints': (C.Case('pose1', joints=False, reg=0.0), True),
        'warm': (C.Case('pose1', warm=warm), False),                 # gprev_mode 2, the ridge references
        'warm_no_joints': (C.Case('pose1', joints=False, warm=warm), False),  # kShareLbsAll in the first pass too
    }


@pytest.mark.parametrize('opt', ['no_joints', 'no_joints_hard', 'reg0', 'kid', 'kid_reg0_no_joints', 'warm', 'warm_no_joints'])
def test_chain_options(opt, model_root, golden, dev, smplfit_env, capsys):
    """SMPL, B = 63: joints omitted, beta_regularizer 0, the kid unknown, a warm start (initial_pose_rotvecs and
    initial_shape_betas from a rounded oracle solution of 'pose1') with and without target joints."""
    c = setup('smpl', model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', '0')
    case, kid = option_cases(c)[opt]
    with capsys.disabled():
        print()
        check_case('smpl', c, case, 63, dev, kid)


BATCH_CASES = [('smpl', 'far', True, 63), ('smpl', 'hard_pose', True, 129), ('smplxfat', 'pose1', False, 63),
               ('smpl_w6', 'mirror', False, 129), ('smpl_w6', 'hard_pose', True, 129)]


@pytest.mark.parametrize('name,family,joints,Bn', BATCH_CASES)
def test_chain_batches(name, family, joints, Bn, model_root, golden, dev, smplfit_env, capsys):
    """The other batches: 63 (no lane 63) and 129 (Mp = 256, a third workgroup of one lane)."""
    c = setup(name, model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', '0')
    with capsys.disabled():
        print()
        check_case(name, c, C.Case(family, joints=joints), Bn, dev)


@pytest.mark.parametrize('name', ['smpl', 'smplxfat'])
def test_prologue_ancestor_chains(name, model_root, golden, dev, smplfit_env, capsys):
    """k_prologue_bm walks each joint's chain of ancestors kProChain = 5 at a time, the tail of a request clamped to the
    last ancestor: S1's joints are held to the fp64 solve JOINT BY JOINT (check_chain: every (row, joint) within
    max(1e-4 m, 2 x the fp32 oracle's)), here reported by chain length — none (the root), at most 5 (one request), exactly
    5 and 6 (a full request; one more), more than 5 (two requests with a clamped tail).  SMPL has all of them: the pelvis;
    e.g. the knees (2) and the neck (4); the collars' children, the shoulders (5); the elbows (6); the wrists and hands
    (7, 8).  The fingers of the fat-part SMPL-X reach 10."""
    c = setup(name, model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', '0')
    n = C.ancestors(list(c['om64'].parents))
    classes = {'0': n == 0, '1..5': (n >= 1) & (n <= 5), '5': n == 5, '6': n == 6, '>5': n > 5}
    assert all(m.any() for m in classes.values()), {k: int(m.sum()) for k, m in classes.items()}
    with capsys.disabled():
        print()
        figs = check_case(name, c, C.Case('hard_pose'), 65, dev)
        e, e32 = figs['S1_joints']
        print(f'[prologue chains {name}] ancestors: max |joint - fp64| m (fp32 oracle)  ' +
              '  '.join(f'{k}: {e[:, m].max():.2e} ({e32[:, m].max():.2e})' for k, m in classes.items()))


@pytest.mark.parametrize('name,row', [('smpl', 5), ('smpl', 62), ('smpl', 63), ('smpl', 64), ('smplxfat', 63), ('smplxfat', 64)])
def test_poisoned_row(name, row, model_root, golden, dev, smplfit_env):
    """One instance with NaN targets (B = 65: inside a wave, its last two lanes, the single lane of the second
    workgroup): every other row of all three fits is bit-identical to the clean fits, and the poisoned row has no finite
    rotation."""
    c = setup(name, model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', '0')
    case, rows = C.Case('pose1'), np.arange(65) % S.B
    clean = clean_fits(name, c, case, rows, dev)
    keep = torch.arange(65, device=dev) != row
    for o0, o in zip(clean, run_fits(c, case, rows, dev, poison_row=row)):
        for k in o0:
            assert torch.isfinite(o0[k]).all(), k
            assert torch.equal(o[k][keep], o0[k][keep]), (row, k)
        assert not torch.isfinite(o['orientations'][row]).all(-1).all(-1).any(), row  # no joint's matrix is finite


@pytest.mark.parametrize('case', FAMILY_CASES, ids=lambda c: c.family)
def test_gemm_planes_bits_on_hard_features(case, model_root, golden, dev, smplfit_env):
    """The SMPL cases once more with SMPLFIT_GEMM_PLANES=0 (k_prologue_bm writes fp32 feature rows, the GEMM splits
    them itself): torch.equal to the default — the claim of tests/test_gpu_gemm_planes.py, here on pose features of order
    2 —, the plane GEMM counted once per solve and not at all; and with SMPLFIT_GEMM=f32 the solves differ in bits (the
    comparison would see another GEMM)."""
    c = setup('smpl', model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', '0')
    rows = np.arange(65) % S.B
    g0 = _lib.gemm_plane_launches()
    default = run_fits(c, case, rows, dev)
    n_default = _lib.gemm_plane_launches() - g0
    if n_default == 0:
        pytest.skip('the GEMM does not read feature planes on this build')
    assert n_default == sum(call['num_iter'] for call in CALLS)
    smplfit_env('SMPLFIT_GEMM_PLANES', '0')
    g0 = _lib.gemm_plane_launches()
    rows_fp32 = run_fits(c, case, rows, dev)
    assert _lib.gemm_plane_launches() == g0
    for o0, o in zip(default, rows_fp32):
        for k in o0:
            assert torch.equal(o[k], o0[k]), (case.family, k)
    smplfit_env('SMPLFIT_GEMM_PLANES', None)
    smplfit_env('SMPLFIT_GEMM', 'f32')
    other = run_fits(c, case, rows, dev, check_route=False)
    assert any(not torch.equal(o['shape_betas'], o0['shape_betas']) for o0, o in zip(default, other)), case.family


def test_both_weights_leave_the_route(model_root, golden, dev, smplfit_env):
    """Vertex AND joint weights enter the shape solve: the call leaves k_solve_bm / k_prologue_bm (route_of: eff_v) —
    seen through the counters; its stages are gated by tests/test_gpu_stages_hard.py and the parity tests."""
    c = setup('smpl', model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', '0')
    fam = c['fams']['part_off']
    rows = np.arange(65) % S.B
    torch.cuda.synchronize()
    before = _lib.stage_launches()
    c['f'].fit(*(t(fam[k][rows], dev) for k in ('tv', 'tj', 'vw', 'jw')), num_iter=2, requested_keys=[])
    torch.cuda.synchronize()
    got = {k: v - before[k] for k, v in _lib.stage_launches().items()}
    assert got['solve_bm'] == 0 and got['prologue_bm_s10'] == 0 and got['rotations_bm'] == 0 and got['refine_bm'] == 0, got
    assert got['shape_solve'] == 2 and got['joint_stage'] == 2 and got['refine_epilogue'] == 1, got


@W6_MIRROR
@pytest.mark.parametrize('name,family,joints,Bn,step', [k + (step,) for k, steps in KNOWN_MISS.items() for step in steps],
                         ids=lambda v: str(v))
def test_known_miss(name, family, joints, Bn, step, model_root, golden, dev, smplfit_env, capsys):
    """The steps of the two smpl_w6 'mirror' cases whose distance gate misses on a hand (KNOWN_MISS above): every other
    gate of these cases is asserted by test_chain_families / test_chain_batches; this raises the deferred assertion of
    one such step, unchanged."""
    c = setup(name, model_root, golden, dev)
    smplfit_env('SMPLFIT_FINE_B', '0')
    with capsys.disabled():
        figs = check_case(name, c, C.Case(family, joints=joints), Bn, dev)
    if step in figs['deferred']:
        raise figs['deferred'][step]
