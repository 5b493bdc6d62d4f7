"""-m gpu: BodyFitter.fit_with_known_shape one stage at a time against the fp64 oracle of that stage, on both kernel
routes (tests/known_shape_chain_util.py: three calls, each with and without scale_fit, expose the first rotation pass R1,
the alignment T1 at it, the refinement F, the second pass R2 and its alignment T2; each is compared with the oracle
function of that stage at the device's own output of the stage before).  The kernels held here run behind no other entry
point: k_fill_shape, the posed pass from a rest or warm pose, k_regress_joints(_bm) into ws.rjreg, k_scale_trans on the
wave route and k_align_partial_bm<1|2, W> + k_align_finish on the batch-major one — their masked tail, their pad lanes
clamped to row B - 1, the substitution reference <- scale * reference + trans into part sums, joints and regressed joints —
and the refinement with RefineArgs::scaled.

Routes: the default (batch-major) and SMPLFIT_BM_KNOWN_SHAPE=0 (wave per instance), each held to the oracle on its own;
that the switch took is shown by the bits (test_routes_differ), and every call asserts joint_stage == num_iter through
smplfit_stage_launches.  The alignment kernels have no launch counter: which of them ran is not provable without a route
query.

Batches tile the 8 source rows of a family (rows = arange(B) % 8): rows of one source must agree bit for bit whatever
their lane, workgroup or chunk, and the references are those of the first eight.  63 / 65 / 129 (Mp = 256) on the fine
and on the coarse cell tables (SMPLFIT_FINE_B=0); 768 | 769, where the tables and the alignment's chunk count 256 -> 64
change together.  Models: smpl, smplxfat (55 joints), smpl_w6 (KW = 8).

One pair misses its distance gate, deterministically and on both routes: smpl_w6 'mirror' at R1, the right hand (part
23, a leaf part whose reflected covariance has gap 0.016) of source row 7 — |G - G64| 7.1e-4 on the batch-major route and
1.26e-3 on the wave route where the fp32 oracle is at 2.6e-4 (gate 5e-4).  It is the pair family of
tests/test_gpu_stage_chain.py's KNOWN_MISS and conditioning, not a wrong term: the deficits of that step are <= 4.1e-8
(the rotation is an optimum of the fp64 covariance to rounding), and on the same part the fp32 oracle itself is 1.3e-3 off
on source row 0 and 2.3e-3 on row 6 (its family maximum 2.25e-3 against the device's 7.1e-4 / 1.26e-3): a floor of 2 x one
fp32 evaluation of a pair does not bound another.  The host emulation misses more such pairs, on every model
(tests/test_known_shape_chain_host.py, where the figures are).  KNOWN_MISS names the step per (model, route); the case
defers it and gates everything else; test_known_miss raises it, expected to fail, strictly."""

import numpy as np
import pytest
import torch

import known_shape_chain_util as K
import stage_util as S
from smplfitter_amd import _lib
from test_gpu_parity import t, to_np
from test_gpu_stage_chain import fitter
from test_gpu_stages_hard import setup

pytestmark = pytest.mark.gpu

KEYS = ('orientations', 'trans', 'scale_corr')
MODELS = ('smpl', 'smplxfat', 'smpl_w6')
ROUTES = {'bm': None, 'wave': '0'}  # SMPLFIT_BM_KNOWN_SHAPE
# 'mirror' with target joints at B = 65 on the fine tables: (model, route) -> the steps deferred to test_known_miss
KNOWN_MISS = {('smpl_w6', 'bm'): ('R1',), ('smpl_w6', 'wave'): ('R1',)}
MIRROR_LOOSE = pytest.mark.xfail(strict=True, reason="smpl_w6 'mirror' R1, (row 7, part 23): 7.1e-4 / 1.26e-3 against 2 x the fp32 "
                                                     "oracle's 2.6e-4 on a pair with gap 0.016 (module docstring)")
_calls = {}    # (model, case, batch, route, tables) -> the six clean calls: computed once, shared, read only
_checked = {}  # the same key -> check_chain's figures


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def set_route(smplfit_env, route, fine_b):
    smplfit_env('SMPLFIT_BM_KNOWN_SHAPE', ROUTES[route])
    smplfit_env('SMPLFIT_FINE_B', fine_b)


def run_calls(c, case, rows, dev, poison_row=None):
    """The six calls of one case on the batch ``rows`` (source row of each instance): {scale_fit: (K1, K1F, K2)} as
    torch dicts.  Every call must launch the joint stage once per rotation pass and none of the stage kernels of a fit."""
    inp, k = case.inputs(c['fams'][case.family]), K.known(c, case)
    args = {n: t(None if a is None else a[rows], dev) for n, a in (
        ('target_vertices', inp['tv']), ('target_joints', inp['tj']), ('vertex_weights', inp['vw']), ('joint_weights', inp['jw']),
        ('shape_betas', k['betas']), ('kid_factor', k['kid']), ('initial_pose_rotvecs', k['pose0']))}
    if poison_row is not None:
        for n in ('target_vertices', 'target_joints'):
            if args[n] is not None:
                args[n] = args[n].clone()
                args[n][poison_row] = float('nan')
    f, outs = fitter(c, case.kid), {}
    for sf in (False, True):
        res = []
        for call in K.CALLS:
            torch.cuda.synchronize()
            before = _lib.stage_launches()
            r = f.fit_with_known_shape(**args, **call, scale_fit=sf, requested_keys=[])
            torch.cuda.synchronize()
            got = {n: v - before[n] for n, v in _lib.stage_launches().items()}
            assert got['joint_stage'] == call['num_iter'], (call, got)
            assert not any(got[n] for n in ('rotations_bm', 'rotations_bm_rounds', 'solve_bm', 'shape_solve', 'refine_bm')), (call, got)
            assert set(r) == set(KEYS if sf else KEYS[:2]), set(r)
            res.append(dict(r))
        outs[sf] = tuple(res)
    return outs


def clean_calls(name, c, case, Bn, dev, route, fine_b):
    key = (name, case.id, Bn, route, fine_b)
    if key not in _calls:
        _calls[key] = run_calls(c, case, np.arange(Bn) % S.B, dev)
    return _calls[key]


def check_case(name, c, case, Bn, dev, route, fine_b=None):
    key = (name, case.id, Bn, route, fine_b)
    if key not in _checked:
        _checked[key] = _check_case(name, c, case, Bn, dev, route, fine_b)
    return _checked[key]


def _check_case(name, c, case, Bn, dev, route, fine_b):
    rows = np.arange(Bn) % S.B
    outs = clean_calls(name, c, case, Bn, dev, route, fine_b)
    for sf, (k1, k1f, _) in outs.items():  # the refinement changes rotations only
        for k in KEYS[1:2 + sf]:
            assert torch.equal(k1[k], k1f[k]), (name, case.id, sf, k)
    outs = {sf: tuple(to_np(o) for o in res) for sf, res in outs.items()}
    for sf, res in outs.items():
        for i, o in enumerate(res):
            for k, v in o.items():
                for src in range(S.B):
                    same = v[rows == src]
                    assert all(np.array_equal(same[0], x) for x in same[1:]), (name, case.id, sf, i, k, src)
    defer = KNOWN_MISS.get((name, route), ()) if case.id == 'mirror-j' and (Bn, fine_b) == (65, None) else ()
    return K.check_chain(name, c, case, outs, f'device {route} B={Bn}' + (' coarse' if fine_b == '0' else ''), rows=rows, defer=defer)


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('name,case', [pytest.param(n, case, id=f'{n}-{case.id}') for n in MODELS for case in K.cases(n)])
def test_chain_families(name, case, route, model_root, golden, dev, smplfit_env, capsys):
    """Every case of known_shape_chain_util.cases() at B = 65 on the fine tables: the unmasked families; the masked ones
    with both weights (weighted in the rotations and in the alignment), with vertex weights alone and with joint weights
    alone (weighted in the rotations, unweighted in the alignment); joints omitted, plain and with vertex weights (which
    then do enter the alignment); a warm start; scaled targets (scale_corr 1 / 0.6 .. 1 / 1.6); the per-row kid factor.
    (observed maxima per model and step, the fp32 oracle's in brackets: DESIGN.md §5)"""
    c = setup(name, model_root, golden, dev)
    set_route(smplfit_env, route, None)
    with capsys.disabled():
        print()
        check_case(name, c, case, 65, dev, route)


BATCH_CASES = [('smpl', K.Case('hard_pose')), ('smpl', K.Case('hard_pose', joints=False, scaled=True)),
               ('smplxfat', K.Case('hard_pose', joints=False, scaled=True)), ('smpl_w6', K.Case('hard_pose'))]


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('Bn,fine_b', [(63, None), (129, None), (63, '0'), (65, '0'), (129, '0')])
@pytest.mark.parametrize('name,case', [pytest.param(n, case, id=f'{n}-{case.id}') for n, case in BATCH_CASES])
def test_chain_batches(name, case, Bn, fine_b, route, model_root, golden, dev, smplfit_env, capsys):
    """The other batches — 63 (a wave short of one lane), 129 (Mp = 256, a third block of one lane and 63 pad lanes that
    copy row 128) — on the fine tables, and all three on the coarse ones."""
    c = setup(name, model_root, golden, dev)
    set_route(smplfit_env, route, fine_b)
    with capsys.disabled():
        print()
        check_case(name, c, case, Bn, dev, route, fine_b)


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('Bn', [768, 769])
@pytest.mark.parametrize('family', ['hard_pose', 'far'])
def test_chain_table_switch(family, Bn, route, model_root, golden, dev, smplfit_env, capsys):
    """sf::kFineMaxBatch = 768 | 769: the last batch on the fine cell tables with 256 alignment chunks (27 vertices a
    chunk: six full steps of four and a tail of three), the first on the coarse ones with 64 (108 a chunk, the last chunk
    86: a tail of two).  SMPL, with and without scale_fit as every case.  (A tail step that kept its weight shows at 768
    and at every smaller batch, 1e-5 .. 2e-4 m in trans; at 769 the one tail of two vertices stays near 1e-6 m, under
    the gate: DESIGN.md §5.)"""
    c = setup('smpl', model_root, golden, dev)
    set_route(smplfit_env, route, None)
    with capsys.disabled():
        print()
        check_case('smpl', c, K.Case(family), Bn, dev, route)


@pytest.mark.parametrize('name', MODELS)
def test_routes_differ(name, model_root, golden, dev, smplfit_env):
    """SMPLFIT_BM_KNOWN_SHAPE=0 takes another route: somewhere in the six calls of a case the two routes differ in bits
    (they sum in another order), with target joints and without them."""
    c = setup(name, model_root, golden, dev)
    for case in (K.Case('hard_pose'), K.Case('hard_pose', joints=False, scaled=True)):
        outs = {}
        for route in ROUTES:
            set_route(smplfit_env, route, None)
            outs[route] = clean_calls(name, c, case, 65, dev, route, None)
        differs = any(not torch.equal(a[k], b[k]) for sf in (False, True)
                      for a, b in zip(outs['bm'][sf], outs['wave'][sf]) for k in a)
        assert differs, (name, case.id, 'SMPLFIT_BM_KNOWN_SHAPE=0 changed nothing: the batch-major route did not run')


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('Bn,row', [(65, 5), (65, 62), (65, 63), (65, 64), (129, 128)])
@pytest.mark.parametrize('name', ['smpl', 'smplxfat'])
def test_poisoned_row(name, Bn, row, route, model_root, golden, dev, smplfit_env):
    """One instance with NaN targets, vertices and joints: inside a wave, its last two lanes, and row B - 1 — the row
    whose mean the pad lanes of k_align_partial_bm read.  Every other row of all six calls is bit-identical to the clean
    calls in all outputs, and the poisoned row has no finite rotation."""
    c = setup(name, model_root, golden, dev)
    set_route(smplfit_env, route, None)
    case = K.Case('pose1')
    clean = clean_calls(name, c, case, Bn, dev, route, None)
    dirty = run_calls(c, case, np.arange(Bn) % S.B, dev, poison_row=row)
    keep = torch.arange(Bn, device=dev) != row
    for sf in (False, True):
        for o0, o in zip(clean[sf], dirty[sf]):
            for k in o0:
                assert torch.isfinite(o0[k]).all(), k
                assert torch.equal(o[k][keep], o0[k][keep]), (row, sf, k)
            assert not torch.isfinite(o['orientations'][row]).all(-1).all(-1).any(), row  # no joint's matrix is finite


@MIRROR_LOOSE
@pytest.mark.parametrize('name,route,step', [k + (s,) for k, steps in KNOWN_MISS.items() for s in steps], ids=lambda v: str(v))
def test_known_miss(name, route, step, model_root, golden, dev, smplfit_env, capsys):
    """The steps of 'mirror' whose distance gate misses on a loose pair (KNOWN_MISS): every other gate of the case is
    asserted by test_chain_families; this raises the deferred assertion of one such step, unchanged."""
    c = setup(name, model_root, golden, dev)
    set_route(smplfit_env, route, None)
    with capsys.disabled():
        figs = check_case(name, c, K.Case('mirror'), 65, dev, route)
    if step in figs['deferred']:
        raise figs['deferred'][step]
