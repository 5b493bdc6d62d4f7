"""-m gpu: fit(scale_target=True) / fit(scale_fit=True) and the same options of fit_with_known_pose one stage at a time
against the fp64 oracle of that stage, on every kernel route a scale unknown takes (tests/scale_chain_util.py: per option
the calls SS0, A, B, C and the unscaled D expose the scaled solve alone, the first pass R1 with the scaled solve SS1,
k_scale_refs + the scaled refinement F, the second pass R2 behind the unscaled solve of a scaled fit, and SS2; each is
compared with the oracle function of that stage at the device's own output of the stage before).  The kernels held here
run behind no other call: k_accum_w_bm<10, 1, true|false, true> + k_accum_combine over NE1 + 16 entries (batch-major
route), k_scale_extras<S, KW> (wave route), k_shape_solve_scaled<false|true>, k_scale_refs, the refinement on ws.tjs /
RefineArgs::scaled, and k_solve_bm behind k_joint_stage + k_jd_transpose (route_of: a scale switches k_prologue_bm off and
keeps k_solve_bm).

Routes.  'bm': the default, SMPL and the fat-part SMPL-X (10 betas, 4 weights: what k_accum_w_bm is built for); 'wave':
SMPLFIT_BM_SCALE=0 on the same two models (k_scale_extras<10, 4>); 'own': the models route_of keeps off the batch-major
path under a scale whatever the switch — the kid fitter <11, 4>, smpl_w6 <10, 8>, smpl_b16 <16, 4> and with the kid unknown
<17, 4> — and smpl_b32 on the general path (k_shape_solve_scaled<true>).  The extra-sum kernels have no launch counter:
that SMPLFIT_BM_SCALE=0 took another one is shown by the bits alone (test_routes_differ); which of them ran is not provable
without a route query.  What the counters do show is asserted on every call: no k_prologue_bm, no
k_rotations_bm, no k_refine_bm, k_joint_stage once per iteration, k_solve_bm exactly for the unscaled solves on the coarse
tables of the batch-major route (not where weights enter the solve) — the same count in C as in D.

D, the unscaled fit whose solve S1 is the state in front of C's second pass, runs on the route a scaled call takes:
SMPLFIT_PROLOGUE_BM=0 on 'bm', SMPLFIT_BM=0 on 'wave' and 'own'; its first pass must be torch.equal to A's.

Batches tile the 8 source rows of a family (rows = arange(B) % 8; B = 1: eight calls of one row each): rows of one source
must agree bit for bit whatever their lane, workgroup or chunk.  65 everywhere; 1, 63, 129 on the fine and 65, 129 on the
coarse cell tables (SMPLFIT_FINE_B=0) on four cases per route; one run in two chunks."""

import numpy as np
import pytest
import torch

import scale_chain_util as X
import stage_util as S
from smplfitter_amd import _lib
from test_gpu_parity import get_model, t, to_np

pytestmark = pytest.mark.gpu

ROUTES = {'bm': None, 'wave': '0', 'own': None}  # SMPLFIT_BM_SCALE
D_ENV = {'bm': ('SMPLFIT_PROLOGUE_BM', '0'), 'wave': ('SMPLFIT_BM', '0'), 'own': ('SMPLFIT_BM', '0')}
OWN = ('smpl_kid', 'smpl_w6', 'smpl_b16', 'smpl_b16_kid')
MODEL_ROUTES = [(n, r) for n in X.FULL for r in ('bm', 'wave')] + [(n, 'own') for n in OWN]
# 'mirror' with target joints at B = 65 on the fine tables, both options: (model, route) -> the steps deferred to
# test_known_miss.  The fat-part SMPL-X on the batch-major route at R1 — the first rotation pass, which no scale unknown
# touches (A's bits are D's): (source row 4, part 51) |G - G64| 2.04e-3 against the gate 2e-3 where the fp32 oracle is at
# 9.2e-4, deficit 1.4e-7 (an optimum of the fp64 covariance to rounding): the loose reflected pair of
# tests/test_known_shape_chain_host.py (part 51 at R1: the fp32 oracle 1.7e-3 off on a neighbouring row).  On the wave
# route the same pair is inside.
KNOWN_MISS = {('smplxfat', 'bm'): ('R1',)}
MIRROR_LOOSE = pytest.mark.xfail(strict=True, reason="smplxfat 'mirror' R1 on the batch-major route, (row 4, part 51): 2.04e-3 against "
                                                     "max(2e-3, 2 x the fp32 oracle's 9.2e-4) on a loose reflected pair")
_setups = {}
_calls = {}    # (model, case, option, batch, route, tables, chunks) -> the clean calls: computed once, shared, read only
_checked = {}  # the same key -> check_chain's figures


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def setup(name, model_root, golden, dev):
    """host_setup of the model plus its BodyModel and the BodyFitter (with the kid unknown where the name says so)."""
    from smplfitter_amd.pt import BodyFitter, BodyModel

    base, nb, kid = X.MODELS[name]
    c = X.host_setup(name, model_root, golden)
    if ('gpu', kid) not in c:
        if 'gpu_m' not in c:
            c['gpu_m'] = (BodyModel('smpl', 'neutral', model_root=f'{model_root}/{base}', num_betas=nb, device=dev) if nb
                          else get_model(model_root, base, golden(base), dev)[0])
        c['gpu', kid] = BodyFitter(c['gpu_m'], enable_kid=kid)
    return c, c['gpu', kid]


def counted(fn):
    torch.cuda.synchronize()
    before = _lib.stage_launches()
    r = fn()
    torch.cuda.synchronize()
    return r, {k: v - before[k] for k, v in _lib.stage_launches().items()}


def run_calls(c, f, name, case, mode, rows, dev, smplfit_env, route, fine_b, poison_row=None, share=None):
    """SS0, A, B, C with the option ``mode`` and the unscaled D (module docstring) on the batch ``rows`` (source row of
    each instance), as torch dicts; every fit asserts what the launch counters show of its route.  ``share``: None, True
    (share_beta) or a list of segment sizes — then SS0 alone."""
    inp = case.inputs(c['fams'][case.family])
    args = {n: t(None if a is None else a[rows], dev) for n, a in (
        ('target_vertices', inp['tv']), ('target_joints', inp['tj']), ('vertex_weights', inp['vw']), ('joint_weights', inp['jw']))}
    if poison_row is not None:
        for n in ('target_vertices', 'target_joints'):
            if args[n] is not None:
                args[n] = args[n].clone()
                args[n][poison_row] = float('nan')
    kw = {k: (t(v[rows], dev) if isinstance(v, np.ndarray) else v) for k, v in case.fit_kwargs().items()}
    opts = X.fit_options(case, mode)
    keep = lambda r: {k: v for k, v in r.items() if k in X.KEYS}  # noqa: E731
    r64 = X.refs(c, name, case)[0]
    pose = t(X.pose_of(r64.R1()[0], c['om64'].parents)[rows], dev)
    kp = dict(beta_regularizer=case.reg)
    if 'initial_shape_betas' in kw:
        kp['beta_regularizer_reference'] = kw['initial_shape_betas']
    if share is not None:
        kp.update(dict(share_beta=True) if share is True else dict(share_beta_segments=list(share)))
    outs = dict(SS0=keep(f.fit_with_known_pose(pose, **args, **kp, **opts)))
    if share is not None:
        return outs
    general = X.MODELS[name][1] == 32
    # k_solve_bm: the coarse tables of the batch-major route, and no weights in the solve (route_of: eff_v — both weights
    # given, or vertex weights without target joints)
    w = case.weights or ''
    coarse_bm = route == 'bm' and fine_b == '0' and not ('v' in w and ('j' in w or not case.joints))
    got = {}
    for key in 'ABCD':
        call = X.CALLS['A' if key == 'D' else key]
        if key == 'D':
            smplfit_env(*D_ENV[route])
        r, got[key] = counted(lambda: f.fit(**args, **kw, **call, **({} if key == 'D' else opts), requested_keys=[]))
        if key == 'D':
            smplfit_env(D_ENV[route][0], None)
        outs[key] = keep(r)
        g = got[key]
        assert not any(g[n] for n in ('prologue_bm_s10', 'prologue_bm_s11', 'rotations_bm', 'rotations_bm_rounds', 'refine_bm')), (key, g)
        if not general:
            assert g['joint_stage'] == call['num_iter'], (key, g)
            assert g['refine_epilogue'] == 1, (key, g)  # (refinement or not, the epilogue is this kernel's)
            # the unscaled solves: D's one and the first of C; A and B have the scaled solve alone
            assert g['solve_bm'] == (int(coarse_bm) if key in 'CD' else 0), (key, route, fine_b, g)
    assert got['C']['solve_bm'] == got['D']['solve_bm'], got
    return outs


def rows_of(Bn):
    return np.arange(max(Bn, S.B)) % S.B


def clean_calls(name, c, f, case, mode, Bn, dev, smplfit_env, route, fine_b, chunks=None):
    """The clean calls of one key.  B = 1: one call per source row, stacked."""
    key = (name, case.id, mode, Bn, route, fine_b, chunks)
    if key not in _calls:
        if Bn == 1:
            one = [run_calls(c, f, name, case, mode, np.array([k]), dev, smplfit_env, route, fine_b) for k in range(S.B)]
            _calls[key] = {call: {k: torch.cat([o[call][k] for o in one]) for k in one[0][call]} for call in one[0]}
        else:
            _calls[key] = run_calls(c, f, name, case, mode, rows_of(Bn), dev, smplfit_env, route, fine_b)
    return _calls[key]


def set_route(smplfit_env, route, fine_b):
    smplfit_env('SMPLFIT_BM_SCALE', ROUTES[route])
    smplfit_env('SMPLFIT_FINE_B', fine_b)


def check_case(name, case, mode, Bn, route, fine_b, model_root, golden, dev, smplfit_env, chunks=None):
    key = (name, case.id, mode, Bn, route, fine_b, chunks)
    if key in _checked:
        return _checked[key]
    c, f = setup(name, model_root, golden, dev)
    case = X.bound(c, case)
    set_route(smplfit_env, route, fine_b)
    rows = rows_of(Bn)
    outs = clean_calls(name, c, f, case, mode, Bn, dev, smplfit_env, route, fine_b, chunks)
    assert torch.equal(outs['A']['orientations'], outs['D']['orientations']), (name, case.id, 'A and D differ in R1')
    for k in outs['A']:  # k_scale_refs copies back what the solve returned; the refinement changes rotations only
        if k != 'orientations':
            assert torch.equal(outs['A'][k], outs['B'][k]), (name, case.id, k)
    outs = {k: to_np(o) for k, o in outs.items()}
    for call, o in outs.items():
        for k, v in o.items():
            assert np.isfinite(v).all(), (name, case.id, call, k)
            for src in range(S.B):
                same = v[rows == src]
                assert all(np.array_equal(same[0], x) for x in same[1:]), (name, case.id, call, k, src)
    label = f'device {route} {"st" if mode == 1 else "sf"} B={Bn}' + (' coarse' if fine_b == '0' else '') + (f' chunks={chunks}' if chunks else '')
    defer = KNOWN_MISS.get((name, route), ()) if (case.id, Bn, fine_b, chunks) == ('mirror-j_reg1', 65, None, None) else ()
    _checked[key] = X.check_chain(name, c, case, mode, outs, label, rows=rows, defer=defer)
    return _checked[key]


FAMILY_PARAMS = [pytest.param(n, r, case, id=f'{n}-{r}-{case.id}') for n, r in MODEL_ROUTES for case in X.cases(n)]


@pytest.mark.parametrize('mode', X.MODES)
@pytest.mark.parametrize('name,route,case', FAMILY_PARAMS)
def test_chain_families(name, route, case, mode, model_root, golden, dev, smplfit_env, capsys):
    """Every case of scale_chain_util.cases(model) at B = 65 on the fine tables, on every route of the model: without
    vertex weights k_accum_w_bm<.., false, true> (the unweighted EXTRAS form), with them <.., true, true>; joints omitted
    (k_scale_refs regressed); a warm start; scale_regularizer 0.5; no ridge; the wave-only instantiations of
    k_scale_extras under the ridge of scale_chain_util.ridge.
    (observed maxima per model, route and step, the fp32 oracle's in brackets: DESIGN.md §5)"""
    with capsys.disabled():
        print()
        check_case(name, case, X.MODES[mode], 65, route, None, model_root, golden, dev, smplfit_env)


@pytest.mark.parametrize('mode', X.MODES)
def test_chain_general(mode, model_root, golden, dev, smplfit_env, capsys):
    """smpl_b32 (33 shape unknowns with the scale: the general path's k_shape_solve_scaled<true>), 'pose1', B = 65."""
    with capsys.disabled():
        print()
        check_case('smpl_b32', X.Case('pose1'), X.MODES[mode], 65, 'own', None, model_root, golden, dev, smplfit_env)


BATCHES = ([('smpl', Bn, fb) for Bn, fb in ((1, None), (63, None), (129, None), (65, '0'), (129, '0'))] +
           [('smplxfat', 63, None), ('smplxfat', 129, '0')])


@pytest.mark.parametrize('mode', X.MODES)
@pytest.mark.parametrize('case', X.few_cases(), ids=lambda c: c.id)
@pytest.mark.parametrize('route', ['bm', 'wave'])
@pytest.mark.parametrize('name,Bn,fine_b', BATCHES)
def test_chain_batches(name, Bn, fine_b, route, case, mode, model_root, golden, dev, smplfit_env, capsys):
    """The other batches on four cases per route: 1 (63 pad lanes, k_accum_combine's narrow width), 63 (a wave short of
    one lane), 129 (Mp = 256: a third block of one lane) on the fine tables; 65 and 129 on the coarse ones, where the
    unscaled solve of C and D is k_solve_bm behind k_joint_stage + k_jd_transpose (counted)."""
    with capsys.disabled():
        print()
        check_case(name, case, X.MODES[mode], Bn, route, fine_b, model_root, golden, dev, smplfit_env)


@pytest.mark.parametrize('mode', X.MODES)
@pytest.mark.parametrize('route', ['bm', 'wave'])
def test_chain_two_chunks(route, mode, model_root, golden, dev, smplfit_env, two_chunks, capsys):
    """SMPL 'hard_pose', B = 65 as two concurrent chunks (33 + 32 rows, each with its own workspace slice)."""
    with capsys.disabled():
        print()
        check_case('smpl', X.Case('hard_pose'), X.MODES[mode], 65, route, None, model_root, golden, dev, smplfit_env, chunks=2)


@pytest.mark.parametrize('mode', X.MODES)
@pytest.mark.parametrize('name', X.FULL)
def test_routes_differ(name, mode, model_root, golden, dev, smplfit_env):
    """SMPLFIT_BM_SCALE=0 takes other kernels for the extra sums and the solve: somewhere in SS1 / SS2 the two routes
    differ in bits (they sum in another order) — the only evidence of which extras kernel ran, these kernels having no
    counter —, with target joints and without them."""
    c, f = setup(name, model_root, golden, dev)
    for case in (X.Case('hard_pose'), X.Case('pose1', joints=False)):
        outs = {}
        for route in ('bm', 'wave'):
            set_route(smplfit_env, route, None)
            outs[route] = clean_calls(name, c, f, case, X.MODES[mode], 65, dev, smplfit_env, route, None)
        differs = any(not torch.equal(outs['bm'][call][k], outs['wave'][call][k]) for call in 'AC'
                      for k in ('shape_betas', 'trans', 'scale_corr'))
        assert differs, (name, case.id, 'SMPLFIT_BM_SCALE=0 changed nothing: the batch-major route did not run')


@pytest.mark.parametrize('mode', X.MODES)
@pytest.mark.parametrize('route', ['bm', 'wave'])
@pytest.mark.parametrize('Bn,row', [(65, 5), (65, 62), (65, 63), (65, 64), (129, 128)])
def test_poisoned_row(Bn, row, route, mode, model_root, golden, dev, smplfit_env):
    """SMPL 'pose1', one instance with NaN targets, vertices and joints: inside a wave, its last two lanes, the single
    lane of the second block, and row 128 of 129.  Every other row of SS0, A, B, C (and D) is bit-identical to the
    clean calls in all outputs, and the poisoned row's own scale_corr is non-finite in all four."""
    c, f = setup('smpl', model_root, golden, dev)
    set_route(smplfit_env, route, None)
    case, m = X.Case('pose1'), X.MODES[mode]
    clean = clean_calls('smpl', c, f, case, m, Bn, dev, smplfit_env, route, None)
    dirty = run_calls(c, f, 'smpl', case, m, rows_of(Bn), dev, smplfit_env, route, None, poison_row=row)
    keep = torch.arange(Bn, device=dev) != row
    for call, o0 in clean.items():
        for k in o0:
            assert torch.isfinite(o0[k]).all(), (call, k)
            assert torch.equal(dirty[call][k][keep], o0[k][keep]), (row, call, k)
        if call != 'D':
            assert not torch.isfinite(dirty[call]['scale_corr'][row]), (row, call)


SHARED = {'B65': (65, True), 'B129': (129, True), 'segments_3_62': (65, [3, 62])}


@pytest.mark.parametrize('mode', X.MODES)
@pytest.mark.parametrize('route', ['bm', 'wave'])
@pytest.mark.parametrize('how', SHARED)
def test_shared_scaled_solve(how, route, mode, model_root, golden, dev, smplfit_env, capsys):
    """SS0 with share_beta (k_shape_solve_scaled, share = 1 | 2: one shape for the batch or the segment, a scale per
    instance) on SMPL 'pose1', against the oracle's partially shared branch on the whole tiled batch (fit_shape per
    segment): B = 65, 129 and share_beta_segments=[3, 62].  Rows of one segment share their betas bit for bit."""
    Bn, share = SHARED[how]
    c, f = setup('smpl', model_root, golden, dev)
    set_route(smplfit_env, route, None)
    case, m, rows = X.Case('pose1'), X.MODES[mode], rows_of(Bn)
    out = to_np(run_calls(c, f, 'smpl', case, m, rows, dev, smplfit_env, route, None, share=share)['SS0'])
    segments = None if share is True else share
    for i, j in zip(np.cumsum([0] + (segments or [Bn]))[:-1], np.cumsum(segments or [Bn])):
        assert (out['shape_betas'][i:j] == out['shape_betas'][i]).all(), (how, i, j)
    r64, r32 = X.refs(c, 'smpl', case, rows)
    G = out['orientations']
    with capsys.disabled():
        print()
        X.check_solve('smpl', case, f'SS0 shared {how}', c['om64'], out, m, r32.solve(G, m, 'known_pose', True, segments),
                      r64.solve(G, m, 'known_pose', True, segments), f'device {route}')


@MIRROR_LOOSE
@pytest.mark.parametrize('mode', X.MODES)
@pytest.mark.parametrize('name,route,step', [k + (s,) for k, steps in KNOWN_MISS.items() for s in steps], ids=lambda v: str(v))
def test_known_miss(name, route, step, mode, model_root, golden, dev, smplfit_env, capsys):
    """The step of 'mirror' whose distance gate misses on a loose pair (KNOWN_MISS): every other gate of the case is
    asserted by test_chain_families; this raises the deferred assertion of that step, unchanged."""
    with capsys.disabled():
        figs = check_case(name, X.Case('mirror'), X.MODES[mode], 65, route, None, model_root, golden, dev, smplfit_env)
    if step in figs['deferred']:
        raise figs['deferred'][step]
