"""-m gpu: ``share_beta`` over segments of the batch (``share_beta_segments``).  The strongest check there
is: every row of a segment inside a larger batch carries exactly the bits of a stand-alone ``share_beta`` call on the
segment's rows — every other kernel keeps a row independent of its batch (tests/test_gpu_parity.py pins that), and the
segmented sum adds a segment's systems in the order the stand-alone call does.  Shapes are the smallest that cross
every boundary of the sum: the 64-row block, the 8-way unroll tail, the general path's 256-row chunk."""

import ctypes as C

import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu

MIXED = [1, 63, 64, 65, 7, 129, 8, 2]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


_models = {}


def get_model(model_root, name, dev, num_betas=10):
    from smplfitter_amd.pt import BodyFitter, BodyModel

    if name not in _models:
        kind = 'smplx' if name.startswith('smplx') else 'smpl'
        m = BodyModel(kind, 'neutral', model_root=f'{model_root}/{util.model_dir(name) if num_betas == 10 else name}',
                      num_betas=num_betas, device=dev)
        _models[name] = (m, BodyFitter(m), BodyFitter(m, enable_kid=True))
    return _models[name]


def t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def make_targets(m, B, seed, dev, noise=0.003, nb=10):
    """Seeded noisy targets with joints; every row its own pose and shape."""
    rs = np.random.RandomState(seed)
    J = m.num_joints
    fw = m(t((rs.randn(B, 3 * J) * 0.1).astype(np.float32), dev), t((rs.randn(B, nb) * 0.5).astype(np.float32), dev),
           t(rs.randn(B, 3).astype(np.float32), dev))
    g = torch.Generator(device='cpu').manual_seed(seed)
    return fw['vertices'] + (torch.randn(fw['vertices'].shape, generator=g) * noise).to(dev), fw['joints']


def rows(v, a, b):
    return v[a:b] if isinstance(v, torch.Tensor) else v


def assert_segments_equal_alone(call, sizes, row_kw, opt_kw, what):
    """``call(share_beta_segments=sizes)`` on the whole batch against ``call(share_beta=True)`` on every segment's rows:
    every result key, ``torch.equal``.  row_kw: the per-row tensors (sliced for the stand-alone calls)."""
    whole = call(**row_kw, **opt_kw, share_beta_segments=sizes)
    a = 0
    for g, n in enumerate(sizes):
        alone = call(**{k: rows(v, a, a + n) for k, v in row_kw.items()}, **opt_kw, share_beta=True)
        assert set(alone) == set(whole), (what, sorted(alone), sorted(whole))
        for k in alone:
            assert torch.equal(whole[k][a:a + n], alone[k]), \
                f'{what}: segment {g} ({n} rows from {a}), {k}: max |diff| {(whole[k][a:a + n] - alone[k]).abs().max().item():.3e}'
        assert (whole['shape_betas'][a:a + n] - whole['shape_betas'][a]).abs().max().item() == 0, (what, g)
        a += n
    return whole


def test_bit_identity_smpl_mixed(model_root, dev):
    """SMPL (batch-major path), joints, num_iter=2, sizes [1,63,64,65,7,129,8,2] (B = 339): every result key of every
    segment equals the stand-alone share_beta call on its rows, bit for bit."""
    m, f, _ = get_model(model_root, 'smpl', dev)
    tv, tj = make_targets(m, sum(MIXED), 41, dev)
    whole = assert_segments_equal_alone(f.fit, MIXED, dict(target_vertices=tv, target_joints=tj),
                                        dict(num_iter=2, beta_regularizer=1.0), 'smpl mixed')
    assert set(whole) == {'pose_rotvecs', 'shape_betas', 'trans', 'orientations', 'relative_orientations'}
    # the segments do get different shapes (the rows come from different bodies)
    assert (whole['shape_betas'][0] - whole['shape_betas'][1]).abs().max().item() > 1e-3


def test_single_segment_and_singletons(model_root, dev):
    """Segments [B] are share_beta=True bitwise (also with a CPU integer tensor for the sizes); [1] * 5 are five
    one-row share calls."""
    m, f, _ = get_model(model_root, 'smpl', dev)
    B = 70
    tv, tj = make_targets(m, B, 42, dev)
    kw = dict(num_iter=2, beta_regularizer=0.5)
    ref = f.fit(tv, tj, share_beta=True, **kw)
    for sizes in ([B], torch.tensor([B]), torch.tensor([B], dtype=torch.int32)):
        o = f.fit(tv, tj, share_beta_segments=sizes, **kw)
        for k in ref:
            assert torch.equal(o[k], ref[k]), k
    assert_segments_equal_alone(f.fit, [1] * 5, dict(target_vertices=tv[:5], target_joints=tj[:5]), kw, 'singletons')


def test_bit_identity_smplx(model_root, dev):
    m, f, _ = get_model(model_root, 'smplx', dev)
    tv, tj = make_targets(m, 8, 43, dev)
    assert_segments_equal_alone(f.fit, [3, 5], dict(target_vertices=tv, target_joints=tj), dict(num_iter=2), 'smplx')


def test_bit_identity_kid_weights(model_root, dev):
    """Kid plus both weights (the wave-per-instance fallbacks of the weighted solve), beta_regularizer2, no final
    refinement, [5, 3]."""
    m, _, kf = get_model(model_root, 'smpl', dev)
    tv, tj = make_targets(m, 8, 44, dev)
    g = torch.Generator(device='cpu').manual_seed(44)
    vw = (torch.rand(8, m.num_vertices, generator=g) + 0.2).to(dev)
    jw = (torch.rand(8, m.num_joints, generator=g) + 0.2).to(dev)
    whole = assert_segments_equal_alone(
        kf.fit, [5, 3], dict(target_vertices=tv, target_joints=tj, vertex_weights=vw, joint_weights=jw),
        dict(num_iter=2, beta_regularizer=0.7, beta_regularizer2=0.1, kid_regularizer=2.0, final_adjust_rots=False), 'kid + weights')
    assert 'kid_factor' in whole
    assert (whole['kid_factor'][:5] - whole['kid_factor'][0]).abs().max().item() == 0  # one kid factor per segment


@pytest.mark.parametrize('case', ['a', 'b'])
def test_bit_identity_scale(case, model_root, golden, dev):
    """scale_target (case a) and scale_fit with kid, weights and a warm start (case b) over [8, 8]: two differently
    noised copies of util.share_scale_inputs — one shape per segment, one scale per row."""
    g = golden('smpl')
    kind, md = util.load_md(model_root, 'smpl', g)
    om, _ = util.make_oracle(md, kind)
    m, f, kf = get_model(model_root, 'smpl', dev)
    kid_fit, tv, kw = util.share_scale_inputs(g, om, case)
    rs = np.random.RandomState(5)
    tv2 = (tv + rs.randn(*tv.shape) * 0.004).astype(np.float32)
    row_kw = {k: t(np.concatenate([v, v]), dev) for k, v in kw.items() if isinstance(v, np.ndarray)}
    row_kw['target_vertices'] = t(np.concatenate([tv, tv2]), dev)
    opt_kw = {k: v for k, v in kw.items() if not isinstance(v, np.ndarray) and v is not None}
    whole = assert_segments_equal_alone((kf if kid_fit else f).fit, [8, 8], row_kw, opt_kw, f'share + scale {case}')
    assert 'scale_corr' in whole and (whole['scale_corr'][:8] - whole['scale_corr'][0]).abs().max().item() > 0
    assert (whole['shape_betas'][0] - whole['shape_betas'][8]).abs().max().item() > 0


def test_bit_identity_known_pose(model_root, dev):
    """fit_with_known_pose over [3, 5], plain and with scale_target (the partially shared solve)."""
    m, f, _ = get_model(model_root, 'smpl', dev)
    rs = np.random.RandomState(45)
    pose = t((rs.randn(8, 3 * m.num_joints) * 0.1).astype(np.float32), dev)
    fw = m(pose, t((rs.randn(8, 10) * 0.5).astype(np.float32), dev), t(rs.randn(8, 3).astype(np.float32), dev))
    tv = fw['vertices'] * 1.05 + t((rs.randn(8, m.num_vertices, 3) * 0.003).astype(np.float32), dev)
    row_kw = dict(pose_rotvecs=pose, target_vertices=tv, target_joints=fw['joints'] * 1.05)
    assert_segments_equal_alone(f.fit_with_known_pose, [3, 5], row_kw, dict(beta_regularizer=1.0), 'known pose')
    assert_segments_equal_alone(f.fit_with_known_pose, [3, 5], row_kw, dict(beta_regularizer=0.5, scale_target=True),
                                'known pose + scale')


def test_bit_identity_general_path(model_root, dev):
    """smpl_b32 (general path: 33 > 17 unknowns) over [300, 5, 70]: the workspace holds 256 system rows, so the first
    segment's blocks are summed in two groups and the last group holds blocks of all three segments."""
    from smplfitter_amd import _lib

    m, f, _ = get_model(model_root, 'smpl_b32', dev, num_betas=32)
    assert m._native(dev).info.vertex_path == _lib.SMPLFIT_PATH_GENERAL
    sizes = [300, 5, 70]
    tv, tj = make_targets(m, sum(sizes), 46, dev, nb=32)
    assert_segments_equal_alone(f.fit, sizes, dict(target_vertices=tv, target_joints=tj),
                                dict(num_iter=2, beta_regularizer=1.0), 'general path')


def surround(arr, pre, post):
    """The fixture's 8 rows between rows `pre` and `post`."""
    return np.concatenate([pre, arr, post]).astype(np.float32)


def test_reference_parity_middle_segment(model_root, golden, dev):
    """The fixture batch of util.share_inputs (8 rows) as the middle segment between two other bodies meets
    util.check_share against the reference's goldens, gates unchanged."""
    g, ge = golden('smpl'), golden('ext_smpl')
    kind, md = util.load_md(model_root, 'smpl', g)
    om, _ = util.make_oracle(md, kind)
    m, f, kf = get_model(model_root, 'smpl', dev)
    n = 0
    for case in util.SHARE_CASES:
        if f'share.{case}.trans' not in ge:
            continue
        kid_fit, tv, kw = util.share_inputs(g, om, case)
        a = om.forward(g['pose'][:5], np.repeat(g['betas'][1:2], 5, 0), g['trans'][:5])
        b = om.forward(g['pose'][5:8], np.repeat(g['betas'][2:3], 3, 0), g['trans'][5:8])
        kwt = {}
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                v = surround(v, a['joints'], b['joints']) if k == 'target_joints' else surround(v, v[:5], v[5:8])
                v = t(v, dev)
            kwt[k] = v
        o = (kf if kid_fit else f).fit(t(surround(tv, a['vertices'], b['vertices']), dev), share_beta_segments=[5, 8, 3],
                                       requested_keys=['pose_rotvecs'], **kwt)
        util.check_share(om, 'smpl', case, {k: v[5:13].cpu().numpy() for k, v in o.items()}, ge, kid_fit)
        n += 1
    assert n >= 1


def test_reference_parity_scale_middle_segment(model_root, golden, dev):
    """The same for util.share_scale_inputs / util.check_share_scale (one shape per segment, one scale per row)."""
    g, gk = golden('smpl'), golden('kp_smpl')
    kind, md = util.load_md(model_root, 'smpl', g)
    om, _ = util.make_oracle(md, kind)
    m, f, kf = get_model(model_root, 'smpl', dev)
    n = 0
    for case in util.SHARE_SCALE_CASES:
        if f'sharescale.{case}.trans' not in gk:
            continue
        kid_fit, tv, kw = util.share_scale_inputs(g, om, case)
        s = np.float32(1.1)
        a = om.forward(g['pose'][:5], np.repeat(g['betas'][1:2], 5, 0), g['trans'][:5])
        b = om.forward(g['pose'][5:8], np.repeat(g['betas'][2:3], 3, 0), g['trans'][5:8])
        kwt = {}
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                v = surround(v, a['joints'] * s, b['joints'] * s) if k == 'target_joints' else surround(v, v[:5], v[5:8])
                v = t(v, dev)
            kwt[k] = v
        o = (kf if kid_fit else f).fit(t(surround(tv, a['vertices'] * s, b['vertices'] * s), dev),
                                       share_beta_segments=[5, 8, 3], requested_keys=['pose_rotvecs'], **kwt)
        util.check_share_scale(om, 'smpl', case, {k: v[5:13].cpu().numpy() for k, v in o.items()}, gk, kid_fit)
        n += 1
    assert n >= 1


def test_run_to_run_and_workspace(model_root, dev):
    """Identical from run to run; identical with a caller-supplied ``_workspace`` zero-filled and NaN-filled (nothing
    is read before it is written, the plan's partial rows and sums included); a workspace of the unsegmented query's
    size is refused."""
    m, f, _ = get_model(model_root, 'smpl', dev)
    sizes = [65, 3, 1, 64]
    B = sum(sizes)
    tv, tj = make_targets(m, B, 47, dev)
    kw = dict(num_iter=2, share_beta_segments=sizes)
    ref = f.fit(tv, tj, **kw)
    again = f.fit(tv, tj, **kw)
    h = m._native(dev)
    plan = f._segment_plan(dev, tuple(sizes))
    need = plan.workspace_bytes(h)
    assert need > h.workspace_bytes(B)
    results = [again]
    for fill in (0, 0xFF):  # (0xFF bytes: NaN in fp32 and fp64)
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
        results.append(f.fit(tv, tj, _workspace=ws, **kw))
        assert not torch.equal(ws, torch.full_like(ws, fill))  # the caller's tensor was the workspace
    for o in results:
        for k in ref:
            assert torch.equal(o[k], ref[k]), k
            assert torch.isfinite(o[k]).all(), k
    with pytest.raises(RuntimeError, match='workspace'):
        f.fit(tv, tj, _workspace=torch.empty(h.workspace_bytes(B), dtype=torch.uint8, device=dev), **kw)


def test_refusals_enqueue_nothing(model_root, dev):
    """Refusals come before anything is enqueued: the pre-filled outputs of a refused C-ABI call are untouched, and the
    Python argument errors are raised for device tensors as for CPU ones."""
    from smplfitter_amd import _lib

    m, f, _ = get_model(model_root, 'smpl', dev)
    lib, h = _lib.load(), m._native(dev)
    B = 6
    tv, tj = make_targets(m, B, 48, dev)
    good, other = _lib.ShareSegments([2, 4]), _lib.ShareSegments([2, 5])
    ws = torch.empty(max(good.workspace_bytes(h), other.workspace_bytes(m._native(dev))), dtype=torch.uint8, device=dev)
    out = {k: torch.full(s, 7.0, device=dev) for k, s in dict(p=(B, 72), b=(B, 10), t=(B, 3)).items()}
    G = m(torch.zeros(B, 72, device=dev), return_vertices=False)['orientations'].contiguous()

    def fit_args(**over):
        a = _lib.FitArgs(target_vertices=tv.data_ptr(), batch=B, num_iter=1, beta_regularizer=1.0, final_adjust_rots=1,
                         pose_rotvecs=out['p'].data_ptr(), shape_betas=out['b'].data_ptr(), trans=out['t'].data_ptr(),
                         workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def solve_args(**over):
        a = _lib.ShapeSolveArgs(glob_rotmats=G.data_ptr(), target_vertices=tv.data_ptr(), batch=B, beta_regularizer=1.0,
                                shape_betas=out['b'].data_ptr(), trans=out['t'].data_ptr(), workspace=ws.data_ptr(),
                                workspace_bytes=ws.numel())
        for k, v in over.items():
            setattr(a, k, v)
        return a

    cb = _lib.ShareAllreduceFn(lambda *a: 0)
    small = good.workspace_bytes(h) - 256
    for fn, args in ((lib.smplfit_fit_segments_f32, fit_args), (lib.smplfit_shape_solve_segments_f32, solve_args)):
        assert fn(h.ptr, C.byref(args()), other.ptr) == _lib.SMPLFIT_ERR_BAD_ARG          # the plan's batch is 7
        assert fn(h.ptr, C.byref(args(share_allreduce=cb)), good.ptr) == _lib.SMPLFIT_ERR_BAD_ARG
        assert fn(h.ptr, C.byref(args(workspace_bytes=small)), good.ptr) == _lib.SMPLFIT_ERR_WORKSPACE
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == 7.0).all(), k
    # ... and the valid calls do write them
    assert lib.smplfit_fit_segments_f32(h.ptr, C.byref(fit_args()), good.ptr) == 0
    torch.cuda.synchronize()
    assert not (out['b'] == 7.0).any() and (out['b'][2:] == out['b'][2]).all() and not torch.equal(out['b'][0], out['b'][2])
    fit_b = out['b'].clone()
    out['b'].fill_(7.0)
    assert lib.smplfit_shape_solve_segments_f32(h.ptr, C.byref(solve_args()), good.ptr) == 0
    torch.cuda.synchronize()
    assert not (out['b'] == 7.0).any() and (out['b'][2:] == out['b'][2]).all() and not torch.equal(out['b'], fit_b)
    for bad in ([2, 3], [6, 0], [3, 3, 1]):
        with pytest.raises(ValueError, match='share_beta_segments'):
            f.fit(tv, tj, share_beta_segments=bad)
    with pytest.raises(ValueError, match='share_beta_group'):
        f.fit(tv, tj, share_beta_segments=[6], share_beta_group=object())
    with pytest.raises(NotImplementedError, match='share_beta'):
        f.fit(tv.clone().requires_grad_(True), tj, share_beta_segments=[6])
    good.close()
    other.close()


def test_plan_cache_bounded(model_root, dev):
    """Plans are cached per (device, sizes), least recently used dropped beyond MAX_SEGMENT_PLANS."""
    from smplfitter_amd.pt import BodyFitter

    m, _, _ = get_model(model_root, 'smpl', dev)
    f = BodyFitter(m)
    B = f.MAX_SEGMENT_PLANS + 4
    tv, tj = make_targets(m, B, 49, dev)
    first = f.fit(tv, tj, share_beta_segments=[1, B - 1])
    plan = f._segment_plans[(0, (1, B - 1))]
    f.fit(tv, tj, share_beta_segments=[1, B - 1])
    assert f._segment_plans[(0, (1, B - 1))] is plan and len(f._segment_plans) == 1
    for k in range(2, B - 1):
        f.fit(tv, tj, share_beta_segments=[k, B - k])
    assert len(f._segment_plans) == f.MAX_SEGMENT_PLANS and (0, (1, B - 1)) not in f._segment_plans
    again = f.fit(tv, tj, share_beta_segments=[1, B - 1])  # (rebuilt)
    for k in first:
        assert torch.equal(first[k], again[k]), k
