"""-m gpu: the mesh-error step — ``BodyFitter.fit(requested_keys=[... 'vertices', 'joints',
'vertex_error', 'joint_error'])`` (smplfit_fit_recon_f32), ``BodyModel.mesh_error`` (smplfit_mesh_error_f32) and the
same keys of fit_with_known_pose / fit_with_known_shape.

Targets: seeded forward meshes plus 2 mm noise (as ``meshes()`` of tests/test_gpu_hand_replacer.py), instance
``util.FWD_FAR`` translated by ~1000 m.

Against fp64: ``util.forward64`` at the RETURNED fp32 parameters (glob_rotmats = orientations).
  vertices, joints   util.forward_excess(...) <= util.FWD_GATE_M: the gate BodyModel.forward is held to.
  vertex_error, joint_error, per element, with ref_e = |v64 - target| in fp64:
      |ours - ref_e| <= sqrt(3) (FWD_GATE_M + 4 ulp32(largest |coordinate| of the point)) + 4 ulp32(ref_e)
  the triangle inequality over the forward's own gate (the fp32 difference mesh - target rounds once more, on
  coordinates no larger than the point's largest), plus the rounding of the result.
Rows: every row up to 129 instances, above that the rows of ``util.forward_rows``.
Observed on one MI355X over all cases (printed as ``[recon]`` lines): forward excess of vertices at most 9.5e-7 m
(SMPL-X-fat; SMPL 5.0e-7) and of joints 1.2e-7 m against the 2e-6 m gate; every error at least 2.9e-6 m inside its gate.

Identity: the fit's ordinary keys are the bits of the call without the new keys; the new keys of ``fit`` are the bits of
``mesh_error`` at its results (the same step), and ``vertices`` / ``joints`` those of ``BodyModel.forward`` at them (the
same passes write them) — on every route tested here."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import util
from test_gpu_forward import _model
from test_gpu_hand_replacer import two_chunk_batch

pytestmark = pytest.mark.gpu

RECON = ['vertices', 'joints', 'vertex_error', 'joint_error']
ORDINARY = ['pose_rotvecs', 'shape_betas', 'trans', 'orientations', 'relative_orientations']
FIT = dict(num_iter=3, beta_regularizer=1.0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


_fitters, _targets = {}, {}


def fitter_of(m, kid=False):
    from smplfitter_amd.pt import BodyFitter

    if (id(m), kid) not in _fitters:
        _fitters[id(m), kid] = BodyFitter(m, enable_kid=kid)
    return _fitters[id(m), kid]


def targets(name, m, B, dev, seed=0):
    """(target_vertices, target_joints) of B instances: a seeded forward plus 2 mm of noise, FWD_FAR ~1000 m away.
    Computed once per (model, batch, seed) and never written to."""
    key = (name, B, seed)
    if key not in _targets:
        rs = np.random.RandomState(100 + seed)
        J, V, S = m.num_joints, m.num_vertices, m.num_betas
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
        trans = rs.randn(B, 3)
        if B > util.FWD_FAR:
            trans[util.FWD_FAR] += (1000.0, -1000.0, 1000.0)
        fw = m(t(rs.randn(B, 3 * J) * 0.1), t(rs.randn(B, S) * 0.5), t(trans))
        _targets[key] = (fw['vertices'] + t(rs.randn(B, V, 3) * 0.002), fw['joints'] + t(rs.randn(B, J, 3) * 0.002))
    return _targets[key]


def rows_of(B):
    return np.arange(B) if B <= 129 else util.forward_rows(B)


def error_gate(ref_pts, ref_e):
    """The per-element gate of an error (module docstring); ref_pts (n, P, 3) fp64, ref_e (n, P)."""
    coord = np.abs(ref_pts).max(-1)
    ulp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)  # noqa: E731
    return math.sqrt(3.0) * (util.FWD_GATE_M + 4 * ulp(coord)) + 4 * ulp(ref_e)


def check_fp64(om, res, params, tv, tj, B, tag):
    """The recon keys of ``res`` against forward64 at ``params`` (tensors: glob_rotmats, shape_betas, trans and maybe
    kid_factor) on the rows of the batch; prints each figure, then asserts."""
    rows = rows_of(B)
    ti = torch.from_numpy(rows).to(tv.device)
    p = {k: v[ti].cpu().numpy() for k, v in params.items() if v is not None}
    ref = util.forward64(om, **p)
    worst = {}
    for key, pts in (('vertices', 'vertices'), ('joints', 'joints')):
        if key in res:
            worst[key] = util.forward_excess(res[key][ti].cpu().numpy(), ref[pts])
    for key, pts, tgt in (('vertex_error', 'vertices', tv), ('joint_error', 'joints', tj)):
        if key in res:
            t64 = tgt[ti].cpu().numpy().astype(np.float64)
            ref_e = np.linalg.norm(ref[pts] - t64, axis=-1)
            ours = res[key][ti].cpu().numpy().astype(np.float64)
            assert ours.shape == ref_e.shape and np.isfinite(ours).all(), (tag, key)
            worst[key] = float((np.abs(ours - ref_e) - error_gate(ref[pts], ref_e)).max())
    print(f'[recon] {tag} B = {B}: ' + ', '.join(f'{k} {v:+.2e}' for k, v in worst.items()) +
          f' (mesh excess gate {util.FWD_GATE_M:.0e}, error excess gate 0)')
    for key, v in worst.items():
        assert v <= (util.FWD_GATE_M if key in ('vertices', 'joints') else 0.0), (tag, key, v)


def fit_params(res):
    return dict(glob_rotmats=res['orientations'], shape_betas=res['shape_betas'], trans=res['trans'],
                kid_factor=res.get('kid_factor'))


def check_fit(name, m, om, B, dev, joints=True, kid=False, tag=None, **opts):
    """One fit with every recon key its targets allow: fp64 gates, and the three identities."""
    f = fitter_of(m, kid)
    tv, tj = targets(name, m, B, dev)
    tj = tj if joints else None
    keys = [k for k in RECON if joints or k != 'joint_error']
    kw = dict(FIT, **opts)
    res = f.fit(tv, tj, requested_keys=['pose_rotvecs'] + keys, **kw)
    assert all(k in res for k in keys) and (joints or 'joint_error' not in res)
    check_fp64(om, res, fit_params(res), tv, tj, B, tag or name)
    plain = f.fit(tv, tj, requested_keys=['pose_rotvecs'], **kw)
    assert not set(plain) & set(RECON)
    for k in plain:
        assert torch.equal(res[k], plain[k]), (name, k)
    p = fit_params(res)
    me = m.mesh_error(tv, tj, return_mesh=True, **p)
    for k in keys:
        assert torch.equal(res[k], me[k]), (name, k)
    fw = m(**p)
    assert torch.equal(res['vertices'], fw['vertices']) and torch.equal(res['joints'], fw['joints'])
    return res


@pytest.mark.parametrize('B', [1, 3, 65, 129])
def test_smpl_batch_edges(B, model_root, golden, dev, smplfit_env):
    """SMPL on the batch-major route at partial 64- and 128-instance blocks, with target joints."""
    smplfit_env('SMPLFIT_BM', None)
    m, om = _model('smpl', model_root, golden, dev)
    assert m.kernel_path() == 'batch-major'
    check_fit('smpl', m, om, B, dev)


@pytest.mark.usefixtures('two_chunks')
def test_two_chunks(model_root, golden, dev):
    """Just above the smallest batch that is cut into two chunks: the chunks are joined before the step runs over the
    whole batch in the same workspace."""
    m, om = _model('smpl', model_root, golden, dev)
    check_fit('smpl', m, om, two_chunk_batch(), dev, tag='smpl two chunks')


@pytest.mark.parametrize('name,B,joints', [('smplxfat', 67, True), ('smpl1024', 67, True), ('smpl_b32', 5, True),
                                            ('smpl_w12', 5, True), ('smpl', 67, False), ('smplxfat', 3, False)])
def test_models_and_routes(name, B, joints, model_root, golden, dev):
    """SMPL-X-fat (tiled GEMM), the 1024-vertex subset (V a multiple of the padding), the general path, and fits
    without target joints."""
    m, om = _model(name, model_root, golden, dev)
    check_fit(name, m, om, B, dev, joints=joints)


def test_wave_route(model_root, golden, dev, smplfit_env):
    """SMPL with SMPLFIT_BM=0: the wave-per-instance forward pass writes the mesh, a plain kernel takes the distances."""
    smplfit_env('SMPLFIT_BM', '0')
    m, om = _model('smpl', model_root, golden, dev)
    check_fit('smpl', m, om, 67, dev, tag='smpl wave')
    tv, _ = targets('smpl', m, 67, dev)
    only = fitter_of(m).fit(tv, requested_keys=['vertex_error'], **FIT)  # the mesh goes to the workspace
    full = fitter_of(m).fit(tv, requested_keys=['vertex_error', 'vertices'], **FIT)
    assert torch.equal(only['vertex_error'], full['vertex_error'])


def test_enable_kid(model_root, golden, dev):
    m, om = _model('smpl', model_root, golden, dev)
    res = check_fit('smpl', m, om, 65, dev, kid=True, tag='smpl kid')
    assert 'kid_factor' in res


def test_weights_do_not_enter(model_root, golden, dev):
    """With both weights the errors are the unweighted distances at the weighted fit's parameters."""
    m, om = _model('smpl', model_root, golden, dev)
    B = 65
    g = torch.Generator(device='cpu').manual_seed(3)
    vw = (torch.rand(B, m.num_vertices, generator=g) + 0.25).to(dev)
    jw = (torch.rand(B, m.num_joints, generator=g) + 0.25).to(dev)
    check_fit('smpl', m, om, B, dev, tag='smpl weighted', vertex_weights=vw, joint_weights=jw)


def test_share_beta_segments(model_root, golden, dev):
    m, om = _model('smpl', model_root, golden, dev)
    res = check_fit('smpl', m, om, 8, dev, tag='smpl segments', share_beta_segments=[3, 5])
    assert torch.equal(res['shape_betas'][0], res['shape_betas'][2]) and torch.equal(res['shape_betas'][3], res['shape_betas'][7])
    check_fit('smpl', m, om, 8, dev, tag='smpl share_beta', share_beta=True)


def test_warm_start(model_root, golden, dev):
    m, om = _model('smpl', model_root, golden, dev)
    tv, tj = targets('smpl', m, 3, dev)
    first = fitter_of(m).fit(tv, tj, **FIT)
    check_fit('smpl', m, om, 3, dev, tag='smpl warm', initial_pose_rotvecs=first['pose_rotvecs'],
              initial_shape_betas=first['shape_betas'])


def test_single_keys_and_determinism(model_root, golden, dev):
    """Each key on its own is the key of the full request; two runs give the same bits."""
    m, om = _model('smpl', model_root, golden, dev)
    f = fitter_of(m)
    tv, tj = targets('smpl', m, 65, dev)
    full = f.fit(tv, tj, requested_keys=RECON, **FIT)
    again = f.fit(tv, tj, requested_keys=RECON, **FIT)
    assert 'pose_rotvecs' not in full
    for k in full:
        assert torch.equal(full[k], again[k]), k
    for k in RECON:
        one = f.fit(tv, tj, requested_keys=[k], **FIT)
        assert [r for r in RECON if r in one] == [k]
        assert torch.equal(one[k], full[k]), k
    me = m.mesh_error(tv, tj, **fit_params(full))
    assert sorted(me) == ['joint_error', 'vertex_error']
    assert sorted(m.mesh_error(tv, **fit_params(full))) == ['vertex_error']


def test_caller_workspace(model_root, golden, dev):
    """A zeroed and a NaN-filled caller workspace of the new query's size give the same bits; the fit's own size is too
    small and gives the workspace error."""
    from smplfitter_amd import _lib

    m, om = _model('smpl', model_root, golden, dev)
    f = fitter_of(m)
    B = 65
    tv, tj = targets('smpl', m, B, dev)
    h = m._native(dev)
    n = h.fit_recon_workspace_bytes(B)
    assert n > h.workspace_bytes(B)
    zero = torch.zeros(n, dtype=torch.uint8, device=dev)
    nan = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
    a = f.fit(tv, tj, requested_keys=RECON, _workspace=zero, **FIT)
    b = f.fit(tv, tj, requested_keys=RECON, _workspace=nan, **FIT)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    small = torch.zeros(h.workspace_bytes(B), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.SmplfitError, match='workspace too small'):
        f.fit(tv, tj, requested_keys=RECON, _workspace=small, **FIT)
    f.fit(tv, tj, _workspace=small, **FIT)  # without the keys: today's call, today's size


def _c_fit_recon(m, dev, tv, tj, outs, scale_mode=0):
    """smplfit_fit_recon_f32 on caller-made outputs; returns (status, the fit's outputs)."""
    from smplfitter_amd import _lib

    B, J, S = tv.shape[0], m.num_joints, m.num_betas
    h = m._native(dev)
    new = lambda *sh: torch.full(sh, float('nan'), dtype=torch.float32, device=dev)  # noqa: E731
    fit = dict(pose_rotvecs=new(B, 3 * J), shape_betas=new(B, S), trans=new(B, 3), orientations=new(B, J, 3, 3))
    scale = new(B)
    ws = torch.empty(h.fit_recon_workspace_bytes(B), dtype=torch.uint8, device=dev)
    args = _lib.FitArgs(target_vertices=tv.data_ptr(), target_joints=None if tj is None else tj.data_ptr(), batch=B,
                        num_iter=3, beta_regularizer=1.0, final_adjust_rots=1, scale_mode=scale_mode,
                        scale_corr=scale.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                        hip_stream=torch.cuda.current_stream(dev).cuda_stream, **{k: v.data_ptr() for k, v in fit.items()})
    rargs = _lib.FitReconArgs(**{k: v.data_ptr() for k, v in outs.items()})
    rc = _lib.load().smplfit_fit_recon_f32(h.ptr, C.byref(args), None, C.byref(rargs))
    torch.cuda.synchronize()
    return rc, fit


def test_outputs_overwritten_and_refusals(model_root, golden, dev):
    """Outputs pre-filled with NaN are fully overwritten; a refused call (a scale option, joint_error without target
    joints, no output at all) leaves them and the fit's outputs untouched and launches no stage kernel."""
    from smplfitter_amd import _lib

    m, om = _model('smpl', model_root, golden, dev)
    B, J, V = 3, m.num_joints, m.num_vertices
    tv, tj = targets('smpl', m, B, dev)
    nan = lambda *sh: torch.full(sh, float('nan'), dtype=torch.float32, device=dev)  # noqa: E731
    make = lambda: dict(vertices=nan(B, V, 3), joints=nan(B, J, 3), vertex_error=nan(B, V), joint_error=nan(B, J))  # noqa: E731
    outs = make()
    rc, fit = _c_fit_recon(m, dev, tv, tj, outs)
    assert rc == _lib.SMPLFIT_OK
    assert all(bool(torch.isfinite(v).all()) for v in list(outs.values()) + list(fit.values()))
    ref = fitter_of(m).fit(tv, tj, requested_keys=RECON, **FIT)
    for k in RECON:
        assert torch.equal(outs[k], ref[k]), k
    for kw, tjx, want in ((dict(scale_mode=1), tj, _lib.SMPLFIT_ERR_UNSUPPORTED), (dict(), None, _lib.SMPLFIT_ERR_BAD_ARG)):
        outs = make()
        before = _lib.stage_launches()
        rc, fit = _c_fit_recon(m, dev, tv, tjx, outs, **kw)
        assert rc == want, _lib.load().smplfit_last_error()
        assert _lib.stage_launches() == before
        assert all(bool(torch.isnan(v).all()) for v in list(outs.values()) + list(fit.values()))
    # the step on its own
    h = m._native(dev)
    ws = torch.empty(h.mesh_error_workspace_bytes(B), dtype=torch.uint8, device=dev)
    common = dict(glob_rotmats=ref['orientations'].data_ptr(), shape_betas=ref['shape_betas'].data_ptr(),
                  num_betas_given=m.num_betas, trans=ref['trans'].data_ptr(), batch=B, target_vertices=tv.data_ptr(),
                  workspace=ws.data_ptr(), workspace_bytes=ws.numel(), hip_stream=torch.cuda.current_stream(dev).cuda_stream)
    outs = make()
    args = _lib.MeshErrorArgs(**common, **{k: v.data_ptr() for k, v in outs.items()})  # joint_error, no target joints
    assert _lib.load().smplfit_mesh_error_f32(h.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_BAD_ARG
    assert _lib.load().smplfit_mesh_error_f32(h.ptr, C.byref(_lib.MeshErrorArgs(**common))) == _lib.SMPLFIT_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in outs.values())
    args = _lib.MeshErrorArgs(**common, target_joints=tj.data_ptr(), **{k: v.data_ptr() for k, v in outs.items()})
    assert _lib.load().smplfit_mesh_error_f32(h.ptr, C.byref(args)) == _lib.SMPLFIT_OK
    torch.cuda.synchronize()
    for k in RECON:
        assert torch.equal(outs[k], ref[k]), k


def test_poisoned_row(model_root, golden, dev):
    """A NaN in one target row: non-finite errors in that row and in no other; at clean parameters the step gives NaN at
    that one element and the bits of the clean call everywhere else."""
    m, om = _model('smpl', model_root, golden, dev)
    f = fitter_of(m)
    B, bad = 67, 5
    tv, tj = targets('smpl', m, B, dev)
    clean = f.fit(tv, tj, requested_keys=RECON, **FIT)
    tvp = tv.clone()
    tvp[bad, 17, 1] = float('nan')
    res = f.fit(tvp, tj, requested_keys=RECON, **FIT)
    keep = torch.arange(B, device=dev) != bad
    assert not bool(torch.isfinite(res['vertex_error'][bad, 17]))
    for k in RECON:
        assert bool(torch.isfinite(res[k][keep]).all()), k
    p = fit_params(clean)
    me = m.mesh_error(tvp, tj, **p)
    assert bool(torch.isnan(me['vertex_error'][bad, 17])) and int(torch.isnan(me['vertex_error']).sum()) == 1
    assert torch.equal(me['joint_error'], clean['joint_error'])


@pytest.mark.parametrize('which', ['known_pose', 'known_shape'])
def test_known_pose_and_shape(which, model_root, golden, dev):
    m, om = _model('smpl', model_root, golden, dev)
    f = fitter_of(m)
    B = 3
    tv, tj = targets('smpl', m, B, dev)
    base = f.fit(tv, tj, **FIT)
    if which == 'known_pose':
        res = f.fit_with_known_pose(base['pose_rotvecs'], tv, tj, requested_keys=RECON)
        plain = f.fit_with_known_pose(base['pose_rotvecs'], tv, tj)
        params = fit_params(res)
        with pytest.raises(NotImplementedError):
            f.fit_with_known_pose(base['pose_rotvecs'], tv, tj, scale_target=True, requested_keys=['vertex_error'])
    else:
        res = f.fit_with_known_shape(base['shape_betas'], tv, tj, num_iter=3, requested_keys=['pose_rotvecs'] + RECON)
        plain = f.fit_with_known_shape(base['shape_betas'], tv, tj, num_iter=3)
        params = dict(glob_rotmats=res['orientations'], shape_betas=base['shape_betas'], trans=res['trans'])
        with pytest.raises(NotImplementedError):
            f.fit_with_known_shape(base['shape_betas'], tv, tj, scale_fit=True, requested_keys=['vertex_error'])
    assert all(k in res for k in RECON) and not set(plain) & set(RECON)
    for k in plain:
        assert torch.equal(res[k], plain[k]), k
    check_fp64(om, res, params, tv, tj, B, which)


def test_gradients(model_root, golden, dev):
    """Targets that require grad: the differentiable route, the keys from BodyModel.forward and torch arithmetic."""
    m, om = _model('smpl', model_root, golden, dev)
    f = fitter_of(m)
    tv, tj = targets('smpl', m, 3, dev)
    tvg = tv.clone().requires_grad_()
    res = f.fit(tvg, tj, requested_keys=RECON, **FIT)
    assert all(res[k].grad_fn is not None for k in RECON)
    res['vertex_error'].sum().backward()
    assert bool(torch.isfinite(tvg.grad).all()) and float(tvg.grad.abs().max()) > 0
    detached = {k: v.detach() for k, v in res.items()}
    check_fp64(om, detached, fit_params(detached), tv, tj, 3, 'grad route')


def test_compile(model_root, golden, dev):
    """Under torch.compile(fullgraph=True) the keys come from the traced forward operator and torch arithmetic."""
    m, om = _model('smpl', model_root, golden, dev)
    f = fitter_of(m)
    tv, tj = targets('smpl', m, 3, dev)

    def pipeline(tv, tj):
        r = f.fit(tv, tj, requested_keys=RECON, **FIT)
        e = m.mesh_error(tv, tj, glob_rotmats=r['orientations'], shape_betas=r['shape_betas'], trans=r['trans'])
        return r, e

    res, e = torch.compile(pipeline, backend='aot_eager', fullgraph=True)(tv, tj)
    assert all(k in res for k in RECON)
    check_fp64(om, res, fit_params(res), tv, tj, 3, 'compile')
    check_fp64(om, e, fit_params(res), tv, tj, 3, 'compile mesh_error')


def test_empty_batch(model_root, golden, dev):
    m, om = _model('smpl', model_root, golden, dev)
    tv = torch.empty(0, m.num_vertices, 3, device=dev)
    tj = torch.empty(0, m.num_joints, 3, device=dev)
    res = fitter_of(m).fit(tv, tj, requested_keys=RECON, **FIT)
    assert res['vertex_error'].shape == (0, m.num_vertices) and res['joints'].shape == (0, m.num_joints, 3)
    me = m.mesh_error(tv, tj, pose_rotvecs=torch.empty(0, 3 * m.num_joints, device=dev), return_mesh=True)
    assert me['joint_error'].shape == (0, m.num_joints) and me['vertices'].shape == (0, m.num_vertices, 3)
