"""-m gpu: BodyFlipper on the HIP kernels.  The fused flip (smplfit_flip_f32: forward with kid_factor, mirror transfer
with x negated into the fit's target stream, naive flip of the pose, warm-started fit) and the unfused one
(SMPLFIT_BM=0: BodyModel.forward + flip_vertices + BodyFitter.fit) against the reference's fixture
(tests/golden/make_golden_flip.py), against each other at scale, the general-path fallback against the fp64 oracle,
guard regions around every output and the workspace, and run-to-run determinism.

Gates (util.check_convert's): max vertex L2 of the fp64 forwards of ours and the reference's parameters <= 1e-4 m,
trans <= 2e-5.  The fixture records its own fp32-vs-fp64 distance (<= 1.8e-5 m), well inside the gate."""

import ctypes as C

import numpy as np
import pytest
import torch

import flip_util
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gf(golden):
    return golden('flip')


_models = {}


def get_model(model_root, tag, dev):
    from smplfitter_amd.pt import BodyModel

    if tag not in _models:
        kind = 'smplx' if tag == 'smplx' else 'smpl'
        gname = flip_util.FLIP_MODELS[tag]
        m = BodyModel(kind, 'neutral', model_root=f'{model_root}/{util.model_dir(gname)}', num_betas=10, device=dev)
        _, md = util.load_md(model_root, gname)
        _models[tag] = (m, util.O.OracleModel(md, np.float64, kind))
    return _models[tag]


def t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def to_np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def flipper(m, path, dev, smplfit_env):
    """A BodyFlipper whose flips take `path`, asserted through its plan."""
    from smplfitter_amd.pt import BodyFlipper

    smplfit_env('SMPLFIT_BM', '1' if path == 'fused' else '0')
    fl = BodyFlipper(m)
    assert (fl._plan(dev) is not None) == (path == 'fused'), path
    return fl


def inputs(J, B, seed, kid=False):
    rs = np.random.RandomState(seed)
    pose = (rs.randn(B, 3 * J) * 0.1).astype(np.float32)
    betas = rs.randn(B, 10).astype(np.float32)
    trans = rs.randn(B, 3).astype(np.float32)
    k = (rs.randn(B) * 0.3).astype(np.float32) if kid else None
    return pose, betas, trans, k


def rows_of(B, n=32):
    n = min(B, n)
    return np.unique(np.r_[0:(n + 1) // 2, B - n // 2:B])  # both ends of the batch (every chunk, the partial last block)


@pytest.mark.parametrize('path', ['fused', 'unfused'])
@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_flip_goldens(tag, path, model_root, gf, dev, data_root_fat, monkeypatch, smplfit_env):
    """naive_flip_rotvecs bit-exact, flip_vertices within 3e-6 m, and flip (num_iter 1 / 3, with kid_factor) within the
    mesh gate of the reference's results, with the reference's result keys."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, om64 = get_model(model_root, tag, dev)
    fl = flipper(m, path, dev, smplfit_env)
    assert util.csr_digest(flip_util.canonical_csr(fl.mirror_csr)) == str(gf[f'{tag}.csr_sha256'])
    pose, betas, trans, kid = (t(gf[f'{tag}.{k}'], dev) for k in ('pose', 'betas', 'trans', 'kid'))
    assert torch.equal(fl.naive_flip_rotvecs(pose).cpu(), torch.from_numpy(gf[f'{tag}.naive']))
    v = fl.flip_vertices(m(pose, betas, trans)['vertices'])
    assert v.shape == (8, m.num_vertices, 3)
    assert np.abs(v.cpu().numpy()[:, ::97] - gf[f'{tag}.vertices_sub']).max() < 3e-6
    for case in flip_util.FLIP_CASES:
        ni, with_kid = flip_util.case_args(case)
        o = to_np(fl.flip(pose, betas, trans, kid_factor=kid if with_kid else None, num_iter=ni))
        flip_util.check_flip(om64, tag, case, o, gf)
        if not with_kid:
            assert np.abs(o['kid_factor']).max() < 1e-4


def _fused_vs_unfused(m, om64, B, dev, smplfit_env, seed, kid=False, num_iter=1):
    pose, betas, trans, k = (t(a, dev) for a in inputs(m.num_joints, B, seed, kid))
    res = {}
    for path in ('fused', 'unfused'):
        fl = flipper(m, path, dev, smplfit_env)
        res[path] = to_np(fl.flip(pose, betas, trans, kid_factor=k, num_iter=num_iter))
    for r in res.values():
        assert set(r) == set(flip_util.FLIP_KEYS)
        assert all(np.isfinite(x).all() for x in r.values())
    idx = rows_of(B)
    a = {key: x[idx] for key, x in res['fused'].items()}
    b = {key: x[idx] for key, x in res['unfused'].items()}
    assert flip_util.mesh_distance(om64, a, b) <= 1e-4
    assert np.abs(res['fused']['trans'] - res['unfused']['trans']).max() <= 2e-5
    return res


@pytest.mark.parametrize('tag,B,kid,num_iter', [('smpl', 1, False, 1), ('smpl', 130, True, 1), ('smplx', 130, False, 3),
                                                 ('smpl', 4096, False, 1), ('smplx', 4096, True, 1)])
def test_flip_fused_matches_unfused(tag, B, kid, num_iter, model_root, dev, data_root_fat, monkeypatch, smplfit_env):
    """The fused flip against forward + flip_vertices + fit (same algorithm, different kernels and summation orders) on
    a single instance, a ragged batch and B = 4096 (SMPL-X: two chunks)."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, om64 = get_model(model_root, tag, dev)
    _fused_vs_unfused(m, om64, B, dev, smplfit_env, seed=B + num_iter, kid=kid, num_iter=num_iter)


@pytest.mark.usefixtures('two_chunks')
def test_flip_fused_two_chunks(model_root, dev, data_root_fat, monkeypatch, smplfit_env):
    """B = 1100 as two concurrent chunks (the second partial) on the SMPL-shaped model, with and without kid_factor."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, om64 = get_model(model_root, 'smpl', dev)
    _fused_vs_unfused(m, om64, 1100, dev, smplfit_env, seed=11)
    _fused_vs_unfused(m, om64, 1100, dev, smplfit_env, seed=12, kid=True, num_iter=2)


def test_flip_options_reloaded(model_root, dev, data_root_fat, monkeypatch, smplfit_env):
    """A plan made while the batch-major kernels applied, then SMPLFIT_BM=0: smplfit_flip_f32 reports unsupported and
    that call takes the unfused path, with the same result as a flipper made under SMPLFIT_BM=0."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, _ = get_model(model_root, 'smpl', dev)
    fl = flipper(m, 'fused', dev, smplfit_env)
    pose, betas, trans, _ = (t(a, dev) for a in inputs(m.num_joints, 64, 5))
    fused = to_np(fl.flip(pose, betas, trans))
    smplfit_env('SMPLFIT_BM', '0')
    late = to_np(fl.flip(pose, betas, trans))
    ref = to_np(flipper(m, 'unfused', dev, smplfit_env).flip(pose, betas, trans))
    for k in flip_util.FLIP_KEYS:
        assert np.array_equal(late[k], ref[k]), k
    assert np.abs(fused['trans'] - late['trans']).max() <= 2e-5


def test_flip_general_path(model_root, dev, data_root_fat, monkeypatch, smplfit_env):
    """A model outside the batch-major kernels (32 betas: the general path) has no plan; its flip (forward +
    flip_vertices + fit) matches the fp64 oracle flip."""
    from smplfitter_amd import modelio
    from smplfitter_amd.pt import BodyFlipper, BodyModel

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    smplfit_env('SMPLFIT_BM', None)
    m = BodyModel('smpl', 'neutral', model_root=f'{model_root}/smpl_b32', num_betas=32, device=dev)
    assert m.kernel_path(enable_kid=True) == 'general'
    fl = BodyFlipper(m)
    assert fl._plan(dev) is None
    md = modelio.load_model('smpl', 'neutral', model_root=f'{model_root}/smpl_b32', num_betas=32)
    om64 = util.O.OracleModel(md, np.float64, 'smpl')
    rs = np.random.RandomState(8)
    B = 8
    pose = (rs.randn(B, 3 * m.num_joints) * 0.1).astype(np.float32)
    betas = (rs.randn(B, 32) * 0.5).astype(np.float32)
    trans = rs.randn(B, 3).astype(np.float32)
    for kid in (None, (rs.randn(B) * 0.3).astype(np.float32)):
        o = to_np(fl.flip(t(pose, dev), t(betas, dev), t(trans, dev), kid_factor=t(kid, dev), num_iter=2))
        ref = flip_util.oracle_flip(om64, fl.mirror_csr, fl.mirror_inds_joints.cpu().numpy(), pose, betas, trans, kid, 2)
        assert flip_util.mesh_distance(om64, o, ref) <= 1e-4
        assert np.abs(o['trans'] - ref['trans']).max() <= 2e-5


GUARD = 1 << 20


def _guarded(nbytes, dev):
    buf = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=dev)
    buf.fill_(0xA5)
    return buf, buf[GUARD:GUARD + nbytes]


def _intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


@pytest.mark.parametrize('tag,B', [('smpl', 130), ('smplx', 1100)])
def test_flip_guards(tag, B, model_root, dev, data_root_fat, monkeypatch, smplfit_env):
    """smplfit_flip_f32 called directly with every output and the workspace between two 1 MB guard regions, outputs
    pre-filled with NaN, the workspace once zeroed and once filled with a NaN pattern: every guard byte survives, every
    output element is written and finite, the two fills give the same bits (no read of a cell nobody wrote, and two runs
    are identical), and kid_factor stays near 0 when none is given (kid ridge 1e9)."""
    from smplfitter_amd import _lib

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, _ = get_model(model_root, tag, dev)
    fl = flipper(m, 'fused', dev, smplfit_env)
    plan = fl._plan(dev)
    J, S = m.num_joints, fl.fitter.n_betas
    pose, betas, trans, _ = (t(a, dev) for a in inputs(J, B, 17))
    sizes = dict(pose=B * J * 3, betas=B * S, trans=B * 3, kid=B, orient=B * J * 9, rel=B * J * 9)
    out = {}
    for fill in ('zero', 'nan'):
        bufs = {k: _guarded(4 * n, dev) for k, n in sizes.items()}
        for _, o in bufs.values():
            o.view(torch.float32).fill_(float('nan'))
        nws = plan.workspace_bytes(B)
        wbuf, ws = _guarded(nws, dev)
        assert ws.data_ptr() % 256 == 0
        if fill == 'zero':
            ws.zero_()
        else:
            ws.view(torch.int32)[: nws // 4].fill_(0x7FC00000 | 0x1234)
        p = lambda k: bufs[k][1].data_ptr()  # noqa: E731
        args = _lib.FlipArgs(
            pose_rotvecs=pose.data_ptr(), shape_betas=betas.data_ptr(), num_betas_given=10, trans=trans.data_ptr(),
            kid_factor=None, batch=B, num_iter=2, beta_regularizer=1e-2, beta_regularizer2=1e-2, kid_regularizer=1e9,
            final_adjust_rots=1, out_pose_rotvecs=p('pose'), out_shape_betas=p('betas'), out_trans=p('trans'),
            out_kid_factor=p('kid'), out_orientations=p('orient'), out_relative_orientations=p('rel'),
            workspace=ws.data_ptr(), workspace_bytes=nws, hip_stream=torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().smplfit_flip_f32(plan.ptr, C.byref(args)))
        torch.cuda.synchronize()
        assert _intact(wbuf, nws), 'workspace guard written'
        for k, (buf, o) in bufs.items():
            assert _intact(buf, o.numel()), f'guard region of output {k} written'
            assert bool(torch.isfinite(o.view(torch.float32)).all()), f'output {k}: an element was not written'
        assert float(bufs['kid'][1].view(torch.float32).abs().max()) < 1e-4
        out[fill] = {k: o.clone() for k, (_, o) in bufs.items()}
        del bufs, wbuf, ws
    for k in out['zero']:
        assert torch.equal(out['zero'][k], out['nan'][k]), k
    # a workspace one byte short is refused before anything is enqueued
    ws = torch.empty(plan.workspace_bytes(B), dtype=torch.uint8, device=dev)
    args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel() - 1
    assert _lib.load().smplfit_flip_f32(plan.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_WORKSPACE


@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_flip_deterministic(tag, model_root, dev, data_root_fat, monkeypatch, smplfit_env):
    """Two fused flips of the same batch give the same bits."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, _ = get_model(model_root, tag, dev)
    fl = flipper(m, 'fused', dev, smplfit_env)
    pose, betas, trans, kid = (t(a, dev) for a in inputs(m.num_joints, 2000, 23, kid=True))
    a = fl.flip(pose, betas, trans, kid_factor=kid, num_iter=2)
    b = fl.flip(pose, betas, trans, kid_factor=kid, num_iter=2)
    for k in flip_util.FLIP_KEYS:
        assert torch.equal(a[k], b[k]), k


def test_flip_grad_inputs_raise(model_root, dev, data_root_fat, monkeypatch):
    from smplfitter_amd.pt import BodyFlipper

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, _ = get_model(model_root, 'smpl', dev)
    fl = BodyFlipper(m)
    pose, betas, trans, _ = (t(a, dev) for a in inputs(m.num_joints, 4, 1))
    with pytest.raises(NotImplementedError):
        fl.flip(pose.requires_grad_(), betas, trans)
    with pytest.raises(NotImplementedError):
        fl.flip_vertices(torch.zeros(2, m.num_vertices, 3, device=dev, requires_grad=True))
    empty = fl.flip(pose[:0].detach(), betas[:0], trans[:0])
    assert set(empty) == set(flip_util.FLIP_KEYS) and empty['pose_rotvecs'].shape == (0, 3 * m.num_joints)
