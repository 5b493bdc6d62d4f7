"""-m gpu: the differentiable ``BodyFitter.fit_with_known_shape`` (smplfit_fit_known_shape_backward_f32,
BodyFitter._fit_known_shape_backward and the autograd Function around the HIP call) against the fp64 arbiter of
tests/known_shape_grad_util.py (``TorchFit.fit_with_known_shape`` in fp64 on the CPU).

Gate of the comparisons with the arbiter, per gradient tensor (all six: shape_betas, kid_factor, the targets, the weights):
max |ours - fp64| <= max(GRAD_REL x max |fp64|, 2 x max |reference fp32 - fp64|).  The second term comes from
tests/golden/golden_known_shape_grad.npz for that case and tensor (SMPL A-G, SMPL-X-fat A and C); models and cases the
fixture does not hold take the SMPL entry of the case scaled to the tensor at hand: the reference's relative error on
SMPL times max |fp64| of the model under test, as tests/test_gpu_fit_grad.py does.

The kid case G runs on the models whose golden set has kid targets (smpl, smpl_w6).  The smpl1024 subset has no joint
regressor over its vertices: its cases without target joints (D, E) cannot be evaluated by the forward, the reference or
the arbiter, and check the refusal instead.  Measured figures: DESIGN.md section 18.
"""

import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import known_shape_grad_util as ku
from test_gpu_forward_grad import _rows
from test_gpu_parity import get_model
from test_known_pose_grad_host import GRAD_REL
from test_known_shape_grad_host import reference_errors

pytestmark = pytest.mark.gpu

# name -> the golden set its inputs come from
MODELS = dict(smpl='smpl', smplxfat='smplxfat', smpl1024='smpl1024', smpl_w6='smpl_w6')
KID_MODELS = ('smpl', 'smpl_w6')
_fitters, _ref_rel, _arb = {}, {}, {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gold():
    import os.path as osp

    return np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'golden_known_shape_grad.npz'))


def _fitter(name, model_root, golden, dev, **kw):
    from smplfitter_amd.pt import BodyFitter

    key = (name, tuple(kw.items()))
    if key not in _fitters:
        m, _ = get_model(model_root, name, golden(MODELS[name]), dev)
        _fitters[key] = BodyFitter(m, **kw)
    return _fitters[key]


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _backward(f, ts, kw, ct, want=None):
    return f._fit_known_shape_backward(ts['shape_betas'], ts.get('kid_factor'), ts['target_vertices'], ts.get('target_joints'),
                                       ts.get('vertex_weights'), ts.get('joint_weights'), kw['num_iter'], kw['final_adjust_rots'],
                                       **ct, want=f.KNOWN_SHAPE_GRAD_NAMES if want is None else want)


def _native(f, x, kw, cot, dev, want=None):
    """The no-gradient HIP call, then the native backward call."""
    ts = {k: _t(v, dev) for k, v in x.items()}
    with torch.no_grad():
        r = f.fit_with_known_shape(**ts, **kw)
    g = _backward(f, ts, kw, {'grad_' + k: _t(v, dev) for k, v in cot.items()}, want)
    torch.cuda.synchronize()
    return r, {k: v.cpu().numpy() for k, v in g.items()}


def _arbiter(name, case, B, seed, cot_seed, model_root, golden, rows=None):
    """The arbiter's results and gradients of a case (computed once per key and left unchanged)."""
    key = (name, case, B, seed, cot_seed)
    if key not in _arb:
        g = golden(MODELS[name])
        x, kw = ku.case_inputs(g, case, B, seed=seed)
        cot = ku.cotangents(cot_seed, B, g['target_joints'].shape[1])
        tf = ku.torchfit64(model_root, MODELS[name], g, False)
        sel = (lambda d: d) if rows is None else (lambda d: {k: v[rows] for k, v in d.items()})
        _arb[key] = (x, kw, cot) + ku.arbiter(tf, sel(x), kw, sel(cot))
    return _arb[key]


def _reference_rel(gold, case, model_root, golden):
    """The reference's relative fp32 error per tensor on the SMPL fixture entry of a case (computed once)."""
    if case not in _ref_rel:
        g = golden('smpl')
        _, _, _, _, grads = _arbiter('smpl', case, 2, 0, int(gold[f'smpl.{case}.seed']), model_root, golden)
        err = reference_errors(gold, 'smpl', case, grads, g['target_vertices'].shape[1])
        _ref_rel[case] = {k: err[k] / max(np.abs(v).max(), 1e-30) for k, v in grads.items()}
    return _ref_rel[case]


def _gate(ours, grads, ref_err, tag, rows=None):
    worst = {}
    assert set(ours) == set(grads), (tag, set(ours), set(grads))
    for k, r in grads.items():
        o = ours[k] if rows is None else ours[k][rows]
        assert np.all(np.isfinite(o)), (tag, k)
        err, gate = np.abs(o - r).max(), max(GRAD_REL * np.abs(r).max(), 2 * ref_err[k])
        worst[k] = (err, gate)
        print(f'[known-shape-grad] {tag} {k} ours-vs-fp64 {err:.2e} ref-vs-fp64 {ref_err[k]:.2e} max {np.abs(r).max():.2e} '
              f'rel {err / max(np.abs(r).max(), 1e-300):.2e} gate {gate:.2e}')
    for k, (err, gate) in worst.items():
        assert err <= gate, (tag, k, err, gate)


@pytest.mark.parametrize('name,case', [(n, c) for n in MODELS for c in ku.CASES if c != 'G' or n in KID_MODELS])
def test_native_vs_arbiter(name, case, model_root, golden, gold, dev):
    f = _fitter(name, model_root, golden, dev)
    if name == 'smpl1024' and not ku.CASES[case]['joints']:
        # the vertex-subset model has no joint regressor over its vertices: without target joints the fit itself is
        # refused (tests/test_gpu_parity.py), by the reference too; the backward refuses the same way, before any launch
        x, kw = ku.case_inputs(golden(MODELS[name]), case, 2)
        ts = {k: _t(v, dev) for k, v in x.items()}
        with pytest.raises(ValueError, match='J_regressor_post_lbs'):
            _backward(f, ts, kw, dict(grad_trans=torch.ones(2, 3, device=dev)))
        return
    in_fixture = case in ku.FIXTURE_CASES.get(name, '')
    seed = int(gold[f'{name}.{case}.seed']) if in_fixture else 7
    x, kw, cot, out, grads = _arbiter(name, case, 2, 0, seed, model_root, golden)
    r, ours = _native(f, x, kw, cot, dev)
    for k in cot:  # the fit the adjoint is evaluated at: the fp32 HIP fit against the fp64 restatement (tests/util.py pose_tol)
        e = np.abs(r[k].cpu().numpy().reshape(out[k].shape) - out[k]).max()
        print(f'[known-shape-grad] {name} {case} forward {k} ours-vs-fp64 {e:.2e}')
        assert e <= 3e-3, (name, case, k)
    if in_fixture:
        ref_err = reference_errors(gold, name, case, grads, x['target_vertices'].shape[1])
    else:
        rel = _reference_rel(gold, case, model_root, golden)
        ref_err = {k: rel[k] * np.abs(v).max() for k, v in grads.items()}
    _gate(ours, grads, ref_err, f'{name} {case}')


@pytest.mark.parametrize('B', [1, 64, 65, 257])
def test_batch_edges(B, model_root, golden, gold, dev):
    rows = _rows(B)
    x, kw, cot, _, grads = _arbiter('smpl', 'C', B, B, B, model_root, golden, rows=rows)
    _, ours = _native(_fitter('smpl', model_root, golden, dev), x, kw, cot, dev)
    rel = _reference_rel(gold, 'C', model_root, golden)
    _gate(ours, grads, {k: rel[k] * np.abs(v).max() for k, v in grads.items()}, f'smpl C B={B}', rows)


@pytest.mark.parametrize('only', ['shape_betas', 'target_vertices'])
def test_autograd_end_to_end(only, model_root, golden, dev):
    """One input requires grad: the results are the no-gradient call's bits, its gradient the native call's, the others
    get none, no warning is raised; no ``grad_fn`` without gradients.  (Before the feature: ``NotImplementedError``.)"""
    x, kw, cot, _, _ = _arbiter('smpl', 'C', 2, 0, 3, model_root, golden)
    f = _fitter('smpl', model_root, golden, dev)
    r0, native = _native(f, x, kw, cot, dev, want=(only,))
    assert set(native) == {only}
    ts = {k: _t(v, dev) for k, v in x.items()}
    ts[only].requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        r = f.fit_with_known_shape(**ts, **kw, requested_keys=['pose_rotvecs', 'relative_orientations'])
    assert set(r) == {'pose_rotvecs', 'trans', 'orientations', 'relative_orientations'}
    for k in ('pose_rotvecs', 'trans', 'orientations'):
        assert torch.equal(r[k], r0[k]), k
        assert r[k].grad_fn is not None, k
    sum((r[k].reshape(c.shape) * _t(c, dev)).sum() for k, c in cot.items()).backward()
    for k, t in ts.items():
        if k != only:
            assert t.grad is None, k
    assert ts[only].grad.shape == ts[only].shape
    assert np.array_equal(ts[only].grad.cpu().numpy(), native[only])
    with torch.no_grad():
        assert f.fit_with_known_shape(**ts, **kw)['trans'].grad_fn is None
    assert f.fit_with_known_shape(**{k: v.detach() for k, v in ts.items()}, **kw)['trans'].grad_fn is None


def test_autograd_shapes_of_betas_and_kid(model_root, golden, dev):
    """``shape_betas`` wider than the model gets its own shape back with zero columns beyond the model's betas; a
    broadcast scalar ``kid_factor`` gets the sum over the batch; ``orientations`` alone carries a gradient."""
    x, kw, cot, _, _ = _arbiter('smpl', 'G', 2, 0, 3, model_root, golden)
    f = _fitter('smpl', model_root, golden, dev)
    ts = {k: _t(v, dev) for k, v in x.items()}
    x1 = dict(x, kid_factor=np.full(2, x['kid_factor'][0], np.float32))
    _, native = _native(f, x1, kw, dict(trans=cot['trans']), dev)
    wide = torch.cat([ts['shape_betas'], torch.ones(2, 3, device=dev)], 1).requires_grad_()
    kid = ts['kid_factor'][:1].clone().requires_grad_()
    rest = {k: v for k, v in ts.items() if k not in ('shape_betas', 'kid_factor')}
    r = f.fit_with_known_shape(shape_betas=wide, kid_factor=kid, **rest, **kw)
    (r['trans'] * _t(cot['trans'], dev)).sum().backward()
    assert wide.grad.shape == wide.shape and not wide.grad[:, 10:].any()
    assert np.array_equal(wide.grad[:, :10].cpu().numpy(), native['shape_betas'])
    assert kid.grad.shape == kid.shape
    np.testing.assert_allclose(kid.grad.item(), native['kid_factor'].sum(), rtol=1e-6)
    tv = ts['target_vertices'].clone().requires_grad_()
    f.fit_with_known_shape(**dict(ts, target_vertices=tv), **kw)['orientations'].square().sum().backward()
    assert torch.isfinite(tv.grad).all() and tv.grad.abs().max().item() > 0


@pytest.mark.parametrize('name', ['smpl', 'smplxfat'])
def test_directional_derivative(name, model_root, golden, dev):
    """The autograd directional derivative of case C along one direction over (target_vertices, target_joints,
    shape_betas) jointly against central differences of the no-gradient HIP call at eps 1e-2, within the 5 % of the
    reference's own gradient test."""
    x, kw, cot, _, _ = _arbiter(name, 'C', 2, 0, 5, model_root, golden)
    f = _fitter(name, model_root, golden, dev)
    cot = {k: _t(v, dev) for k, v in cot.items()}
    names = ('target_vertices', 'target_joints', 'shape_betas')
    fixed = {k: _t(v, dev) for k, v in x.items() if k not in names}
    base = {k: _t(x[k], dev) for k in names}
    loss = lambda r: sum((r[k].reshape(c.shape) * c).sum() for k, c in cot.items())  # noqa: E731
    var = {k: v.clone().requires_grad_() for k, v in base.items()}
    loss(f.fit_with_known_shape(**var, **fixed, **kw)).backward()
    gen = torch.Generator().manual_seed(7)
    d = {k: torch.randn(v.shape, generator=gen).to(dev) for k, v in base.items()}
    d = {k: v / v.norm() for k, v in d.items()}
    ag = sum((var[k].grad * d[k]).sum().item() for k in names)
    eps = 1e-2
    with torch.no_grad():
        lp = loss(f.fit_with_known_shape(**{k: base[k] + eps * d[k] for k in names}, **fixed, **kw)).item()
        lm = loss(f.fit_with_known_shape(**{k: base[k] - eps * d[k] for k in names}, **fixed, **kw)).item()
    fd = (lp - lm) / (2 * eps)
    print(f'[known-shape-grad] direction {name} autograd {ag:.5e} finite differences {fd:.5e}')
    assert abs(ag - fd) / max(abs(ag), abs(fd), 1e-3) < 5e-2, (ag, fd)


def test_output_subsets_and_determinism(model_root, golden, dev):
    """Each output alone gives the bits of the all-outputs call; two runs give identical bits."""
    x, kw, cot, _, _ = _arbiter('smpl', 'G', 2, 0, 11, model_root, golden)
    f = _fitter('smpl', model_root, golden, dev)
    _, full = _native(f, x, kw, cot, dev)
    _, again = _native(f, x, kw, cot, dev)
    assert set(full) == set(f.KNOWN_SHAPE_GRAD_NAMES)
    for k in full:
        assert np.array_equal(full[k], again[k]), k
    for k in f.KNOWN_SHAPE_GRAD_NAMES:
        _, one = _native(f, x, kw, cot, dev, want=(k,))
        assert set(one) == {k}
        assert np.array_equal(one[k], full[k]), k


@pytest.mark.parametrize('name,case,B', [('smpl', 'G', 65), ('smplxfat', 'C', 5)])
def test_backward_guards(name, case, B, model_root, golden, dev):
    """smplfit_fit_known_shape_backward_f32 called directly (every input, every cotangent, every output; two resp. three
    iterations and the refinement, so that every region of its workspace is used; B = 65: a second, partial block of the
    lane-per-instance kernels; smplxfat: more than 32 joints).  Every output and a workspace of exactly the queried size
    lie between two 1 MB guard regions, the outputs pre-filled with NaN, the workspace once zeroed and once filled with
    a NaN pattern: every guard byte survives, every output element is written and finite, the two fills give the same
    bits.  A workspace one byte short is refused before anything is enqueued."""
    from smplfitter_amd import _lib
    from test_gpu_flipper import _guarded, _intact

    g = golden(MODELS[name])
    x, kw = ku.case_inputs(g, case, B, seed=B)
    f = _fitter(name, model_root, golden, dev)
    m = f.body_model
    J, V = m.num_joints, m.num_vertices
    ts = {k: _t(v, dev) for k, v in x.items()}
    rs = np.random.RandomState(B)
    cot = {'grad_' + k: _t(v, dev) for k, v in ku.cotangents(B, B, J).items()}
    cot['grad_orientations'] = _t(rs.randn(B, J, 3, 3).astype(np.float32), dev)
    cot['grad_relative_orientations'] = _t(rs.randn(B, J, 3, 3).astype(np.float32), dev)
    kid = 'kid_factor' in x
    h = m._native(dev, kid=kid)
    nws = h.fit_known_shape_backward_workspace_bytes(B, kw['num_iter'])
    assert nws > h.forward_backward_workspace_bytes(B)
    sizes = dict(target_vertices=B * V * 3, target_joints=B * J * 3, vertex_weights=B * V, joint_weights=B * J, shape_betas=B * 10)
    if kid:
        sizes['kid_factor'] = B
    lib = _lib.load()
    mk = lambda outs, ws, n: _lib.FitKnownShapeBackwardArgs(  # noqa: E731
        **{k: v.data_ptr() for k, v in ts.items()}, num_betas_given=10, batch=B, num_iter=kw['num_iter'],
        final_adjust_rots=int(kw['final_adjust_rots']), **{k: v.data_ptr() for k, v in cot.items()},
        **{f'grad_{k}': o.data_ptr() for k, o in outs.items()}, workspace=ws.data_ptr(), workspace_bytes=n,
        hip_stream=torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for fill in ('zero', 'nan'):
        bufs = {k: _guarded(4 * n, dev) for k, n in sizes.items()}
        for _, o in bufs.values():
            o.view(torch.float32).fill_(float('nan'))
        wbuf, ws = _guarded(nws, dev)
        assert ws.data_ptr() % 256 == 0
        if fill == 'zero':
            ws.zero_()
        else:
            ws.view(torch.int32)[: nws // 4].fill_(0x7FC00000 | 0x1234)
        _lib.check(lib.smplfit_fit_known_shape_backward_f32(h.ptr, C.byref(mk({k: o for k, (_, o) in bufs.items()}, ws, nws))))
        torch.cuda.synchronize()
        assert _intact(wbuf, nws), 'workspace guard written'
        for k, (buf, o) in bufs.items():
            assert _intact(buf, o.numel()), f'guard region of output {k} written'
            assert bool(torch.isfinite(o.view(torch.float32)).all()), f'output {k}: an element was not written'
        out[fill] = {k: o.clone() for k, (_, o) in bufs.items()}
        del bufs, wbuf, ws
    for k in out['zero']:
        assert torch.equal(out['zero'][k], out['nan'][k]), k
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    outs = {k: torch.full((n,), float('nan'), device=dev) for k, n in sizes.items()}
    assert lib.smplfit_fit_known_shape_backward_f32(h.ptr, C.byref(mk(outs, ws, nws - 1))) == _lib.SMPLFIT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs.values())  # nothing was enqueued


def test_refusals(model_root, golden, dev):
    """``scale_fit`` and ``initial_pose_rotvecs`` (given, or requiring grad) with gradients raise ``NotImplementedError``."""
    x, kw, _, _, _ = _arbiter('smpl', 'C', 2, 0, 3, model_root, golden)
    f = _fitter('smpl', model_root, golden, dev)
    ts = {k: _t(v, dev) for k, v in x.items()}
    betas = ts.pop('shape_betas').requires_grad_()
    J = ts['target_joints'].shape[1]
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    for bad in (dict(scale_fit=True), dict(initial_pose_rotvecs=z(2, J * 3))):
        with pytest.raises(NotImplementedError):
            f.fit_with_known_shape(shape_betas=betas, **ts, **kw, **bad)
    with pytest.raises(NotImplementedError):
        f.fit_with_known_shape(shape_betas=betas.detach(), **ts, **kw, initial_pose_rotvecs=z(2, J * 3).requires_grad_())


def test_native_backward_false(model_root, golden, gold, dev):
    """``BodyFitter(..., native_backward=False)`` takes the ``TorchFit`` route with its warning and stays within the gate."""
    x, kw, cot, _, grads = _arbiter('smpl', 'C', 2, 0, int(gold['smpl.C.seed']), model_root, golden)
    f = _fitter('smpl', model_root, golden, dev, native_backward=False)
    ts = {k: _t(v, dev).requires_grad_() for k, v in x.items()}
    with pytest.warns(RuntimeWarning, match='PyTorch'):
        r = f.fit_with_known_shape(**ts, **kw)
    sum((r[k].reshape(c.shape) * _t(c, dev)).sum() for k, c in cot.items()).backward()
    ours = {k: t.grad.cpu().numpy() for k, t in ts.items()}
    _gate(ours, grads, reference_errors(gold, 'smpl', 'C', grads, x['target_vertices'].shape[1]), 'smpl C TorchFit route')


def test_poisoned_row(model_root, golden, dev):
    """A NaN in one row leaves every other row's gradients unchanged."""
    g = golden('smpl')
    x, kw = ku.case_inputs(g, 'C', 3)
    f = _fitter('smpl', model_root, golden, dev)
    cot = ku.cotangents(13, 3, g['target_joints'].shape[1])
    _, clean = _native(f, x, kw, cot, dev)
    xp = {k: v.copy() for k, v in x.items()}
    xp['target_vertices'][1, 17, 2] = np.nan
    _, bad = _native(f, xp, kw, cot, dev)
    for k in clean:
        assert np.all(np.isfinite(clean[k])), k
        assert np.array_equal(clean[k][[0, 2]], bad[k][[0, 2]]), k
    assert not np.all(np.isfinite(bad['target_vertices'][1]))
