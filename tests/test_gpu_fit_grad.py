"""-m gpu: the differentiable ``BodyFitter.fit`` (smplfit_fit_backward_f32, BodyFitter._fit_backward and the autograd
Function around the HIP fit) against the fp64 arbiter of tests/fit_grad_util.py (``TorchFit`` in fp64 on the CPU).

Gate of the comparisons with the arbiter, per gradient tensor:
max |ours - fp64| <= max(GRAD_REL x max |fp64|, 2 x max |reference fp32 - fp64|).  The second term comes from
tests/golden/golden_fit_grad.npz for that case and tensor (SMPL A-G, SMPL-X-fat A and C); models and cases the fixture
does not hold take the SMPL entry of the case scaled to the tensor at hand: the reference's relative error on SMPL times
max |fp64| of the model under test, as tests/test_gpu_known_pose_grad.py does.

Measured on an MI355X (relative to max |fp64| of the tensor, worst over the four models and seven cases):
target_vertices 5.7e-6, target_joints 2.0e-6, vertex_weights 2.7e-5, joint_weights 1.9e-5; the tensor nearest its gate
is vertex_weights of smplxfat C at 0.14 of it.  Direction check: -3.39128 against -3.38804 (smpl), -20.2724 against
-20.2389 (smplxfat).  The smpl1024 subset has no joint regressor over its vertices: its cases without target joints
(D, E) cannot be evaluated by the forward, the reference or the arbiter, and check the refusal instead.
"""

import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import fit_grad_util as fu
from test_fit_grad_host import reference_errors
from test_gpu_forward_grad import _rows
from test_gpu_parity import get_model
from test_known_pose_grad_host import GRAD_REL

pytestmark = pytest.mark.gpu

# name -> the golden set its inputs come from
MODELS = dict(smpl='smpl', smplxfat='smplxfat', smpl1024='smpl1024', smpl_w6='smpl_w6')
_fitters, _ref_rel, _arb = {}, {}, {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gold():
    import os.path as osp

    return np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'golden_fit_grad.npz'))


def _fitter(name, kid, model_root, golden, dev):
    from smplfitter_amd.pt import BodyFitter

    if (name, kid) not in _fitters:
        m, _ = get_model(model_root, name, golden(MODELS[name]), dev)
        _fitters[name, kid] = BodyFitter(m, enable_kid=kid)
    return _fitters[name, kid]


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _native(f, x, kw, cot, dev, want=None):
    """The no-gradient HIP fit, then the native backward call."""
    ts = {k: _t(v, dev) for k, v in x.items()}
    with torch.no_grad():
        r = f.fit(**ts, **kw)
    ct = {'grad_' + k: _t(v, dev) for k, v in cot.items()}
    kid_reg = kw.get('kid_regularizer', kw['beta_regularizer'])
    g = f._fit_backward(ts['target_vertices'], ts.get('target_joints'), ts.get('vertex_weights'), ts.get('joint_weights'),
                        kw['num_iter'], kw['beta_regularizer'], kw['beta_regularizer2'], kid_reg, kw['final_adjust_rots'],
                        **ct, want=f.FIT_GRAD_NAMES if want is None else want)
    torch.cuda.synchronize()
    return r, {k: v.cpu().numpy() for k, v in g.items()}


def _arbiter(name, case, B, seed, cot_seed, model_root, golden, rows=None):
    """The arbiter's results and gradients of a case (computed once per key and left unchanged)."""
    key = (name, case, B, seed, cot_seed)
    if key not in _arb:
        g = golden(MODELS[name])
        x, kw, kid = fu.case_inputs(g, case, B, seed=seed)
        J = g['target_joints'].shape[1]
        cot = fu.cotangents(cot_seed, B, J, 10, kid)
        tf = fu.torchfit64(model_root, MODELS[name], g, kid)
        sel = (lambda d: d) if rows is None else (lambda d: {k: v[rows] for k, v in d.items()})
        _arb[key] = (x, kw, kid, cot) + fu.arbiter(tf, sel(x), kw, sel(cot))
    return _arb[key]


def _reference_rel(gold, case, model_root, golden):
    """The reference's relative fp32 error per tensor on the SMPL fixture entry of a case (computed once)."""
    if case not in _ref_rel:
        g = golden('smpl')
        _, _, _, _, _, grads = _arbiter('smpl', case, 2, 0, int(gold[f'smpl.{case}.seed']), model_root, golden)
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
        print(f'[fit-grad] {tag} {k} ours-vs-fp64 {err:.2e} ref-vs-fp64 {ref_err[k]:.2e} max {np.abs(r).max():.2e} '
              f'rel {err / np.abs(r).max():.2e} gate {gate:.2e}')
    for k, (err, gate) in worst.items():
        assert err <= gate, (tag, k, err, gate)


@pytest.mark.parametrize('name,case', [(n, c) for n in MODELS for c in fu.CASES if c != 'G' or n == 'smpl'])
def test_native_vs_arbiter(name, case, model_root, golden, gold, dev):
    if name == 'smpl1024' and not fu.CASES[case]['joints']:
        # the vertex-subset model has no joint regressor over its vertices: without target joints the fit itself is
        # refused (tests/test_gpu_parity.py), by the reference too; the backward refuses the same way, before any launch
        f = _fitter(name, False, model_root, golden, dev)
        x, kw, _ = fu.case_inputs(golden(MODELS[name]), case, 2)
        tv = _t(x['target_vertices'], dev)
        with pytest.raises(ValueError, match='J_regressor_post_lbs'):
            f._fit_backward(tv, None, _t(x.get('vertex_weights'), dev), None, kw['num_iter'], kw['beta_regularizer'],
                            kw['beta_regularizer2'], kw['beta_regularizer'], kw['final_adjust_rots'],
                            grad_trans=torch.ones(2, 3, device=dev))
        return
    in_fixture = case in fu.FIXTURE_CASES.get(name, '')
    seed = int(gold[f'{name}.{case}.seed']) if in_fixture else 7
    x, kw, kid, cot, out, grads = _arbiter(name, case, 2, 0, seed, model_root, golden)
    r, ours = _native(_fitter(name, kid, model_root, golden, dev), x, kw, cot, dev)
    for k in cot:  # the fit the adjoint is evaluated at: the fp32 HIP fit against the fp64 restatement (tests/util.py pose_tol)
        e = np.abs(r[k].cpu().numpy().reshape(out[k].shape) - out[k]).max()
        print(f'[fit-grad] {name} {case} forward {k} ours-vs-fp64 {e:.2e}')
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
    x, kw, kid, cot, _, grads = _arbiter('smpl', 'C', B, B, B, model_root, golden, rows=rows)
    _, ours = _native(_fitter('smpl', kid, model_root, golden, dev), x, kw, cot, dev)
    rel = _reference_rel(gold, 'C', model_root, golden)
    _gate(ours, grads, {k: rel[k] * np.abs(v).max() for k, v in grads.items()}, f'smpl C B={B}', rows)


@pytest.mark.parametrize('case', ['C', 'G'])
def test_autograd_end_to_end(case, model_root, golden, dev):
    """Every tensor input requires grad: the results are the no-gradient call's bits, the gradients the native call's,
    no warning is raised; ``orientations`` alone carries a gradient; no ``grad_fn`` without gradients."""
    x, kw, kid, cot, _, _ = _arbiter('smpl', case, 2, 0, 3, model_root, golden)
    f = _fitter('smpl', kid, model_root, golden, dev)
    r0, native = _native(f, x, kw, cot, dev)
    ts = {k: _t(v, dev).requires_grad_() for k, v in x.items()}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        r = f.fit(**ts, **kw)
    keys = ('pose_rotvecs', 'shape_betas', 'trans', 'orientations', 'relative_orientations') + (('kid_factor',) if kid else ())
    for k in keys:
        assert torch.equal(r[k], r0[k]), k
        assert r[k].grad_fn is not None, k
    sum((r[k].reshape(c.shape) * _t(c, dev)).sum() for k, c in cot.items()).backward()
    for k, t in ts.items():
        assert t.grad is not None and t.grad.shape == t.shape, k
        assert np.array_equal(t.grad.cpu().numpy(), native[k]), k
    tv = _t(x['target_vertices'], dev).requires_grad_()
    rest = {k: v.detach() for k, v in ts.items() if k != 'target_vertices'}
    f.fit(target_vertices=tv, **rest, **kw)['orientations'].square().sum().backward()
    assert torch.isfinite(tv.grad).all() and tv.grad.abs().max().item() > 0
    with torch.no_grad():
        assert f.fit(**ts, **kw)['shape_betas'].grad_fn is None
    assert f.fit(**{k: v.detach() for k, v in ts.items()}, **kw)['shape_betas'].grad_fn is None


@pytest.mark.parametrize('name', ['smpl', 'smplxfat'])
def test_directional_derivative(name, model_root, golden, dev):
    """The autograd directional derivative of case C w.r.t. (target_vertices, target_joints) against central differences
    of the no-gradient HIP call at eps 1e-2, within the 5 % of the reference's own gradient test."""
    x, kw, kid, cot, _, _ = _arbiter(name, 'C', 2, 0, 5, model_root, golden)
    f = _fitter(name, kid, model_root, golden, dev)
    cot = {k: _t(v, dev) for k, v in cot.items()}
    names = ('target_vertices', 'target_joints')
    fixed = {k: _t(v, dev) for k, v in x.items() if k not in names}
    base = {k: _t(x[k], dev) for k in names}
    loss = lambda r: sum((r[k].reshape(c.shape) * c).sum() for k, c in cot.items())  # noqa: E731
    var = {k: v.clone().requires_grad_() for k, v in base.items()}
    loss(f.fit(**var, **fixed, **kw)).backward()
    gen = torch.Generator().manual_seed(7)
    d = {k: torch.randn(v.shape, generator=gen).to(dev) for k, v in base.items()}
    d = {k: v / v.norm() for k, v in d.items()}
    ag = sum((var[k].grad * d[k]).sum().item() for k in names)
    eps = 1e-2
    with torch.no_grad():
        lp = loss(f.fit(**{k: base[k] + eps * d[k] for k in names}, **fixed, **kw)).item()
        lm = loss(f.fit(**{k: base[k] - eps * d[k] for k in names}, **fixed, **kw)).item()
    fd = (lp - lm) / (2 * eps)
    print(f'[fit-grad] direction {name} autograd {ag:.5e} finite differences {fd:.5e}')
    assert abs(ag - fd) / max(abs(ag), abs(fd), 1e-3) < 5e-2, (ag, fd)


def test_output_subsets_and_determinism(model_root, golden, dev):
    """Each output alone gives the bits of the all-outputs call; two runs give identical bits."""
    x, kw, kid, cot, _, _ = _arbiter('smpl', 'C', 2, 0, 11, model_root, golden)
    f = _fitter('smpl', kid, model_root, golden, dev)
    _, full = _native(f, x, kw, cot, dev)
    _, again = _native(f, x, kw, cot, dev)
    assert set(full) == set(f.FIT_GRAD_NAMES)
    for k in full:
        assert np.array_equal(full[k], again[k]), k
    for k in f.FIT_GRAD_NAMES:
        _, one = _native(f, x, kw, cot, dev, want=(k,))
        assert set(one) == {k}
        assert np.array_equal(one[k], full[k]), k


@pytest.mark.parametrize('name,case,B', [('smpl', 'G', 65), ('smplxfat', 'C', 5)])
def test_fit_backward_guards(name, case, B, model_root, golden, dev):
    """smplfit_fit_backward_f32 called directly (every input, every cotangent, every output; three resp. two iterations
    and the refinement, so that every region of its workspace is used; B = 65: a second, partial block of the
    lane-per-instance kernels; smplxfat: more than 32 joints).  Every output and a workspace of exactly the queried size
    lie between two 1 MB guard regions, the outputs pre-filled with NaN, the workspace once zeroed and once filled with
    a NaN pattern: every guard byte survives, every output element is written and finite, the two fills give the same
    bits.  A workspace one byte short is refused before anything is enqueued."""
    from smplfitter_amd import _lib
    from test_gpu_flipper import _guarded, _intact

    g = golden(MODELS[name])
    x, kw, kid = fu.case_inputs(g, case, B, seed=B)
    f = _fitter(name, kid, model_root, golden, dev)
    m = f.body_model
    J, V = m.num_joints, m.num_vertices
    ts = {k: _t(v, dev) for k, v in x.items()}
    rs = np.random.RandomState(B)
    cot = {'grad_' + k: _t(v, dev) for k, v in fu.cotangents(B, B, J, 10, kid).items()}
    cot['grad_orientations'] = _t(rs.randn(B, J, 3, 3).astype(np.float32), dev)
    cot['grad_relative_orientations'] = _t(rs.randn(B, J, 3, 3).astype(np.float32), dev)
    h = m._native(dev, kid=kid)
    nws = h.fit_backward_workspace_bytes(B, kw['num_iter'])
    assert nws > h.shape_solve_backward_workspace_bytes(B)
    sizes = dict(target_vertices=B * V * 3, target_joints=B * J * 3, vertex_weights=B * V, joint_weights=B * J)
    lib = _lib.load()
    mk = lambda outs, ws, n: _lib.FitBackwardArgs(  # noqa: E731
        **{k: v.data_ptr() for k, v in ts.items()}, batch=B, num_iter=kw['num_iter'], beta_regularizer=kw['beta_regularizer'],
        beta_regularizer2=kw['beta_regularizer2'], kid_regularizer=kw.get('kid_regularizer', kw['beta_regularizer']),
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
        _lib.check(lib.smplfit_fit_backward_f32(h.ptr, C.byref(mk({k: o for k, (_, o) in bufs.items()}, ws, nws))))
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
    assert lib.smplfit_fit_backward_f32(h.ptr, C.byref(mk(outs, ws, nws - 1))) == _lib.SMPLFIT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs.values())  # nothing was enqueued


def test_refusals(model_root, golden, dev):
    """``share_beta``, both scale options and the warm starts with gradients raise ``NotImplementedError``."""
    x, kw, kid, _, _, _ = _arbiter('smpl', 'C', 2, 0, 3, model_root, golden)
    f = _fitter('smpl', kid, model_root, golden, dev)
    ts = {k: _t(v, dev) for k, v in x.items()}
    tv = ts.pop('target_vertices').requires_grad_()
    J = ts['target_joints'].shape[1]
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    for bad in (dict(share_beta=True), dict(scale_target=True), dict(scale_fit=True), dict(initial_pose_rotvecs=z(2, J * 3)),
                dict(initial_shape_betas=z(2, 10))):
        with pytest.raises(NotImplementedError):
            f.fit(target_vertices=tv, **ts, **kw, **bad)


@pytest.mark.parametrize('route', ['smpl_b32', 'native_backward=False'])
def test_torchfit_route_kept(route, model_root, golden, dev):
    """More than 17 shape unknowns, and ``BodyFitter(..., native_backward=False)``, take the ``TorchFit`` route with its
    warning and give finite, non-zero gradients."""
    from smplfitter_amd.pt import BodyFitter, BodyModel

    g = golden('smpl')
    if route == 'smpl_b32':
        f = BodyFitter(BodyModel('smpl', 'neutral', model_root=f'{model_root}/smpl_b32', num_betas=32, device=dev))
    else:
        f = BodyFitter(get_model(model_root, 'smpl', g, dev)[0], native_backward=False)
    tv = _t(g['target_vertices'][:2].copy(), dev).requires_grad_()
    with pytest.warns(RuntimeWarning, match='PyTorch'):
        r = f.fit(tv, _t(g['target_joints'][:2].copy(), dev), num_iter=1)
    r['shape_betas'].square().sum().backward()
    assert torch.isfinite(tv.grad).all() and tv.grad.abs().max().item() > 0


def test_poisoned_row(model_root, golden, dev):
    """A NaN in one row leaves every other row's gradients unchanged."""
    g = golden('smpl')
    x, kw, kid = fu.case_inputs(g, 'C', 3)
    f = _fitter('smpl', kid, model_root, golden, dev)
    cot = fu.cotangents(13, 3, g['target_joints'].shape[1], 10, kid)
    _, clean = _native(f, x, kw, cot, dev)
    xp = {k: v.copy() for k, v in x.items()}
    xp['target_vertices'][1, 17, 2] = np.nan
    _, bad = _native(f, xp, kw, cot, dev)
    for k in clean:
        assert np.all(np.isfinite(clean[k])), k
        assert np.array_equal(clean[k][[0, 2]], bad[k][[0, 2]]), k
    assert not np.all(np.isfinite(bad['target_vertices'][1]))
