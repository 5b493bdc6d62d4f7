"""-m gpu: the differentiable fit_with_known_pose (smplfit_shape_solve_backward_f32, BodyFitter._shape_solve_backward and
the autograd Function around the shape solve) against the fp64 arbiter of tests/known_pose_grad_util.py.

Gate, per gradient tensor: max |ours - fp64| <= max(GRAD_REL x max |fp64|, 2 x max |reference fp32 - fp64|).  The second
term comes from tests/golden/golden_known_pose_grad.npz for that case and tensor.  Models and cases the fixture does not
hold (it has SMPL a-f and SMPL-X-fat a, c) take the SMPL entry of the case scaled to the tensor at hand: the
reference's relative error (its error over max |fp64| on SMPL) times max |fp64| of the model under test: the same
solve on the same kind of inputs, whose fp32 error scales with the gradient.
The pose gradient is the native grad_glob_rotmats chained through BodyModel.forward's backward, as autograd does.

Measured on an MI355X (relative to max |fp64| of the tensor, worst over the five models and six cases): pose_rotvecs
6.5e-6, target_vertices 1.9e-6, target_joints 3.1e-6, both ridge references 2.7e-6, vertex_weights 1.7e-4, joint_weights
2.5e-4; the tensor nearest its gate is joint_weights of smpl_w6 f at 0.86 of it.  The weight gradient is delta . res
with res = target - fit of order 1e-2 m, so it magnifies the rounding of the fitted vertex a hundredfold: the adjoint
recomputes the pose blend shapes WITHOUT the template (k_adj_zero_bias) and adds the template once; with the template
inside the posedirs accumulator grad vertex_weights of smplxfat b was 6.8e-8 off (gate 5.3e-8), now 2.0e-8.
"""

import numpy as np
import pytest
import torch

import grad_util
import known_pose_grad_util as ku
import util
from test_gpu_forward_grad import _rows
from test_gpu_parity import get_model
from test_known_pose_grad_host import GRAD_REL, reference_errors

pytestmark = pytest.mark.gpu

# name -> the golden set its inputs come from
MODELS = dict(smpl='smpl', smplxfat='smplxfat', smpl_w6='smpl_w6', smpl1024='smpl1024', smpl_w12='smpl')
_cache, _fitters, _ref_rel = {}, {}, {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gold():
    import os.path as osp

    return np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'golden_known_pose_grad.npz'))


def _model(name, model_root, golden, dev):
    if name not in _cache:
        from smplfitter_amd import modelio
        from smplfitter_amd.pt import BodyModel

        g = golden(MODELS[name])
        if name == 'smpl_w12':
            m = BodyModel('smpl', 'neutral', model_root=f'{model_root}/smpl_w12', num_betas=10, device=dev)
            md = modelio.load_model('smpl', 'neutral', model_root=f'{model_root}/smpl_w12', num_betas=10)
        else:
            m, _ = get_model(model_root, name, g, dev)
            _, md = util.load_md(model_root, name, g)
        _cache[name] = (m, md, grad_util.Model64(md), g)
    return _cache[name]


def _fitter(name, kid, model_root, golden, dev):
    from smplfitter_amd.pt import BodyFitter

    if (name, kid) not in _fitters:
        _fitters[name, kid] = BodyFitter(_model(name, model_root, golden, dev)[0], enable_kid=kid)
    return _fitters[name, kid]


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _native(f, x, kw, kid, cot, dev, want=None):
    """The no-gradient HIP forward, then the native backward call (+ the pose gradient through the forward's backward)."""
    ts = {k: _t(v, dev) for k, v in x.items()}
    with torch.no_grad():
        r = f.fit_with_known_pose(**ts, **kw)
    ct = {k: _t(v, dev) for k, v in cot.items()}
    kid_reg = kw.get('kid_regularizer', kw['beta_regularizer'])
    want = f.GRAD_NAMES if want is None else want
    g = f._shape_solve_backward(
        r['orientations'], ts['target_vertices'], ts.get('target_joints'), ts.get('vertex_weights'),
        ts.get('joint_weights'), kw['beta_regularizer'], kw['beta_regularizer2'], kid_reg,
        ts.get('beta_regularizer_reference'), ts.get('kid_regularizer_reference'), r['shape_betas'], r['trans'],
        r.get('kid_factor'), ct['shape_betas'], ct['trans'], ct.get('kid_factor'), want=want)
    if 'glob_rotmats' in g:
        g['pose_rotvecs'] = f.body_model._backward_direct(ts['pose_rotvecs'], None, None, None, None, None,
                                                          grad_orientations=g['glob_rotmats'])[0]
    torch.cuda.synchronize()
    return r, {k: v.cpu().numpy() for k, v in g.items()}


def _reference_rel(gold, case, model_root, golden, dev):
    """The reference's relative fp32 error per tensor on the SMPL fixture entry of a case (computed once)."""
    if case not in _ref_rel:
        _, md, m64, g = _model('smpl', model_root, golden, dev)
        x, kw, kid = ku.case_inputs(g, case, 2)
        cot = ku.cotangents(int(gold[f'smpl.{case}.seed']), 2, 10, kid)
        _, grads = ku.arbiter(m64, x, kw, kid, cot)
        err = reference_errors(gold, 'smpl', case, grads, md.v_template.shape[0])
        _ref_rel[case] = {k: err[k] / max(np.abs(v).max(), 1e-30) for k, v in grads.items()}
    return _ref_rel[case]


def _gate(ours, grads, ref_err, tag, rows=None):
    worst = {}
    for k, r in grads.items():
        o = ours[k] if rows is None else ours[k][rows]
        assert np.all(np.isfinite(o)), (tag, k)
        err, gate = np.abs(o - r).max(), max(GRAD_REL * np.abs(r).max(), 2 * ref_err[k])
        worst[k] = (err, gate)
        print(f'[kp-grad] {tag} {k} ours-vs-fp64 {err:.2e} ref-vs-fp64 {ref_err[k]:.2e} max {np.abs(r).max():.2e} gate {gate:.2e}')
    for k, (err, gate) in worst.items():
        assert err <= gate, (tag, k, err, gate)


@pytest.mark.parametrize('case', list(ku.CASES))
@pytest.mark.parametrize('name', list(MODELS))
def test_native_vs_arbiter(name, case, model_root, golden, gold, dev):
    m, md, m64, g = _model(name, model_root, golden, dev)
    x, kw, kid = ku.case_inputs(g, case, 2)
    in_fixture = case in ku.FIXTURE_CASES.get(name, '')
    seed = int(gold[f'{name}.{case}.seed']) if in_fixture else 7
    cot = ku.cotangents(seed, 2, 10, kid)
    out, grads = ku.arbiter(m64, x, kw, kid, cot)
    r, ours = _native(_fitter(name, kid, model_root, golden, dev), x, kw, kid, cot, dev)
    for k, v in out.items():  # the forward's solution the adjoint is evaluated at
        e = np.abs(r[k].cpu().numpy() - v).max()
        print(f'[kp-grad] {name} {case} forward {k} ours-vs-fp64 {e:.2e}')
        assert e <= 1e-4, (name, case, k)
    if in_fixture:
        ref_err = reference_errors(gold, name, case, grads, md.v_template.shape[0])
    else:
        rel = _reference_rel(gold, case, model_root, golden, dev)
        ref_err = {k: rel[k] * np.abs(v).max() for k, v in grads.items()}
    _gate(ours, grads, ref_err, f'{name} {case}')
    if case == 'd':
        assert np.all(ours['vertex_weights'] == 0)
    if case == 'f':
        assert ours['beta_regularizer_reference'].shape == (2, 4)


@pytest.mark.parametrize('B', [1, 64, 65, 257])
def test_batch_edges(B, model_root, golden, gold, dev):
    m, md, m64, g = _model('smpl', model_root, golden, dev)
    x, kw, kid = ku.case_inputs(g, 'a', B, seed=B)
    cot = ku.cotangents(B, B, 10, kid)
    _, ours = _native(_fitter('smpl', kid, model_root, golden, dev), x, kw, kid, cot, dev)
    rows = _rows(B)
    _, grads = ku.arbiter(m64, {k: v[rows] for k, v in x.items()}, kw, kid, {k: v[rows] for k, v in cot.items()})
    rel = _reference_rel(gold, 'a', model_root, golden, dev)
    _gate(ours, grads, {k: rel[k] * np.abs(v).max() for k, v in grads.items()}, f'smpl a B={B}', rows)


@pytest.mark.parametrize('case', ['a', 'e'])
def test_autograd_end_to_end(case, model_root, golden, gold, dev):
    """Every tensor input requires grad: the gradients are the native call's bits, the results those of the no-grad call."""
    m, md, m64, g = _model('smpl', model_root, golden, dev)
    x, kw, kid = ku.case_inputs(g, case, 2)
    cot = ku.cotangents(3, 2, 10, kid)
    f = _fitter('smpl', kid, model_root, golden, dev)
    r0, native = _native(f, x, kw, kid, cot, dev)
    ts = {k: _t(v, dev).requires_grad_() for k, v in x.items()}
    r = f.fit_with_known_pose(**ts, **kw)
    for k in ('shape_betas', 'trans', 'orientations', 'relative_orientations') + (('kid_factor',) if kid else ()):
        assert torch.equal(r[k], r0[k]), k
    assert r['shape_betas'].requires_grad and r['orientations'].requires_grad
    sum((r[k] * _t(c, dev)).sum() for k, c in cot.items()).backward()
    for k, t in ts.items():
        assert t.grad is not None and t.grad.shape == t.shape, k
        assert np.array_equal(t.grad.cpu().numpy(), native[k]), k
    # orientations carry gradients to the pose on their own
    pose = _t(x['pose_rotvecs'], dev).requires_grad_()
    r2 = f.fit_with_known_pose(pose, *(ts[k].detach() for k in ('target_vertices', 'target_joints')))
    r2['relative_orientations'].square().sum().backward()
    assert torch.isfinite(pose.grad).all()
    # no gradients wanted: today's code, no grad_fn
    with torch.no_grad():
        assert f.fit_with_known_pose(**ts, **kw)['shape_betas'].grad_fn is None
    assert f.fit_with_known_pose(**{k: v.detach() for k, v in ts.items()}, **kw)['shape_betas'].grad_fn is None


@pytest.mark.parametrize('name', ['smpl', 'smplxfat'])
def test_directional_derivative(name, model_root, golden, dev):
    """The autograd directional derivative w.r.t. (target_vertices, target_joints, pose_rotvecs) against central
    differences of the no-gradient HIP call at eps 1e-2, within the 5 % of the reference's own gradient test."""
    m, md, m64, g = _model(name, model_root, golden, dev)
    x, kw, kid = ku.case_inputs(g, 'a', 2)
    f = _fitter(name, kid, model_root, golden, dev)
    cot = {k: _t(v, dev) for k, v in ku.cotangents(5, 2, 10, kid).items()}
    fixed = {k: _t(v, dev) for k, v in x.items() if k not in ('target_vertices', 'target_joints', 'pose_rotvecs')}
    names = ('target_vertices', 'target_joints', 'pose_rotvecs')
    base = {k: _t(x[k], dev) for k in names}
    loss = lambda r: sum((r[k] * c).sum() for k, c in cot.items())  # noqa: E731
    var = {k: v.clone().requires_grad_() for k, v in base.items()}
    loss(f.fit_with_known_pose(**var, **fixed, **kw)).backward()
    gen = torch.Generator().manual_seed(7)
    d = {k: torch.randn(v.shape, generator=gen).to(dev) for k, v in base.items()}
    d = {k: v / v.norm() for k, v in d.items()}
    ag = sum((var[k].grad * d[k]).sum().item() for k in names)
    eps = 1e-2
    with torch.no_grad():
        lp = loss(f.fit_with_known_pose(**{k: base[k] + eps * d[k] for k in names}, **fixed, **kw)).item()
        lm = loss(f.fit_with_known_pose(**{k: base[k] - eps * d[k] for k in names}, **fixed, **kw)).item()
    fd = (lp - lm) / (2 * eps)
    print(f'[kp-grad] direction {name} autograd {ag:.5e} finite differences {fd:.5e}')
    assert abs(ag - fd) / max(abs(ag), abs(fd), 1e-3) < 5e-2, (ag, fd)


def test_output_subsets_and_determinism(model_root, golden, dev):
    """Each output alone gives the bits of the all-outputs call; two runs give identical bits."""
    m, md, m64, g = _model('smpl', model_root, golden, dev)
    x, kw, kid = ku.case_inputs(g, 'e', 2)
    cot = ku.cotangents(11, 2, 10, kid)
    f = _fitter('smpl', kid, model_root, golden, dev)
    _, full = _native(f, x, kw, kid, cot, dev)
    _, again = _native(f, x, kw, kid, cot, dev)
    assert set(full) == set(f.GRAD_NAMES) | {'pose_rotvecs'}
    for k in full:
        assert np.array_equal(full[k], again[k]), k
    for k in f.GRAD_NAMES:
        _, one = _native(f, x, kw, kid, cot, dev, want=(k,))
        assert set(one) - {'pose_rotvecs'} == {k}
        assert np.array_equal(one[k], full[k]), k


def test_refusals_and_poisoned_row(model_root, golden, dev):
    from smplfitter_amd.pt import BodyFitter, BodyModel

    m, md, m64, g = _model('smpl', model_root, golden, dev)
    x, kw, kid = ku.case_inputs(g, 'a', 3)
    ts = {k: _t(v, dev) for k, v in x.items()}
    tv = ts['target_vertices'].clone().requires_grad_()
    rest = {k: v for k, v in ts.items() if k != 'target_vertices'}
    for d, nb in (('smpl_b32', 32), ('smpl_b300', None)):
        fb = BodyFitter(BodyModel('smpl', 'neutral', model_root=f'{model_root}/{d}', num_betas=nb, device=dev))
        with pytest.raises(NotImplementedError):
            fb.fit_with_known_pose(ts['pose_rotvecs'], tv, ts['target_joints'])
    f = _fitter('smpl', False, model_root, golden, dev)
    for bad in (dict(share_beta=True), dict(scale_target=True), dict(scale_fit=True)):
        with pytest.raises(NotImplementedError):
            f.fit_with_known_pose(target_vertices=tv, **rest, **kw, **bad)
    # a NaN in one row leaves every other row's gradients unchanged
    cot = ku.cotangents(13, 3, 10, kid)
    _, clean = _native(f, x, kw, kid, cot, dev)
    xp = {k: v.copy() for k, v in x.items()}
    xp['target_vertices'][1, 17, 2] = np.nan
    _, bad = _native(f, xp, kw, kid, cot, dev)
    for k in clean:
        assert np.array_equal(clean[k][[0, 2]], bad[k][[0, 2]]), k
    assert np.isnan(bad['vertex_weights'][1]).any()  # (delta . res: the residual of the poisoned row)


@pytest.mark.parametrize('name,B', [('smpl', 65), ('smplxfat', 5)])
def test_shape_solve_backward_guards(name, B, model_root, golden, dev):
    """smplfit_shape_solve_backward_f32 called directly on case e (target joints, both weight kinds, a kid handle, both
    ridge references) with every gradient output requested, so that every region of its workspace is used and the three
    backward passes run; B = 65: a second, partial block of k_bwd_joint; smplxfat: more than 32 joints.  Every output
    and a workspace of exactly the queried size lie between two 1 MB guard regions, the outputs pre-filled with NaN, the
    workspace once zeroed and once filled with a NaN pattern: every guard byte survives, every output element is
    written and finite, the two fills give the same bits.  A workspace one byte short is refused before anything is
    enqueued."""
    import ctypes as C

    from smplfitter_amd import _lib
    from test_gpu_flipper import _guarded, _intact

    m, md, m64, g = _model(name, model_root, golden, dev)
    x, kw, kid = ku.case_inputs(g, 'e', B, seed=B)
    assert kid
    f = _fitter(name, kid, model_root, golden, dev)
    ts = {k: _t(v, dev) for k, v in x.items()}
    with torch.no_grad():
        r = f.fit_with_known_pose(**ts, **kw)
    cot = {k: _t(v, dev) for k, v in ku.cotangents(B, B, 10, kid).items()}
    J, V, nref = m.num_joints, m.num_vertices, x['beta_regularizer_reference'].shape[1]
    G = r['orientations'].contiguous()
    h = m._native(dev, kid=True)
    nws = h.shape_solve_backward_workspace_bytes(B)
    assert nws > h.forward_backward_workspace_bytes(B)
    sizes = dict(glob_rotmats=B * J * 9, target_vertices=B * V * 3, target_joints=B * J * 3, vertex_weights=B * V,
                 joint_weights=B * J, beta_regularizer_reference=B * nref, kid_regularizer_reference=B)
    lib = _lib.load()
    mk = lambda outs, ws, n: _lib.ShapeSolveBackwardArgs(  # noqa: E731
        glob_rotmats=G.data_ptr(), target_vertices=ts['target_vertices'].data_ptr(),
        target_joints=ts['target_joints'].data_ptr(), vertex_weights=ts['vertex_weights'].data_ptr(),
        joint_weights=ts['joint_weights'].data_ptr(), beta_regularizer=kw['beta_regularizer'],
        beta_regularizer2=kw['beta_regularizer2'], kid_regularizer=kw['kid_regularizer'],
        beta_regularizer_reference=ts['beta_regularizer_reference'].data_ptr(), num_reference_betas=nref,
        kid_regularizer_reference=ts['kid_regularizer_reference'].data_ptr(), batch=B,
        shape_betas=r['shape_betas'].data_ptr(), trans=r['trans'].data_ptr(), kid_factor=r['kid_factor'].data_ptr(),
        grad_shape_betas=cot['shape_betas'].data_ptr(), grad_trans=cot['trans'].data_ptr(),
        grad_kid_factor=cot['kid_factor'].data_ptr(), workspace=ws.data_ptr(), workspace_bytes=n,
        hip_stream=torch.cuda.current_stream(dev).cuda_stream,
        **{f'grad_{k}': o.data_ptr() for k, o in outs.items()})
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
        _lib.check(lib.smplfit_shape_solve_backward_f32(h.ptr, C.byref(mk({k: o for k, (_, o) in bufs.items()}, ws, nws))))
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
    assert lib.smplfit_shape_solve_backward_f32(h.ptr, C.byref(mk(outs, ws, nws - 1))) == _lib.SMPLFIT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs.values())  # nothing was enqueued
