"""-m gpu: the mesh-distance objective call (smplfit_mesh_objective_f32, BodyModel._objective_direct) and BodyFlipperOpt.

* value and gradient against the fp64 torch restatement (tests/grad_util.py) with the loss written in torch.  Gate per
  gradient tensor: max |ours - fp64| <= max(GRAD_REL x max |fp64|, 2 x the same error of the existing path —
  BodyModel.forward under autograd with the loss in torch operators — measured in the same test); loss 1e-5 relative;
* guard regions, NaN-filled outputs, zeroed / NaN-patterned workspace, run-to-run bits, NULL outputs in turn;
* refine_steps = 0 is BodyFlipper.flip; the refinement against the reference's fixture
  (tests/golden/make_golden_flip_opt.py): at least half of the reference's own improvement of the objective, evaluated
  by the fp64 oracle.

Every test prints its figures before it asserts (the errors of the fused and, in brackets, of the unfused path; the
share of the reference's improvement the refinement reaches).
"""

import ctypes as C

import numpy as np
import pytest
import torch

import flip_opt_util
import flip_util
import grad_util
from test_gpu_flipper import _guarded, _intact, get_model, inputs, t, to_np

pytestmark = pytest.mark.gpu

GRAD_REL = 2e-4  # the project's gradient gate (tests/test_gpu_forward_grad.py)
# name -> (directory under the model root, model kind, num_betas)
GRAD_MODELS = {'smpl': ('smpl', 'smpl', 10), 'smplxfat': ('smplx_fat', 'smplx', 10), 'smpl_b32': ('smpl_b32', 'smpl', 32)}
_gm = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gfo(golden):
    return golden('flip_opt')


def _gmodel(name, model_root, dev):
    if name not in _gm:
        from smplfitter_amd import modelio
        from smplfitter_amd.pt import BodyModel

        d, kind, nb = GRAD_MODELS[name]
        m = BodyModel(kind, 'neutral', model_root=f'{model_root}/{d}', num_betas=nb, device=dev)
        md = modelio.load_model(kind, 'neutral', model_root=f'{model_root}/{d}', num_betas=nb)
        _gm[name] = (m, grad_util.Model64(md))
    return _gm[name]


def _rot(rv):
    return grad_util.rotvec2mat(torch.as_tensor(rv, dtype=torch.float64)).numpy()


def _case(m64, B, V, form, kid, weights, seed):
    """Inputs x (fp32), the target = the fp64 forward of parameters perturbed by 0.05 rad / 0.3 in the betas (residuals
    of centimetres: the direction r / |r| is well conditioned), and the weights: uniform in [0, 2], one in ten exactly 0."""
    rs = np.random.RandomState(seed)
    J, S = m64.J, m64.S
    pose = rs.randn(B, J, 3) * 0.4
    dpose = rs.randn(B, J, 3) * 0.05
    x = dict(shape_betas=rs.randn(B, S) * (1.0 if S <= 10 else 0.5), trans=rs.randn(B, 3))
    y = dict(shape_betas=x['shape_betas'] + 0.3 * rs.randn(B, S), trans=x['trans'] + 0.01 * rs.randn(B, 3))
    if form == 'pose':
        x['pose_rotvecs'] = pose.reshape(B, J * 3)
        y['pose_rotvecs'] = (pose + dpose).reshape(B, J * 3)
    elif form == 'rel':
        x['rel_rotmats'] = _rot(pose)
    else:
        x['glob_rotmats'] = grad_util.random_rotmats(rs, (B, J))
    x = {k: v.astype(np.float32) for k, v in x.items()}
    for k in ('rel_rotmats', 'glob_rotmats'):
        if k in x:
            y[k] = x[k].astype(np.float64) @ _rot(dpose)
    if kid:
        x['kid_factor'] = rs.uniform(-0.5, 1.5, B).astype(np.float32)
        y['kid_factor'] = x['kid_factor'] + 0.05 * rs.randn(B)
    with torch.no_grad():
        target = grad_util.forward(m64, **{k: torch.as_tensor(v, dtype=torch.float64) for k, v in y.items()})['vertices']
    w = None
    if weights:
        w = rs.uniform(0, 2, (B, V))
        w[rs.rand(B, V) < 0.1] = 0.0
        w = w.astype(np.float32)
    return x, target.numpy().astype(np.float32), w


def _loss_torch(vertices, target, w, scale):
    d = torch.linalg.norm(vertices - target, dim=-1)
    return scale * (d if w is None else w * d).sum(-1)


def _fp64(m64, x, target, w, scale, rows):
    ts = {k: torch.tensor(v[rows].astype(np.float64), requires_grad=True) for k, v in x.items()}
    loss = _loss_torch(grad_util.forward(m64, **ts)['vertices'], torch.tensor(target[rows].astype(np.float64)),
                       None if w is None else torch.tensor(w[rows].astype(np.float64)), scale)
    gs = torch.autograd.grad(loss.sum(), list(ts.values()))
    return loss.detach().numpy(), {k: g.numpy() for k, g in zip(ts, gs)}


def _fused(m, x, target, w, scale, dev):
    ins = {k: t(v, dev) for k, v in x.items()}
    loss, gs = m._objective_direct(t(target, dev), vertex_weights=t(w, dev), scale=scale, **ins)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), {k: g.cpu().numpy() for k, g in zip(grad_util.INPUT_NAMES, gs) if g is not None}


def _unfused(m, x, target, w, scale, dev):
    ins = {k: t(v, dev).requires_grad_() for k, v in x.items()}
    loss = _loss_torch(m(**ins)['vertices'], t(target, dev), t(w, dev), scale)
    loss.sum().backward()
    return loss.detach().cpu().numpy(), {k: v.grad.cpu().numpy() for k, v in ins.items()}


@pytest.mark.parametrize('name,B,form', [('smpl', 1, 'rel'), ('smpl', 3, 'rel'), ('smpl', 65, 'rel'), ('smplxfat', 5, 'rel'),
                                         ('smpl_b32', 2, 'rel'), ('smpl', 3, 'pose'), ('smpl', 3, 'glob')])
def test_objective_against_fp64(name, B, form, model_root, dev):
    """B = 65: k_bwd_joint runs 64 lanes, so a second, partial block; smpl_b32: the general-path model.  With and
    without kid_factor, with and without vertex_weights."""
    m, m64 = _gmodel(name, model_root, dev)
    V = m.num_vertices
    scale = 1.0 / (B * V)
    rows = np.arange(B) if B <= 8 else np.array([0, 1, 31, 63, 64])  # (the instances are independent)
    for kid in (False, True):
        for weights in (False, True):
            x, target, w = _case(m64, B, V, form, kid, weights, seed=B + 2 * kid + weights)
            loss64, g64 = _fp64(m64, x, target, w, scale, rows)
            loss, g = _fused(m, x, target, w, scale, dev)
            loss_u, g_u = _unfused(m, x, target, w, scale, dev)
            assert set(g) == set(x) and loss.shape == (B,)
            rel_loss = np.abs(loss[rows] - loss64).max() / np.abs(loss64).max()
            line = [f'loss {rel_loss:.1e}']
            fails = []
            for k, r in g64.items():
                ref = max(np.abs(r).max(), 1e-30)
                err = np.abs(g[k][rows] - r).max()
                err_u = np.abs(g_u[k][rows] - r).max()
                line.append(f'{k} {err / ref:.1e} ({err_u / ref:.1e})')
                assert np.all(np.isfinite(g[k])), (name, k)
                if err > max(GRAD_REL * ref, 2 * err_u):
                    fails.append((k, err, err_u, ref))
            print(f'[objective] {name} B={B} {form} kid={int(kid)} w={int(weights)}: ' + ', '.join(line))
            assert rel_loss <= 1e-5, (name, B, form, kid, weights, rel_loss)
            assert not fails, (name, B, form, kid, weights, fails)


def _objective_args(_lib, x, target, w, scale, B, nb, outs, ws, nws, dev):
    p = lambda o: None if o is None else o.data_ptr()  # noqa: E731
    return _lib.MeshObjectiveArgs(
        rel_rotmats=x['rel_rotmats'].data_ptr(), shape_betas=x['shape_betas'].data_ptr(), num_betas_given=nb,
        trans=x['trans'].data_ptr(), kid_factor=x['kid_factor'].data_ptr(), batch=B, target_vertices=target.data_ptr(),
        vertex_weights=w.data_ptr(), scale=scale, loss=p(outs['loss']), grad_rel_rotmats=p(outs['rel']),
        grad_shape_betas=p(outs['betas']), grad_trans=p(outs['trans']), grad_kid_factor=p(outs['kid']),
        workspace=ws.data_ptr(), workspace_bytes=nws, hip_stream=torch.cuda.current_stream(dev).cuda_stream)


@pytest.mark.parametrize('name,B', [('smpl', 130), ('smplxfat', 5)])
def test_objective_guards(name, B, model_root, dev):
    """smplfit_mesh_objective_f32 called directly with every output and the workspace between two 1 MB guard regions,
    outputs pre-filled with NaN, the workspace once zeroed and once filled with a NaN pattern: every guard byte survives,
    every output element is written and finite, the two runs give the same bits.  A workspace one byte short is refused.
    Each NULL-able output left NULL in turn leaves the others' bits unchanged."""
    from smplfitter_amd import _lib

    m, m64 = _gmodel(name, model_root, dev)
    J, V, nb = m.num_joints, m.num_vertices, 10
    xn, target, w = _case(m64, min(B, 4), V, 'rel', True, True, seed=3)
    rep = lambda a: t(np.ascontiguousarray(np.resize(a, (B,) + a.shape[1:])), dev)  # noqa: E731  (rows repeated)
    x, target, w = {k: rep(v) for k, v in xn.items()}, rep(target), rep(w)
    scale = 1.0 / (B * V)
    h = m._native(dev, kid=True)
    nws = h.mesh_objective_workspace_bytes(B)
    sizes = dict(loss=B, rel=B * J * 9, betas=B * nb, trans=B * 3, kid=B)
    lib = _lib.load()
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
        args = _objective_args(_lib, x, target, w, scale, B, nb, {k: o for k, (_, o) in bufs.items()}, ws, nws, dev)
        _lib.check(lib.smplfit_mesh_objective_f32(h.ptr, C.byref(args)))
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
    plain = lambda: {k: torch.full((n,), float('nan'), device=dev) for k, n in sizes.items()}  # noqa: E731
    outs = plain()
    args = _objective_args(_lib, x, target, w, scale, B, nb, outs, ws, nws - 1, dev)
    assert lib.smplfit_mesh_objective_f32(h.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs.values())  # nothing was enqueued
    for missing in ('rel', 'betas', 'trans', 'kid'):
        outs = plain()
        outs[missing] = None
        args = _objective_args(_lib, x, target, w, scale, B, nb, outs, ws, nws, dev)
        _lib.check(lib.smplfit_mesh_objective_f32(h.ptr, C.byref(args)))
        torch.cuda.synchronize()
        for k, o in outs.items():
            if o is not None:
                assert torch.equal(o.view(torch.uint8), out['zero'][k]), (missing, k)
    args.loss = None  # the loss is required
    assert lib.smplfit_mesh_objective_f32(h.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_BAD_ARG


@pytest.mark.parametrize('kid', [False, True])
def test_no_refinement_is_the_flip(kid, model_root, dev, data_root_fat, monkeypatch):
    from smplfitter_amd.pt import BodyFlipperOpt

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, _ = get_model(model_root, 'smpl', dev)
    fl = BodyFlipperOpt(m)
    pose, betas, trans, k = (t(a, dev) for a in inputs(m.num_joints, 9, 4, kid))
    a = fl.flip(pose, betas, trans, kid_factor=k, num_iter=2)
    b = fl.flipper.flip(pose, betas, trans, kid_factor=k, num_iter=2)
    assert set(a) == set(flip_util.FLIP_KEYS)
    for key in flip_util.FLIP_KEYS:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])
@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_refinement_against_reference(tag, fused, model_root, gfo, dev, data_root_fat, monkeypatch):
    """The fixture's inputs, 100 steps: finite results with the reference's keys whose objective (fp64 oracle, against
    the oracle-mirrored target, as the generator evaluates it) reaches at least half of the reference's own improvement:
    obj <= obj0 - 0.5 (obj0 - obj100).  Parameter-space parity is not asked: Adam's first steps move every component by
    about the learning rate in the direction of the gradient's sign, so two fp32 implementations part ways on components
    whose gradient is near zero, then both descend."""
    from smplfitter_amd.pt import BodyFlipperOpt

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, om64 = get_model(model_root, tag, dev)
    fl = BodyFlipperOpt(m, fused_objective=fused)
    pose, betas, trans, kid = (gfo[f'{tag}.{k}'] for k in ('pose', 'betas', 'trans', 'kid'))
    for case in flip_opt_util.CASES:
        ni, with_kid = flip_util.case_args(case)
        kf = kid if with_kid else None
        o = to_np(fl.flip(t(pose, dev), t(betas, dev), t(trans, dev), kid_factor=t(kf, dev), num_iter=ni,
                          refine_steps=flip_opt_util.STEPS))
        assert set(o) == set(flip_util.FLIP_KEYS) == {str(k) for k in gfo['keys']}
        assert all(np.isfinite(v).all() for v in o.values())
        assert o['pose_rotvecs'].shape == pose.shape and o['kid_factor'].shape == (pose.shape[0],)
        target = flip_opt_util.target64(om64, fl.flipper.mirror_csr, pose, betas, trans, kf)
        obj = flip_opt_util.objective64(om64, o, target)
        obj0, obj100 = float(gfo[f'{tag}.{case}.obj0']), float(gfo[f'{tag}.{case}.obj100'])
        share = (obj0 - obj) / (obj0 - obj100)
        print(f'[flip-opt] {tag} {case} {"fused" if fused else "unfused"}: {obj * 1e3:.3f} mm (reference {obj0 * 1e3:.3f} '
              f'-> {obj100 * 1e3:.3f} mm), share of the reference\'s improvement {share:.3f}')
        assert obj <= obj0 - 0.5 * (obj0 - obj100), (tag, case, fused, obj, obj0, obj100)


def test_refinement_deterministic(model_root, dev, data_root_fat, monkeypatch):
    """Two fused refinements of the same batch (B = 65, 10 steps) give the same bits."""
    from smplfitter_amd.pt import BodyFlipperOpt

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, _ = get_model(model_root, 'smpl', dev)
    fl = BodyFlipperOpt(m)
    pose, betas, trans, kid = (t(a, dev) for a in inputs(m.num_joints, 65, 29, kid=True))
    a = fl.flip(pose, betas, trans, kid_factor=kid, refine_steps=10)
    b = fl.flip(pose, betas, trans, kid_factor=kid, refine_steps=10)
    for k in flip_util.FLIP_KEYS:
        assert torch.equal(a[k], b[k]), k
    start = fl.flipper.flip(pose, betas, trans, kid_factor=kid)
    assert not torch.equal(a['pose_rotvecs'], start['pose_rotvecs'])  # (the refinement ran)


def test_argument_handling(model_root, dev, data_root_fat, monkeypatch):
    from smplfitter_amd.pt import BodyFlipperOpt

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m, _ = get_model(model_root, 'smpl', dev)
    fl = BodyFlipperOpt(m)
    J = m.num_joints
    pose, betas, trans, _ = (t(a, dev) for a in inputs(J, 4, 1))
    for bad in ((pose.clone().requires_grad_(), betas, trans), (pose, betas, trans.clone().requires_grad_())):
        with pytest.raises(NotImplementedError):
            fl.flip(*bad, refine_steps=2)
    empty = fl.flip(pose[:0], betas[:0], trans[:0], refine_steps=5)
    assert set(empty) == set(flip_util.FLIP_KEYS)
    assert empty['pose_rotvecs'].shape == (0, 3 * J) and empty['trans'].shape == (0, 3)
    assert empty['shape_betas'].shape[0] == 0 and empty['kid_factor'].shape == (0,)
    loss, grads = m._objective_direct(torch.zeros(0, m.num_vertices, 3, device=dev), shape_betas=betas[:0])
    assert loss.shape == (0,) and grads[1].shape == betas[:0].shape
