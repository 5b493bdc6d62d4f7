"""-m gpu: the fit objective — the mesh-distance objective with a joint term (smplfit_fit_objective_f32,
BodyModel._objective_direct with target_joints) — and BodyFitterOpt's fused refinement on it.

* value and gradient against the fp64 torch restatement (tests/grad_util.py) with both terms of the loss written in
  torch.  Gate per gradient tensor: max |ours - fp64| <= max(GRAD_REL x max |fp64|, 2 x the same error of the existing
  path — BodyModel.forward under autograd with the loss in torch operators — measured in the same test); loss 1e-5
  relative.  One target joint per instance equals the fp32 joint the library returns: the zero-distance path, whose
  term and cotangent are exactly 0 (torch.linalg.norm's backward), so the fp64 restatement leaves that joint out;
* guard regions, NaN-filled outputs, zeroed / NaN-patterned workspace, run-to-run bits, NULL outputs in turn;
* without target joints the call is smplfit_mesh_objective_f32 bit for bit; with scale = 0 it is
  smplfit_forward_backward_f32 fed the joint cotangent;
* BodyFitterOpt, fused and unfused, against the reference's fixture (tests/golden/make_golden_fitter_opt.py): at least
  half of the reference's own improvement of the objective, evaluated by the fp64 oracle; fused against unfused from
  one start; determinism; argument handling.

Every test prints its figures before it asserts.
"""

import ctypes as C

import numpy as np
import pytest
import torch

import fitter_opt_util as U
import grad_util
from test_gpu_flipper import _guarded, _intact, get_model, t, to_np
from test_gpu_flipper_opt import GRAD_REL, _case, _gmodel, _loss_torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gfo(golden):
    return golden('fitter_opt')


def _joint_case(m, m64, x, weights, seed, dev):
    """Target joints: the fp64 joints at the inputs plus 3 cm of Gaussian noise (a well-conditioned direction), joint
    b % J of instance b replaced by the fp32 joint of the library's own forward (zero distance; `live` is 0 there);
    joint weights uniform in [0, 2], one in ten exactly 0."""
    rs = np.random.RandomState(1000 + seed)
    with torch.no_grad():
        j64 = grad_util.forward(m64, **{k: torch.as_tensor(v, dtype=torch.float64) for k, v in x.items()},
                                return_vertices=False)['joints'].numpy()
        j32 = m(**{k: t(v, dev) for k, v in x.items()}, return_vertices=False)['joints'].cpu().numpy()
    B, J = j64.shape[:2]
    tj = (j64 + 0.03 * rs.randn(B, J, 3)).astype(np.float32)
    live = np.ones((B, J))
    zero = np.arange(B) % J
    tj[np.arange(B), zero] = j32[np.arange(B), zero]
    live[np.arange(B), zero] = 0.0
    jw = None
    if weights:
        jw = rs.uniform(0, 2, (B, J))
        jw[rs.rand(B, J) < 0.1] = 0.0
        jw = jw.astype(np.float32)
    return tj, jw, live


def _joint_loss_torch(joints, tj, jw, joint_scale, live=None):
    d = torch.linalg.norm(joints - tj, dim=-1)
    if jw is not None:
        d = jw * d
    if live is not None:
        d = live * d
    return joint_scale * d.sum(-1)


def _fp64(m64, x, target, w, scale, tj, jw, joint_scale, live, rows):
    f64 = lambda a: None if a is None else torch.tensor(a[rows].astype(np.float64))  # noqa: E731
    ts = {k: torch.tensor(v[rows].astype(np.float64), requires_grad=True) for k, v in x.items()}
    out = grad_util.forward(m64, **ts)
    loss = _loss_torch(out['vertices'], f64(target), f64(w), scale)
    loss = loss + _joint_loss_torch(out['joints'], f64(tj), f64(jw), joint_scale, f64(live))
    gs = torch.autograd.grad(loss.sum(), list(ts.values()))
    return loss.detach().numpy(), {k: g.numpy() for k, g in zip(ts, gs)}


def _fused(m, x, target, w, scale, tj, jw, joint_scale, dev):
    ins = {k: t(v, dev) for k, v in x.items()}
    loss, gs = m._objective_direct(t(target, dev), vertex_weights=t(w, dev), scale=scale, target_joints=t(tj, dev),
                                   joint_weights=t(jw, dev), joint_scale=joint_scale, **ins)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), {k: g.cpu().numpy() for k, g in zip(grad_util.INPUT_NAMES, gs) if g is not None}


def _unfused(m, x, target, w, scale, tj, jw, joint_scale, dev):
    ins = {k: t(v, dev).requires_grad_() for k, v in x.items()}
    out = m(**ins)
    loss = _loss_torch(out['vertices'], t(target, dev), t(w, dev), scale)
    loss = loss + _joint_loss_torch(out['joints'], t(tj, dev), t(jw, dev), joint_scale)
    loss.sum().backward()
    return loss.detach().cpu().numpy(), {k: v.grad.cpu().numpy() for k, v in ins.items()}


@pytest.mark.parametrize('name,B,form', [('smpl', 1, 'glob'), ('smpl', 3, 'glob'), ('smpl', 65, 'glob'),
                                         ('smplxfat', 5, 'glob'), ('smpl_b32', 2, 'glob'), ('smpl', 3, 'rel'),
                                         ('smpl', 3, 'pose')])
def test_fit_objective_against_fp64(name, B, form, model_root, dev):
    """B = 65: k_obj_joint and k_bwd_joint run 64 lanes, so a second, partial block; smplxfat: 55 joints, four LDS
    stages of k_obj_joint, the last one partial; smpl_b32: the general-path model.  With and without kid_factor, with
    and without both weight arrays."""
    m, m64 = _gmodel(name, model_root, dev)
    V, J = m.num_vertices, m.num_joints
    scale, joint_scale = 1.0 / (B * V), 1.0 / (B * J)
    rows = np.arange(B) if B <= 8 else np.array([0, 1, 31, 63, 64])  # (the instances are independent)
    for kid in (False, True):
        for weights in (False, True):
            seed = B + 2 * kid + weights
            x, target, w = _case(m64, B, V, form, kid, weights, seed=seed)
            tj, jw, live = _joint_case(m, m64, x, weights, seed, dev)
            loss64, g64 = _fp64(m64, x, target, w, scale, tj, jw, joint_scale, live, rows)
            loss, g = _fused(m, x, target, w, scale, tj, jw, joint_scale, dev)
            loss_u, g_u = _unfused(m, x, target, w, scale, tj, jw, joint_scale, dev)
            assert set(g) == set(x) and loss.shape == (B,)
            assert np.all(np.isfinite(loss))
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
            print(f'[fit-objective] {name} B={B} {form} kid={int(kid)} w={int(weights)}: ' + ', '.join(line))
            assert rel_loss <= 1e-5, (name, B, form, kid, weights, rel_loss)
            assert not fails, (name, B, form, kid, weights, fails)


def _fit_objective_args(_lib, x, target, w, scale, tj, jw, joint_scale, B, nb, outs, ws, nws, dev):
    p = lambda o: None if o is None else o.data_ptr()  # noqa: E731
    return _lib.FitObjectiveArgs(
        rel_rotmats=x['rel_rotmats'].data_ptr(), shape_betas=x['shape_betas'].data_ptr(), num_betas_given=nb,
        trans=x['trans'].data_ptr(), kid_factor=x['kid_factor'].data_ptr(), batch=B, target_vertices=target.data_ptr(),
        vertex_weights=w.data_ptr(), scale=scale, target_joints=p(tj), joint_weights=p(jw), joint_scale=joint_scale,
        loss=p(outs['loss']), grad_rel_rotmats=p(outs['rel']), grad_shape_betas=p(outs['betas']),
        grad_trans=p(outs['trans']), grad_kid_factor=p(outs['kid']), workspace=ws.data_ptr(), workspace_bytes=nws,
        hip_stream=torch.cuda.current_stream(dev).cuda_stream)


def _guard_inputs(name, B, model_root, dev):
    m, m64 = _gmodel(name, model_root, dev)
    xn, target, w = _case(m64, min(B, 4), m.num_vertices, 'rel', True, True, seed=3)
    tj, jw, _ = _joint_case(m, m64, xn, True, 3, dev)
    rep = lambda a: t(np.ascontiguousarray(np.resize(a, (B,) + a.shape[1:])), dev)  # noqa: E731  (rows repeated)
    return m, {k: rep(v) for k, v in xn.items()}, rep(target), rep(w), rep(tj), rep(jw)


@pytest.mark.parametrize('name,B', [('smpl', 130), ('smplxfat', 5)])
def test_fit_objective_guards(name, B, model_root, dev):
    """smplfit_fit_objective_f32 called directly with every output and the workspace between two 1 MB guard regions,
    outputs pre-filled with NaN, the workspace once zeroed and once filled with a NaN pattern: every guard byte survives,
    every output element is written and finite, the two runs give the same bits.  A workspace one byte short is refused
    and nothing is enqueued.  Each NULL-able output left NULL in turn leaves the others' bits unchanged.  joint_weights
    without target_joints is refused."""
    from smplfitter_amd import _lib

    m, x, target, w, tj, jw = _guard_inputs(name, B, model_root, dev)
    J, V, nb = m.num_joints, m.num_vertices, 10
    scale, joint_scale = 1.0 / (B * V), 1.0 / (B * J)
    h = m._native(dev, kid=True)
    nws = h.fit_objective_workspace_bytes(B)
    assert nws >= h.mesh_objective_workspace_bytes(B) + B * J * 12
    sizes = dict(loss=B, rel=B * J * 9, betas=B * nb, trans=B * 3, kid=B)
    lib = _lib.load()
    mk = lambda outs, ws, n, tj_=tj, jw_=jw: _fit_objective_args(  # noqa: E731
        _lib, x, target, w, scale, tj_, jw_, joint_scale, B, nb, outs, ws, n, dev)
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
        args = mk({k: o for k, (_, o) in bufs.items()}, ws, nws)
        _lib.check(lib.smplfit_fit_objective_f32(h.ptr, C.byref(args)))
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
    args = mk(outs, ws, nws - 1)
    assert lib.smplfit_fit_objective_f32(h.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs.values())  # nothing was enqueued
    for missing in ('rel', 'betas', 'trans', 'kid'):
        outs = plain()
        outs[missing] = None
        args = mk(outs, ws, nws)
        _lib.check(lib.smplfit_fit_objective_f32(h.ptr, C.byref(args)))
        torch.cuda.synchronize()
        for k, o in outs.items():
            if o is not None:
                assert torch.equal(o.view(torch.uint8), out['zero'][k]), (missing, k)
    outs = plain()
    args = mk(outs, ws, nws, tj_=None)  # joint_weights without target_joints
    assert lib.smplfit_fit_objective_f32(h.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_BAD_ARG
    args = mk(outs, ws, nws)
    args.loss = None  # the loss is required
    assert lib.smplfit_fit_objective_f32(h.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs.values())


@pytest.mark.parametrize('name,B', [('smpl', 65), ('smplxfat', 5)])
def test_no_joint_term_is_the_mesh_objective(name, B, model_root, dev):
    """target_joints NULL: the loss and every gradient equal smplfit_mesh_objective_f32's (through
    BodyModel._objective_direct), bit for bit."""
    from smplfitter_amd import _lib

    m, x, target, w, _, _ = _guard_inputs(name, B, model_root, dev)
    J, V, nb = m.num_joints, m.num_vertices, 10
    scale = 1.0 / (B * V)
    loss_ref, g_ref = m._objective_direct(target, vertex_weights=w, scale=scale, **x)
    h = m._native(dev, kid=True)
    nws = h.fit_objective_workspace_bytes(B)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    outs = {k: torch.full((n,), float('nan'), device=dev)
            for k, n in dict(loss=B, rel=B * J * 9, betas=B * nb, trans=B * 3, kid=B).items()}
    args = _fit_objective_args(_lib, x, target, w, scale, None, None, 123.0, B, nb, outs, ws, nws, dev)
    _lib.check(_lib.load().smplfit_fit_objective_f32(h.ptr, C.byref(args)))
    torch.cuda.synchronize()
    ref = dict(loss=loss_ref, rel=g_ref[4], betas=g_ref[1], trans=g_ref[2], kid=g_ref[3])
    for k, o in outs.items():
        assert torch.equal(o, ref[k].reshape(-1)), k


@pytest.mark.parametrize('name,B,form', [('smpl', 65, 'glob'), ('smplxfat', 5, 'rel'), ('smpl', 3, 'pose')])
def test_joint_term_alone(name, B, form, model_root, dev):
    """scale = 0: the gradients equal smplfit_forward_backward_f32's fed the joint cotangent computed in torch as
    grad_joints and no grad_vertices, within GRAD_REL of each tensor's largest element; the loss is the joint term."""
    m, m64 = _gmodel(name, model_root, dev)
    V, J = m.num_vertices, m.num_joints
    joint_scale = 1.0 / (B * J)
    x, target, w = _case(m64, B, V, form, True, True, seed=11)
    tj, jw, _ = _joint_case(m, m64, x, True, 11, dev)
    loss, g = _fused(m, x, target, w, 0.0, tj, jw, joint_scale, dev)
    ins = {k: t(v, dev) for k, v in x.items()}
    with torch.no_grad():
        p = m(**ins, return_vertices=False)['joints']
    r = p - t(tj, dev)
    d = torch.linalg.norm(r, dim=-1, keepdim=True)
    u = joint_scale * t(jw, dev)[..., None]
    cot = torch.where(d > 0, u * r / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(r))
    gs = m._backward_direct(ins.get('pose_rotvecs'), ins['shape_betas'], ins['trans'], ins['kid_factor'],
                            ins.get('rel_rotmats'), ins.get('glob_rotmats'), grad_joints=cot)
    torch.cuda.synchronize()
    ref = {k: v.cpu().numpy() for k, v in zip(grad_util.INPUT_NAMES, gs) if v is not None}
    loss_ref = (u[..., 0] * d[..., 0]).sum(-1).cpu().numpy()
    line = [f'loss {np.abs(loss - loss_ref).max() / np.abs(loss_ref).max():.1e}']
    assert set(ref) == set(g)
    fails = []
    for k, rv in ref.items():
        scale_k = max(np.abs(rv).max(), 1e-30)
        err = np.abs(g[k] - rv).max()
        line.append(f'{k} {err / scale_k:.1e}')
        if not np.all(np.isfinite(g[k])) or err > GRAD_REL * scale_k:
            fails.append((k, err, scale_k))
    print(f'[joint-term] {name} B={B} {form}: ' + ', '.join(line))
    assert np.abs(loss - loss_ref).max() <= 1e-5 * np.abs(loss_ref).max()
    assert not fails, fails


def _fixture_inputs(gfo, om64, case, dev):
    joints, kid = U.case_args(case)
    tv, tj = U.targets(om64, gfo)
    tj, jw = (tj, gfo['joint_weights']) if joints else (None, None)
    return kid, tv, tj, jw


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])
def test_refinement_against_reference(fused, model_root, gfo, dev):
    """The fixture's inputs, 100 steps: finite results with the reference's keys whose objective (fp64 oracle, as the
    generator evaluates it) reaches at least half of the reference's own improvement: obj <= obj0 - 0.5 (obj0 - obj100).
    Parameter parity is not asked (tests/test_gpu_flipper_opt.py::test_refinement_against_reference says why)."""
    from smplfitter_amd.pt import BodyFitterOpt

    m, om64 = get_model(model_root, 'smpl', dev)
    for case in U.CASES:
        kid, tv, tj, jw = _fixture_inputs(gfo, om64, case, dev)
        fo = BodyFitterOpt(m, enable_kid=kid, fused_objective=fused)
        o = to_np(fo.fit(t(tv, dev), t(tj, dev), joint_weights=t(jw, dev), refine_steps=U.STEPS, **U.FIT_KW))
        assert set(o) == {str(k) for k in gfo[f'{case}.keys']}
        assert all(np.isfinite(v).all() for v in o.values())
        for k, v in o.items():
            assert v.shape == gfo[f'{case}.s{U.STEPS}.{k}'].shape, k
        obj = U.objective64(om64, o, tv, tj, jw)
        obj0, obj100 = float(gfo[f'{case}.obj0']), float(gfo[f'{case}.obj100'])
        share = (obj0 - obj) / (obj0 - obj100)
        print(f'[fitter-opt] {case} {"fused" if fused else "unfused"}: {obj * 1e3:.3f} mm (reference {obj0 * 1e3:.3f} '
              f'-> {obj100 * 1e3:.3f} mm), share of the reference\'s improvement {share:.3f}')
        assert obj <= obj0 - 0.5 * (obj0 - obj100), (case, fused, obj, obj0, obj100)


def test_fused_against_unfused_same_start(model_root, gfo, dev):
    """B = 8, 20 steps from one closed-form start (the fixture's targets, joints, weights and kid): both objectives
    (fp64 oracle) are below the start's, and they differ by at most the smaller of the two improvements."""
    from smplfitter_amd.pt import BodyFitterOpt

    m, om64 = get_model(model_root, 'smpl', dev)
    kid, tv, tj, jw = _fixture_inputs(gfo, om64, 'kid.vj', dev)
    a = (t(tv, dev), t(tj, dev))
    obj = {}
    for fused in (True, False):
        fo = BodyFitterOpt(m, enable_kid=kid, fused_objective=fused)
        if 'start' not in obj:  # (the start of a refinement: the closed-form fit without its final adjustment)
            start = to_np(fo.fit(*a, joint_weights=t(jw, dev), final_adjust_rots=False, refine_steps=0, **U.FIT_KW))
            obj['start'] = U.objective64(om64, start, tv, tj, jw)
        o = to_np(fo.fit(*a, joint_weights=t(jw, dev), refine_steps=20, **U.FIT_KW))
        obj[fused] = U.objective64(om64, o, tv, tj, jw)
    gain = {k: obj['start'] - obj[k] for k in (True, False)}
    print(f'[fitter-opt] 20 steps from {obj["start"] * 1e3:.3f} mm: fused {obj[True] * 1e3:.3f} mm, unfused '
          f'{obj[False] * 1e3:.3f} mm')
    assert gain[True] > 0 and gain[False] > 0, obj
    assert abs(obj[True] - obj[False]) <= min(gain.values()), obj


def _noisy_targets(m, B, seed, dev):
    rs = np.random.RandomState(seed)
    f = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)  # noqa: E731
    with torch.no_grad():
        out = m(f(rs.randn(B, 3 * m.num_joints) * 0.5), f(rs.randn(B, 10)), f(rs.randn(B, 3)))
    noise = lambda x: x + f(rs.randn(*x.shape) * U.NOISE_M)  # noqa: E731
    return noise(out['vertices']), noise(out['joints']), f(rs.uniform(0, 2, (B, m.num_joints)))


def test_refinement_deterministic(model_root, dev):
    """Two fused refinements of the same batch (B = 65, 10 steps, joints and kid) give the same bits, and the result
    differs from the start."""
    from smplfitter_amd.pt import BodyFitterOpt

    m, _ = get_model(model_root, 'smpl', dev)
    tv, tj, jw = _noisy_targets(m, 65, 5, dev)
    fo = BodyFitterOpt(m, enable_kid=True)
    a = fo.fit(tv, tj, joint_weights=jw, refine_steps=10, **U.FIT_KW)
    b = fo.fit(tv, tj, joint_weights=jw, refine_steps=10, **U.FIT_KW)
    assert set(a) == {'pose_rotvecs', 'shape_betas', 'trans', 'kid_factor'}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    start = fo.fit(tv, tj, joint_weights=jw, final_adjust_rots=False, refine_steps=0, **U.FIT_KW)
    assert not torch.equal(a['pose_rotvecs'], start['pose_rotvecs'])  # (the refinement ran)


def test_argument_handling(model_root, dev):
    from smplfitter_amd.pt import BodyFitterOpt

    m, _ = get_model(model_root, 'smpl', dev)
    J, V = m.num_joints, m.num_vertices
    tv, tj, jw = _noisy_targets(m, 4, 6, dev)
    fo = BodyFitterOpt(m)
    empty = fo.fit(tv[:0], tj[:0], joint_weights=jw[:0], refine_steps=5)
    closed = fo.fit(tv[:0], tj[:0], joint_weights=jw[:0], refine_steps=0)  # (the closed-form result, whatever it holds)
    assert set(empty) == set(closed) and {'pose_rotvecs', 'shape_betas', 'trans'} <= set(empty)
    assert empty['pose_rotvecs'].shape == (0, 3 * J) and empty['trans'].shape == (0, 3)
    assert empty['shape_betas'].shape[0] == 0
    betas = torch.zeros(4, 10, device=dev)
    for bad in (dict(target_joints=tj[:, :-1]), dict(target_joints=tj[:3]), dict(target_joints=tj, joint_weights=jw[:, :-1]),
                dict(target_joints=tj, joint_weights=jw[..., None]), dict(joint_weights=jw)):
        with pytest.raises(ValueError):
            m._objective_direct(tv, shape_betas=betas, **bad)
    loss, grads = m._objective_direct(torch.zeros(0, V, 3, device=dev), shape_betas=betas[:0],
                                      target_joints=torch.zeros(0, J, 3, device=dev))
    assert loss.shape == (0,) and grads[1].shape == betas[:0].shape
    out = BodyFitterOpt(m, fused_objective=False).fit(tv, tj, joint_weights=jw, refine_steps=2, **U.FIT_KW)
    assert set(out) == {'pose_rotvecs', 'shape_betas', 'trans'}
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
