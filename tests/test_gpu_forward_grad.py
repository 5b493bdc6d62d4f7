"""-m gpu: the backward of BodyModel.forward (smplfit_forward_backward_f32, BodyModel._backward_direct, the autograd
Function and the compiled operator) against the fp64 torch restatement of tests/grad_util.py.

Gate: per gradient tensor, max |ours - fp64| <= GRAD_REL x max |fp64| over the compared rows (sampled rows of large
batches; the rows are independent except through a broadcast trans / kid, which the tests compare in full).
"""

import itertools

import numpy as np
import pytest
import torch

import grad_util
import util
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

GRAD_REL = 2e-4
# name -> (directory under the model root or None: a golden kind, num_betas)
MODELS = {'smpl': (None, 10), 'smplxfat': (None, 10), 'smpl_w6': (None, 10), 'smpl_b300': ('smpl_b300', None),
          'smpl_w12': ('smpl_w12', 10)}
_cache = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def _model(name, model_root, golden, dev):
    if name not in _cache:
        from smplfitter_amd import modelio
        from smplfitter_amd.pt import BodyModel

        d, nb = MODELS[name]
        if d is None:
            g = golden(name)
            m, _ = get_model(model_root, name, g, dev)
            _, md = util.load_md(model_root, name, g)
        else:
            m = BodyModel('smpl', 'neutral', model_root=f'{model_root}/{d}', num_betas=nb, device=dev)
            md = modelio.load_model('smpl', 'neutral', model_root=f'{model_root}/{d}', num_betas=nb)
        _cache[name] = (m, grad_util.Model64(md))
    return _cache[name]


def _inputs(B, J, S, form, seed=0, kid=False):
    rs = np.random.RandomState(seed)
    pose = (rs.randn(B, J * 3) * 0.4).astype(np.float32)
    x = dict(shape_betas=(rs.randn(B, min(S, 16)) * (1.0 if S <= 32 else 0.15)).astype(np.float32),
             trans=rs.randn(B, 3).astype(np.float32))
    if form == 'pose':
        x['pose_rotvecs'] = pose
    elif form in ('rel', 'glob'):
        x[f'{form}_rotmats'] = grad_util.random_rotmats(rs, (B, J)).astype(np.float32)
    if kid:
        x['kid_factor'] = rs.uniform(-0.5, 1.5, B).astype(np.float32)
    return x


def _cot(B, J, V, which, seed=1):
    rs = np.random.RandomState(seed)
    c = dict(vertices=rs.randn(B, V, 3).astype(np.float32), joints=rs.randn(B, J, 3).astype(np.float32),
             orientations=rs.randn(B, J, 3, 3).astype(np.float32))
    return {k: (v if k in which else None) for k, v in c.items()}


def _ours(m, x, cot, dev):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ins = [t(x.get(k)) for k in grad_util.INPUT_NAMES]
    gs = m._backward_direct(*ins, t(cot['joints']), t(cot['orientations']), t(cot['vertices']))
    torch.cuda.synchronize()
    return {k: g.cpu().numpy() for k, g in zip(grad_util.INPUT_NAMES, gs) if g is not None}


def _rows(B):
    return np.arange(B) if B <= 65 else np.unique(np.r_[0, 1, 63, 64, 65, B // 2, B - 2, B - 1])


def _check(m64, x, cot, ours, rows, tag):
    xr = {k: v[rows] for k, v in x.items()}
    cr = {k: (None if v is None else v[rows]) for k, v in cot.items()}
    ref = grad_util.grads(m64, xr, cr, return_vertices=cot['vertices'] is not None)
    worst = 0.0
    for k, r in ref.items():
        o = ours[k][rows]
        scale = max(np.abs(r).max(), 1e-30)
        err = np.abs(o - r).max()
        worst = max(worst, err / scale)
        assert np.all(np.isfinite(o)), (tag, k)
        assert err <= GRAD_REL * scale + 1e-6 * (k == 'shape_betas'), (tag, k, err, scale)
    print(f'[grad] {tag} max rel {worst:.2e}')


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('form', ['pose', 'rel', 'glob', 'none'])
def test_grad_forms(name, form, model_root, golden, dev):
    m, m64 = _model(name, model_root, golden, dev)
    B = 65
    x = _inputs(B, m.num_joints, m.num_betas, form)
    subsets = [w for n in range(4) for w in itertools.combinations(('vertices', 'joints', 'orientations'), n)]
    assert len(subsets) == 8
    for which in subsets:
        cot = _cot(B, m.num_joints, m.num_vertices, which)
        _check(m64, x, cot, _ours(m, x, cot, dev), _rows(B), f'{name} {form} {"+".join(which) or "none"}')


@pytest.mark.parametrize('B', [1, 63, 64, 65, 1001, 4096])
@pytest.mark.parametrize('name', ['smpl', 'smplxfat'])
def test_grad_batches(name, B, model_root, golden, dev):
    m, m64 = _model(name, model_root, golden, dev)
    x = _inputs(B, m.num_joints, m.num_betas, 'pose', seed=B)
    cot = _cot(B, m.num_joints, m.num_vertices, ('vertices', 'joints', 'orientations'), seed=B + 1)
    _check(m64, x, cot, _ours(m, x, cot, dev), _rows(B), f'{name} B={B}')


def test_grad_kid_and_broadcasts(model_root, golden, dev):
    """kid factor per instance and as one element, (1, 3) trans, betas beyond the model's, autograd end to end."""
    m, m64 = _model('smpl', model_root, golden, dev)
    B, J = 9, m.num_joints
    x = _inputs(B, J, 10, 'pose', kid=True)
    cot = _cot(B, J, m.num_vertices, ('vertices', 'joints'))
    _check(m64, x, cot, _ours(m, x, cot, dev), np.arange(B), 'smpl kid')
    rs = np.random.RandomState(5)
    pose = torch.from_numpy(x['pose_rotvecs']).to(dev).requires_grad_()
    betas = torch.from_numpy(rs.randn(B, 12).astype(np.float32)).to(dev).requires_grad_()
    trans = torch.from_numpy(rs.randn(1, 3).astype(np.float32)).to(dev).requires_grad_()
    kid = torch.tensor([0.3], device=dev).requires_grad_()
    out = m(pose, betas, trans, kid)
    cv = torch.from_numpy(cot['vertices']).to(dev)
    cj = torch.from_numpy(cot['joints']).to(dev)
    ((out['vertices'] * cv).sum() + (out['joints'] * cj).sum()).backward()
    assert trans.grad.shape == (1, 3) and kid.grad.shape == (1,) and betas.grad.shape == (B, 12)
    assert torch.all(betas.grad[:, 10:] == 0)
    ref = grad_util.grads(m64, dict(pose_rotvecs=x['pose_rotvecs'], shape_betas=betas.detach().cpu().numpy(),
                                    trans=trans.detach().cpu().numpy(), kid_factor=kid.detach().cpu().numpy()),
                          dict(vertices=cot['vertices'], joints=cot['joints'], orientations=None))
    for k, g in (('pose_rotvecs', pose.grad), ('shape_betas', betas.grad), ('trans', trans.grad),
                 ('kid_factor', kid.grad)):
        r = ref[k]
        assert np.abs(g.cpu().numpy() - r).max() <= GRAD_REL * np.abs(r).max() + 1e-6, k


def test_grad_no_vertices_and_dtype(model_root, golden, dev):
    """return_vertices=False under autograd; fp64 inputs get fp64 gradients; forward under grad == no_grad bitwise."""
    m, m64 = _model('smpl', model_root, golden, dev)
    B, J = 17, m.num_joints
    x = _inputs(B, J, 10, 'rel')
    rel = torch.from_numpy(x['rel_rotmats']).double().to(dev).requires_grad_()
    betas = torch.from_numpy(x['shape_betas']).to(dev).requires_grad_()
    out = m(rel_rotmats=rel, shape_betas=betas, return_vertices=False)
    with torch.no_grad():
        ref_out = m(rel_rotmats=rel, shape_betas=betas, return_vertices=False)
    assert torch.equal(out['joints'], ref_out['joints']) and torch.equal(out['orientations'], ref_out['orientations'])
    cot = _cot(B, J, m.num_vertices, ('joints', 'orientations'))
    gj, go = (torch.from_numpy(cot[k]).to(dev) for k in ('joints', 'orientations'))
    ((out['joints'] * gj).sum() + (out['orientations'] * go).sum()).backward()
    assert rel.grad.dtype == torch.float64
    ref = grad_util.grads(m64, dict(rel_rotmats=x['rel_rotmats'], shape_betas=x['shape_betas']),
                          dict(joints=cot['joints'], orientations=cot['orientations']), return_vertices=False)
    for k, g in (('rel_rotmats', rel.grad), ('shape_betas', betas.grad)):
        assert np.abs(g.cpu().numpy() - ref[k]).max() <= GRAD_REL * np.abs(ref[k]).max(), k
    pv = torch.from_numpy(_inputs(B, J, 10, 'pose')['pose_rotvecs']).to(dev).requires_grad_()
    fw = m(pv, betas, return_vertices=True)
    with torch.no_grad():
        fw0 = m(pv, betas, return_vertices=True)
    assert all(torch.equal(fw[k], fw0[k]) for k in fw0)


def test_grad_deterministic_and_guarded(model_root, golden, dev):
    """Two runs bitwise equal; NaN-filled workspace and outputs; guard regions around every output untouched."""
    from smplfitter_amd import _lib
    import ctypes as C

    m, _ = _model('smpl', model_root, golden, dev)
    B, J, V = 300, m.num_joints, m.num_vertices
    x = _inputs(B, J, 10, 'pose', kid=False)
    cot = _cot(B, J, V, ('vertices', 'joints', 'orientations'))
    a = _ours(m, x, cot, dev)
    b = _ours(m, x, cot, dev)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    h = m._native(dev)
    G = 4096
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    nbytes = h.forward_backward_workspace_bytes(B)
    ws = torch.full((nbytes // 4 + 2 * G,), float('nan'), device=dev)
    outs = {k: torch.full((n + 2 * G,), float('nan'), device=dev)
            for k, n in (('pose', B * J * 3), ('betas', B * 10), ('trans', B * 3))}
    mid = lambda o: o[G:-G].data_ptr()  # noqa: E731
    # a workspace base 256-byte aligned inside the guarded buffer
    base = (ws.data_ptr() + G * 4 + 255) // 256 * 256
    ins = {k: t(v) for k, v in x.items()}
    cts = {k: t(v) for k, v in cot.items()}
    args = _lib.ForwardBackwardArgs(
        pose_rotvecs=ins['pose_rotvecs'].data_ptr(), shape_betas=ins['shape_betas'].data_ptr(), num_betas_given=10,
        batch=B, grad_vertices=cts['vertices'].data_ptr(), grad_joints=cts['joints'].data_ptr(),
        grad_orientations=cts['orientations'].data_ptr(), grad_pose_rotvecs=mid(outs['pose']),
        grad_shape_betas=mid(outs['betas']), grad_trans=mid(outs['trans']), workspace=base, workspace_bytes=nbytes,
        hip_stream=torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().smplfit_forward_backward_f32(h.ptr, C.byref(args)))
    torch.cuda.synchronize()
    for k, o in outs.items():
        assert torch.isnan(o[:G]).all() and torch.isnan(o[-G:]).all(), k
    assert torch.isnan(ws[:G]).all() and torch.isnan(ws[-G:]).all()
    assert np.array_equal(outs['pose'][G:-G].cpu().numpy().reshape(B, J * 3), a['pose_rotvecs'])
    assert np.array_equal(outs['betas'][G:-G].cpu().numpy().reshape(B, 10), a['shape_betas'])
    assert np.array_equal(outs['trans'][G:-G].cpu().numpy().reshape(B, 3), a['trans'])


def test_grad_compiled_matches_eager(model_root, golden, dev):
    m, _ = _model('smpl', model_root, golden, dev)
    B, J = 33, m.num_joints
    x = _inputs(B, J, 10, 'pose')
    cv = torch.from_numpy(_cot(B, J, m.num_vertices, ('vertices',))['vertices']).to(dev)

    def loss(pose, betas, trans):
        o = m(pose, betas, trans)
        return (o['vertices'] * cv).sum() + o['joints'].square().sum()

    def run(fn):
        ps = [torch.from_numpy(x[k]).to(dev).requires_grad_() for k in ('pose_rotvecs', 'shape_betas', 'trans')]
        fn(*ps).backward()
        return [p.grad.clone() for p in ps]

    eager = run(loss)
    comp = run(torch.compile(loss, fullgraph=True))
    for e, c in zip(eager, comp):
        assert torch.equal(e, c)


GOLD_MODELS = {'smpl': 'smpl', 'smplxfat': 'smplxfat', 'smpl_w6': 'smpl_w6', 'smpl_b300': 'smpl_b300'}


@pytest.mark.parametrize('tag', list(GOLD_MODELS))
def test_grad_vs_reference_fixture(tag, model_root, golden, dev):
    """Every case of golden_forward_grad.npz: ours vs the reference's fp64 gradients <= 3 x the reference's own fp32
    error + 1e-6 x max |fp64|."""
    import os.path as osp

    from grad_util import cotangents

    gold = np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'golden_forward_grad.npz'))
    m, _ = _model(tag, model_root, golden, dev)
    cases = sorted({k.split('.')[1] for k in gold.files if k.startswith(tag + '.')})
    assert len(cases) == 9
    for case in cases:
        p = f'{tag}.{case}.'
        x = {k[len(p) + 3:]: gold[k] for k in gold.files if k.startswith(p + 'in.')}
        which = str(gold[p + 'which']).split(',')
        c = cotangents(int(gold[p + 'seed']), 8, m.num_joints, m.num_vertices, which)
        cot = {k: c.get(k) for k in ('vertices', 'joints', 'orientations')}
        ours = _ours(m, x, cot, dev)
        for k, o in ours.items():
            r = gold[p + 'g64.' + k]
            err = np.abs(o - r).max()
            gate = 3 * float(gold[p + 'err32.' + k]) + 1e-6 * np.abs(r).max()
            print(f'[grad] fixture {tag} {case} {k} err {err:.1e} gate {gate:.1e}')
            assert err <= gate, (tag, case, k, err, gate)
