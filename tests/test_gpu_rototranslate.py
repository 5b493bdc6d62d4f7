"""-m gpu: BodyModel.rototranslate on the device (smplfit_rototranslate_f32 and its backward, the autograd Function and
the compiled operators) against the fp64 restatement of tests/rototranslate_util.py.

Gates: FLOOR_MARGIN (5) x the reference's own fp32-against-fp64 floor recorded per case in
tests/golden/golden_rototranslate.npz — the root compared as a rotation matrix, new_trans relative to
max(1, |new_trans|_inf), a gradient relative to its max abs.  A gradient summed over B rows (an input shared across the
batch) is gated by B x (5 x floor + B 2^-24) x max |per-row fp64 gradient|: the sum of the per-row gates plus the fp32
rounding of a B-term sum.
"""

import ctypes as C

import numpy as np
import pytest
import torch

import rototranslate_util as U
import util

pytestmark = pytest.mark.gpu

EDGES = (1, 63, 64, 65, 257, 1001)
_cache = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gold():
    return np.load(U.GOLDEN)


def _model(tag, model_root, dev):
    if tag not in _cache:
        from smplfitter_amd.pt import BodyModel

        kind, d, nb = U.MODELS[tag]
        m = BodyModel(kind, 'neutral', model_root=f'{model_root}/{d}', num_betas=nb, device=dev)
        _cache[tag] = (m, U.load_md(tag, model_root))
    return _cache[tag]


def _t(x, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in x.items()}


def _call(m, x, post, dev):
    xt = _t(x, dev)
    p, tr = m.rototranslate(xt['R'], xt.get('t'), xt['pose_rotvecs'], xt['shape_betas'], xt['trans'],
                            xt.get('kid_factor'), post_translate=post)
    return p.cpu().numpy(), tr.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_parity(gold, tag, case, md, x, post, new_pose, new_trans):
    root64, trans64 = U.forward64(md, x['R'], x.get('t'), x['pose_rotvecs'], x['shape_betas'], x['trans'],
                                  x.get('kid_factor'), post)
    e_root, e_trans = U.root_error(new_pose, root64), U.trans_error(new_trans, trans64)
    f_root, f_trans = float(gold[f'{tag}.{case}.floor.root']), float(gold[f'{tag}.{case}.floor.trans'])
    print(f'{tag} {case}: root {e_root:.2e} (floor {f_root:.2e})  trans {e_trans:.2e} (floor {f_trans:.2e})')
    assert e_root <= U.FLOOR_MARGIN * f_root, (tag, case)
    assert e_trans <= U.FLOOR_MARGIN * f_trans, (tag, case)
    assert np.array_equal(_bits(new_pose[:, 3:]), _bits(x['pose_rotvecs'][:, 3:])), (tag, case)


# ---- parity ------------------------------------------------------------------------------------
def test_unbatched_signature(gold, model_root, dev):
    """Every fixture case of smpl through the reference's signature, one row per call."""
    m, md = _model('smpl', model_root, dev)
    for case in U.cases_of('smpl'):
        x, post = U.case_inputs(gold, 'smpl', case)
        xt = _t(x, dev)
        poses, transs = [], []
        for i in range(U.ROWS):
            kid = xt['kid_factor'][i:i + 1] if 'kid_factor' in xt else None
            p, tr = m.rototranslate(xt['R'][i], xt['t'][i] if 't' in xt else None, xt['pose_rotvecs'][i],
                                    xt['shape_betas'][i], xt['trans'][i], kid, post_translate=post)
            assert p.shape == (72,) and tr.shape == (3,)
            poses.append(p)
            transs.append(tr)
        _check_parity(gold, 'smpl', case, md, x, post, torch.stack(poses).cpu().numpy(),
                      torch.stack(transs).cpu().numpy())


@pytest.mark.parametrize('tag', list(U.MODELS))
def test_batched_per_instance(gold, tag, model_root, dev):
    m, md = _model(tag, model_root, dev)
    for case in U.cases_of(tag):
        x, post = U.case_inputs(gold, tag, case)
        new_pose, new_trans = _call(m, x, post, dev)
        _check_parity(gold, tag, case, md, x, post, new_pose, new_trans)


# ---- batch edges -------------------------------------------------------------------------------
def _tiled(x, B):
    return {k: np.ascontiguousarray(v[np.arange(B) % len(v)]) for k, v in x.items()}


@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_batch_edges(gold, tag, model_root, dev):
    """The fixture's rows tiled to batches with a ragged last wave / workgroup: every row has the bits of the same row
    in the batch of 16.  (63 and 1001 rows of 3J = 165 floats end on a run that is no multiple of four floats: the
    copy's dword tail behind its 16-byte part.)"""
    m, md = _model(tag, model_root, dev)
    for case in ('post_kid', 'pre_nokid'):
        x, post = U.case_inputs(gold, tag, case)
        p16, t16 = _call(m, x, post, dev)
        for B in EDGES:
            xb = _tiled(x, B)
            p, tr = _call(m, xb, post, dev)
            idx = np.arange(B) % U.ROWS
            assert np.array_equal(_bits(p), _bits(p16[idx])), (case, B)
            assert np.array_equal(_bits(tr), _bits(t16[idx])), (case, B)


@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_shared_inputs_have_the_expanded_bits(gold, tag, model_root, dev):
    m, md = _model(tag, model_root, dev)
    x, post = U.case_inputs(gold, tag, 'pre_kid')
    for B in (16, 65, 257):
        xb = _tiled(x, B)
        row = lambda k: np.ascontiguousarray(np.broadcast_to(xb[k][3], xb[k].shape))  # noqa: E731
        expanded = dict(xb, R=row('R'), t=row('t'), shape_betas=row('shape_betas'), kid_factor=row('kid_factor'))
        pe, te = _call(m, expanded, post, dev)
        for shared in (dict(expanded, R=xb['R'][3], t=xb['t'][3]),
                       dict(expanded, shape_betas=xb['shape_betas'][3]),
                       dict(expanded, kid_factor=xb['kid_factor'][3:4]),
                       dict(expanded, R=xb['R'][3], t=xb['t'][3], shape_betas=xb['shape_betas'][3])):
            p, tr = _call(m, shared, post, dev)
            assert np.array_equal(_bits(p), _bits(pe)) and np.array_equal(_bits(tr), _bits(te)), B
    # a scalar kid_factor
    xt = _t(expanded, dev)
    p, tr = m.rototranslate(xt['R'], xt['t'], xt['pose_rotvecs'], xt['shape_betas'], xt['trans'],
                            float(xb['kid_factor'][3]), post_translate=post)
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(pe))


def test_empty_batch_and_shape_errors(gold, model_root, dev):
    m, md = _model('smpl', model_root, dev)
    x, post = U.case_inputs(gold, 'smpl', 'post_kid')
    xt = _t(x, dev)
    p, tr = m.rototranslate(xt['R'][:0], xt['t'][:0], xt['pose_rotvecs'][:0], xt['shape_betas'][:0], xt['trans'][:0],
                            xt['kid_factor'][:0])
    assert p.shape == (0, 72) and tr.shape == (0, 3) and p.device == dev
    p, tr = m.rototranslate(xt['R'][0], None, xt['pose_rotvecs'][:0], xt['shape_betas'][0], xt['trans'][:0])
    assert p.shape == (0, 72) and tr.shape == (0, 3)
    a = (xt['R'], xt['t'], xt['pose_rotvecs'], xt['shape_betas'], xt['trans'], xt['kid_factor'])
    bad = [
        (0, xt['R'][:5]), (0, xt['R'][0, :2]), (1, xt['t'][:5]), (1, xt['t'][0, :2]), (2, xt['pose_rotvecs'][:, :71]),
        (3, xt['shape_betas'][:5]), (3, torch.zeros(16, 11, device=dev)), (4, xt['trans'][:5]), (4, xt['trans'][0]),
        (5, xt['kid_factor'][:5]),
    ]
    for i, v in bad:
        with pytest.raises(ValueError):
            m.rototranslate(*[v if k == i else a[k] for k in range(6)])
    with pytest.raises(ValueError):  # unbatched pose with a batch of R
        m.rototranslate(xt['R'], None, xt['pose_rotvecs'][0], xt['shape_betas'][0], xt['trans'][0])
    with pytest.raises(RuntimeError, match='There is no CPU path'):
        m.rototranslate(xt['R'].cpu(), xt['t'], xt['pose_rotvecs'], xt['shape_betas'], xt['trans'])


def _abi_args(m, xt, post, new_pose, new_trans, dev, per=True, **over):
    from smplfitter_amd import _lib

    f = dict(R=xt['R'].data_ptr(), R_per_instance=int(per), t=xt['t'].data_ptr(), t_per_instance=int(per),
             pose_rotvecs=xt['pose_rotvecs'].data_ptr(), shape_betas=xt['shape_betas'].data_ptr(),
             num_betas_given=xt['shape_betas'].shape[1], trans=xt['trans'].data_ptr(),
             kid_factor=xt['kid_factor'].data_ptr() if 'kid_factor' in xt else None, post_translate=int(post),
             batch=xt['pose_rotvecs'].shape[0], new_pose_rotvecs=new_pose.data_ptr(), new_trans=new_trans.data_ptr(),
             hip_stream=torch.cuda.current_stream(dev).cuda_stream)
    f.update(over)
    return _lib.RototranslateArgs(**f)


@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_in_place_and_unaligned(gold, tag, model_root, dev):
    """The C-ABI call with new_pose_rotvecs == pose_rotvecs (and new_trans == trans): the bits of the out-of-place
    call; and the out-of-place call on arrays whose base is only 4-byte aligned (the dword form of the copy)."""
    from smplfitter_amd import _lib

    m, md = _model(tag, model_root, dev)
    x, post = U.case_inputs(gold, tag, 'post_kid')
    lib, h = _lib.load(), m._native(dev, kid=True)
    for B in (16, 257):
        xt = _t(_tiled(x, B), dev)
        p_ref, t_ref = m.rototranslate(xt['R'], xt['t'], xt['pose_rotvecs'], xt['shape_betas'], xt['trans'],
                                       xt['kid_factor'], post_translate=post)
        pose, trans = xt['pose_rotvecs'].clone(), xt['trans'].clone()
        xi = dict(xt, pose_rotvecs=pose, trans=trans)
        _lib.check(lib.smplfit_rototranslate_f32(h.ptr, C.byref(_abi_args(m, xi, post, pose, trans, dev))))
        torch.cuda.synchronize()
        assert torch.equal(pose, p_ref) and torch.equal(trans, t_ref), B
        # base pointers off by one float
        J3 = pose.shape[1]
        src = torch.zeros(B * J3 + 1, device=dev)
        src[1:] = xt['pose_rotvecs'].reshape(-1)
        dst = torch.full((B * J3 + 3,), 7.0, device=dev)
        out_t = torch.empty_like(trans)
        xu = dict(xt, pose_rotvecs=src[1:].view(B, J3))
        _lib.check(lib.smplfit_rototranslate_f32(h.ptr, C.byref(_abi_args(m, xu, post, dst[1:], out_t, dev))))
        torch.cuda.synchronize()
        assert torch.equal(dst[1:-2].view(B, J3), p_ref) and torch.equal(out_t, t_ref), B
        assert dst[0] == 7.0 and (dst[-2:] == 7.0).all()  # nothing outside the (B, 3J) rows is written


def test_refused_calls_leave_outputs_untouched(gold, model_root, dev):
    from smplfitter_amd import _lib

    m, md = _model('smpl', model_root, dev)
    x, post = U.case_inputs(gold, 'smpl', 'post_kid')
    xt = _t(x, dev)
    lib, h_kid, h = _lib.load(), m._native(dev, kid=True), m._native(dev, kid=False)
    new_pose, new_trans = torch.full((U.ROWS, 72), 3.0, device=dev), torch.full((U.ROWS, 3), 3.0, device=dev)
    g = {k: torch.full(s, 3.0, device=dev) for k, s in dict(
        grad_R=(U.ROWS, 9), grad_t=(U.ROWS, 3), grad_pose_rotvecs=(U.ROWS, 72), grad_shape_betas=(U.ROWS, 10),
        grad_trans=(U.ROWS, 3), grad_kid_factor=(U.ROWS,)).items()}
    refused = [(h_kid, dict(R=None)), (h_kid, dict(pose_rotvecs=None)), (h_kid, dict(trans=None)),
               (h_kid, dict(num_betas_given=11)), (h, dict()), (h_kid, dict(batch=-1)), (None, dict())]
    for handle, over in refused:
        args = _abi_args(m, xt, post, new_pose, new_trans, dev, **over)
        assert lib.smplfit_rototranslate_f32(handle.ptr if handle else None, C.byref(args)) == _lib.SMPLFIT_ERR_BAD_ARG, over
        fields = {f[0]: getattr(args, f[0]) for f in _lib.RototranslateBackwardArgs._fields_ if hasattr(args, f[0])}
        bargs = _lib.RototranslateBackwardArgs(**fields, grad_new_trans=xt['trans'].data_ptr(),
                                               **{k: v.data_ptr() for k, v in g.items()})
        assert lib.smplfit_rototranslate_backward_f32(handle.ptr if handle else None, C.byref(bargs)) == _lib.SMPLFIT_ERR_BAD_ARG, over
    for o in (dict(new_pose_rotvecs=None), dict(new_trans=None)):
        args = _abi_args(m, xt, post, new_pose, new_trans, dev)
        setattr(args, *next(iter(o.items())))
        assert lib.smplfit_rototranslate_f32(h_kid.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_BAD_ARG
    assert lib.smplfit_rototranslate_f32(h_kid.ptr, None) == _lib.SMPLFIT_ERR_BAD_ARG
    # an empty batch is a call that enqueues nothing
    assert lib.smplfit_rototranslate_f32(h_kid.ptr, C.byref(_abi_args(m, xt, post, new_pose, new_trans, dev, batch=0))) == 0
    torch.cuda.synchronize()
    assert (new_pose == 3.0).all() and (new_trans == 3.0).all()
    assert all((v == 3.0).all() for v in g.values())


# ---- the defining identity ---------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_identity_through_the_forward(gold, tag, model_root, dev):
    """forward(new_pose, betas, new_trans, kid) = R forward(pose, betas, trans, kid) + t (or R (... - t)), both through
    the HIP forward: the error of our parameters against the fp64 oracle mesh transformed in fp64 is within 5 x that
    of the reference's parameters pushed through the same forward."""
    m, md = _model(tag, model_root, dev)
    om64, _ = util.make_oracle(md, U.MODELS[tag][0], np.float64)
    for case in ('post_kid', 'pre_nokid'):
        x, post = U.case_inputs(gold, tag, case)
        kid = x.get('kid_factor')
        v64 = util.forward64(om64, x['pose_rotvecs'], x['shape_betas'], x['trans'], kid)['vertices']
        R, t = x['R'].astype(np.float64), x['t'].astype(np.float64)
        want = np.einsum('bij,bvj->bvi', R, v64) + t[:, None] if post else np.einsum('bij,bvj->bvi', R, v64 - t[:, None])
        ours = _call(m, x, post, dev)
        ref_pose = x['pose_rotvecs'].copy()
        ref_pose[:, :3] = gold[f'{tag}.{case}.ref.new_root']
        errs = []
        for new_pose, new_trans in (ours, (ref_pose, gold[f'{tag}.{case}.ref.new_trans'])):
            a = _t(dict(p=new_pose, b=x['shape_betas'], t=new_trans), dev)
            v = m(a['p'], a['b'], a['t'], None if kid is None else torch.from_numpy(kid).to(dev))['vertices']
            errs.append(float(np.linalg.norm(v.cpu().numpy().astype(np.float64) - want, axis=-1).max()))
        e_ours, e_ref = errs
        print(f'{tag} {case}: e_ours {e_ours:.2e} e_ref {e_ref:.2e}')
        assert e_ours <= U.FLOOR_MARGIN * e_ref, (tag, case)


# ---- gradients ---------------------------------------------------------------------------------
def _autograd(m, x, cp, ct, post, dev, rows=None):
    """autograd.grad of <cp, new_pose> + <ct, new_trans> through the public method: name -> numpy."""
    xt = {k: v.requires_grad_() for k, v in _t(x, dev).items()}
    c = _t(dict(p=cp, t=ct), dev)
    p, tr = m.rototranslate(xt['R'], xt.get('t'), xt['pose_rotvecs'], xt['shape_betas'], xt['trans'],
                            xt.get('kid_factor'), post_translate=post)
    assert p.grad_fn is not None and tr.grad_fn is not None
    names = list(xt)
    gs = torch.autograd.grad((p * c['p']).sum() + (tr * c['t']).sum(), [xt[k] for k in names])
    return {k: g.cpu().numpy() for k, g in zip(names, gs)}


@pytest.mark.parametrize('case', list(U.GRAD_CASES))
@pytest.mark.parametrize('tag', list(U.MODELS))
def test_gradients_batched(gold, tag, case, model_root, dev):
    m, md = _model(tag, model_root, dev)
    x, post = U.case_inputs(gold, tag, case, grad=True)
    cp, ct = gold[f'{tag}.grad.cot.pose'], gold[f'{tag}.grad.cot.trans']
    g = _autograd(m, x, cp, ct, post, dev)
    g64 = U.grads64(md, x, cp, ct, post)
    assert set(g) == set(g64) == set(x)
    for k in g64:
        assert g[k].shape == x[k].shape
        e, floor = U.grad_error(g[k], g64[k]), float(gold[f'{tag}.grad.{case}.gfloor.{k}'])
        print(f'{tag} {case} {k}: {e:.2e} (floor {floor:.2e})')
        assert e <= U.FLOOR_MARGIN * floor, (tag, case, k)
    assert np.array_equal(_bits(g['pose_rotvecs'][:, 3:]), _bits(cp[:, 3:]))


def test_gradients_unbatched(gold, model_root, dev):
    m, md = _model('smpl', model_root, dev)
    for case in U.GRAD_CASES:
        x, post = U.case_inputs(gold, 'smpl', case, grad=True)
        cp, ct = gold['smpl.grad.cot.pose'], gold['smpl.grad.cot.trans']
        g64 = U.grads64(md, x, cp, ct, post)
        rows = []
        for i in range(U.GRAD_ROWS):
            xi = {k: (v[i:i + 1] if k == 'kid_factor' else v[i]) for k, v in x.items()}
            rows.append(_autograd(m, xi, cp[i], ct[i], post, dev))
        for k in g64:
            g = np.stack([r[k].reshape(g64[k].shape[1:]) for r in rows])
            e, floor = U.grad_error(g, g64[k]), float(gold[f'smpl.grad.{case}.gfloor.{k}'])
            print(f'smpl {case} {k}: {e:.2e} (floor {floor:.2e})')
            assert e <= U.FLOOR_MARGIN * floor, (case, k)


@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_gradients_of_shared_inputs_are_row_sums(gold, tag, model_root, dev):
    """R (3, 3), t (3,), betas (n,) and kid (1,) shared by the batch: each gets the sum of the per-row gradients of the
    same values expanded (module docstring for the gate)."""
    m, md = _model(tag, model_root, dev)
    x, post = U.case_inputs(gold, tag, 'post_kid', grad=True)
    cp, ct = gold[f'{tag}.grad.cot.pose'], gold[f'{tag}.grad.cot.trans']
    B = U.GRAD_ROWS
    shared = ('R', 't', 'shape_betas', 'kid_factor')
    expanded = dict(x, **{k: np.ascontiguousarray(np.broadcast_to(x[k][0], x[k].shape)) for k in shared})
    g64 = U.grads64(md, expanded, cp, ct, post)
    g = _autograd(m, dict(expanded, **{k: (x[k][:1] if k == 'kid_factor' else x[k][0]) for k in shared}), cp, ct, post, dev)
    for k in g64:
        floor = float(gold[f'{tag}.grad.post_kid.gfloor.{k}'])
        if k in shared:
            assert g[k].shape == ((1,) if k == 'kid_factor' else x[k].shape[1:])
            err = float(np.abs(g[k].reshape(g64[k].shape[1:]) - g64[k].sum(0)).max())
            gate = B * (U.FLOOR_MARGIN * floor + B * 2.0 ** -24) * float(np.abs(g64[k]).max())
        else:
            err, gate = U.grad_error(g[k], g64[k]), U.FLOOR_MARGIN * floor
        print(f'{tag} {k}: {err:.2e} (gate {gate:.2e})')
        assert err <= gate, (tag, k)


# ---- plumbing ----------------------------------------------------------------------------------
def test_compile_and_gradients_through_the_graph(gold, model_root, dev):
    m, md = _model('smpl', model_root, dev)
    x, post = U.case_inputs(gold, 'smpl', 'post_kid', grad=True)
    cv = torch.from_numpy(np.random.RandomState(5).randn(U.GRAD_ROWS, m.num_vertices, 3).astype(np.float32)).to(dev)

    def loss(R, t, pose, betas, trans, kid):
        p, tr = m.rototranslate(R, t, pose, betas, trans, kid, post_translate=post)
        return (m(p, betas, tr, kid)['vertices'] * cv).sum()

    def run(fn):
        xt = _t(x, dev)
        ps = [xt[k].requires_grad_() for k in U.INPUTS]
        out = fn(*ps)
        out.backward()
        return [out.detach()] + [p.grad.clone() for p in ps]

    eager = run(loss)
    comp = run(torch.compile(loss, backend='aot_eager', fullgraph=True))
    for e, c in zip(eager, comp):
        assert torch.equal(e, c)
    assert all(float(g.abs().max()) > 0 for g in eager[1:])


def test_graph_capture(gold, model_root, dev):
    m, md = _model('smplx', model_root, dev)
    x, post = U.case_inputs(gold, 'smplx', 'pre_kid')
    xa, xb = _t(_tiled(x, 65), dev), _t({k: v[::-1] for k, v in _tiled(x, 65).items()}, dev)
    call = lambda a: m.rototranslate(a['R'], a['t'], a['pose_rotvecs'], a['shape_betas'], a['trans'],  # noqa: E731
                                     a['kid_factor'], post_translate=post)
    buf = {k: v.clone() for k, v in xa.items()}
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # warm-up outside the capture (the handle is made on first use)
        call(buf)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(buf)
    for k in buf:
        buf[k].copy_(xb[k])
    graph.replay()
    torch.cuda.synchronize()
    eager = call(xb)
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    assert not torch.equal(eager[0], call(xa)[0])
