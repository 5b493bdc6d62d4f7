"""The differentiable ``BodyConverter`` on the GPU: ``smplfit_transfer_backward_f32`` against scipy in fp64
and against the forward call (adjoint identity), ``convert_vertices`` under autograd, and the gradients of ``convert`` — a
composition of the existing native adjoints with the new one between them — against the fp64 arbiter of
tests/convert_grad_util.py and the reference's own fp32 gradients (golden_convert_grad.npz)."""

import os.path as osp
import warnings

import numpy as np
import pytest
import torch

import convert_grad_util as cu
import util

pytestmark = pytest.mark.gpu
HERE = osp.dirname(osp.abspath(__file__))
EPS = 2.0 ** -23


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(osp.join(HERE, 'golden', 'golden_convert_grad.npz')))


_models = {}


def get_model(model_root, name, dev):
    from smplfitter_amd.pt import BodyModel

    if name not in _models:
        kind = 'smplx' if name.startswith('smplx') else 'smpl'
        nb = 32 if name == 'smpl_b32' else 10
        mdir = name if name == 'smpl_b32' else util.model_dir(name)
        _models[name] = BodyModel(kind, 'neutral', model_root=f'{model_root}/{mdir}', num_betas=nb, device=dev)
    return _models[name]


_converters = {}


def get_converter(model_root, tag, dev):
    """One converter per direction for the module (DATA_ROOT is read when it is made)."""
    from smplfitter_amd.pt import BodyConverter

    if tag not in _converters:
        a, b = cu.DIRS[tag]
        _converters[tag] = BodyConverter(get_model(model_root, a, dev), get_model(model_root, b, dev))
    return _converters[tag]


_arbiter = {}


def arbiter(model_root, data_root, gold, tag, case):
    """(inputs, cotangents, fp64 results, fp64 gradients) of a fixture case: computed once, shared, never modified."""
    if (tag, case) not in _arbiter:
        x = cu.fixture_inputs(gold, tag)
        cot = cu.cotangents(int(gold[f'{tag}.{case}.seed']), case, x['known_output_pose_rotvecs'].shape[1] // 3)
        _arbiter[tag, case] = (x, cot) + cu.arbiter(model_root, data_root, tag, case, x, cot)
    return _arbiter[tag, case]


def t(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


def to_np(d):
    return {k: v.detach().cpu().numpy() for k, v in d.items()}


def run_case(conv, case, x, cot, dev):
    """``convert`` of a case with its inputs requiring grad -> (results, gradients of sum(cot . results)), numpy."""
    names = cu.grad_names(case)
    ts = {k: t(v, dev, grad=k in names) for k, v in x.items()}
    r = conv.convert(**cu.convert_kwargs(case, ts))
    assert set(r) == set(cot)
    loss = sum((r[k].reshape(c.shape) * t(c, dev)).sum() for k, c in cot.items())
    gs = torch.autograd.grad(loss, [ts[k] for k in names], allow_unused=True)
    assert all(g is not None for g in gs), (case, [n for n, g in zip(names, gs) if g is None])
    return to_np(r), {k: g.cpu().numpy() for k, g in zip(names, gs)}


def awkward_matrix(rs, vin, vout):
    """A (V_out x V_in) CSR matrix a barycentric file does not produce, duplicates kept as separate entries: rows of 0 to 7
    seeded entries in the columns below V_in - 10 (the last ten input vertices stay unused), the last entry of every third
    row repeating its first column, and column 7 with 2000 more entries — one in each of the first 2000 rows, or, with
    fewer rows than that, four in each of the first 500."""
    per_row = 1 if vout >= 2000 else 4
    indptr, indices = [0], []
    for r in range(vout):
        n = rs.randint(0, 8)
        cols = rs.randint(0, vin - 10, size=n).tolist()
        if n > 1 and r % 3 == 0:
            cols[-1] = cols[0]
        if r < 2000 // per_row:
            cols += [7] * per_row
        indices += cols
        indptr.append(len(indices))
    indptr, indices = np.array(indptr, np.int32), np.array(indices, np.int32)
    return indptr, indices, rs.randn(len(indices)).astype(np.float32)


def backward_bound(mt_abs, counts, g):
    """Per element (n_c + 1) 2^-23 (|M|^T |g|)_c: a sequential fp32 sum of n_c products (n_c roundings of the products,
    n_c - 1 of the additions, first order: (2 n_c - 1) / 2 units in the last place of the sum of magnitudes), times 2."""
    return (counts + 1)[None, :, None] * EPS * np.stack([mt_abs @ np.abs(gb) for gb in g.astype(np.float64)])


@pytest.mark.parametrize('negate_x', [False, True])
@pytest.mark.parametrize('vin,vout', [(300, 517), (1000, 20000)])
def test_transfer_backward_matrix_shapes(vin, vout, negate_x, dev):
    """``smplfit_transfer_backward_f32`` on awkward matrices (``awkward_matrix``; the cotangent of the second exceeds the
    LDS and is gathered from global memory), batch 1 and 3 and 0, with and without SMPLFIT_TRANSFER_NEGATE_X, into a
    buffer pre-filled with a sentinel: against scipy's M^T g in fp64 within ``backward_bound``; an input vertex no row
    uses comes back exactly 0."""
    import scipy.sparse as sp

    from smplfitter_amd import _lib

    rs = np.random.RandomState(11)
    indptr, indices, vals = awkward_matrix(rs, vin, vout)
    tr = _lib.Transfer(vin, vout, indptr, indices, vals, negate_x=negate_x)
    counts = np.bincount(indices, minlength=vin)
    # (copies: scipy sums duplicates in place when it converts; its products add them either way)
    m64 = sp.csr_matrix((vals.astype(np.float64), indices.copy(), indptr.copy()), shape=(vout, vin))
    mt, mt_abs = m64.T.tocsr(), abs(m64).T.tocsr()
    assert counts.max() >= 2000 and (counts[-10:] == 0).all() and (np.diff(indptr) == 0).any()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for B in (1, 3):
        g = rs.randn(B, vout, 3).astype(np.float32)
        gd, out = t(g, dev), torch.full((B, vin, 3), 7.0, device=dev)
        tr.backward(gd.data_ptr(), B, out.data_ptr(), stream)
        ours = out.cpu().numpy()
        ref = np.stack([mt @ gb for gb in g.astype(np.float64)])
        if negate_x:
            ref[..., 0] = -ref[..., 0]
        excess = np.abs(ours - ref) - backward_bound(mt_abs, counts, g)
        assert excess.max() <= 0, (B, float(excess.max()))
        assert (ours[:, counts == 0] == 0).all() and not (ours == 7.0).any()
    before = out.clone()
    tr.backward(gd.data_ptr(), 0, out.data_ptr(), stream)  # a batch of 0 enqueues nothing
    assert torch.equal(out, before)
    with pytest.raises(ValueError):
        tr.backward(gd.data_ptr(), -1, out.data_ptr(), stream)


@pytest.mark.parametrize('tag', list(cu.DIRS))
def test_adjoint_identity(tag, dev, data_root_fat):
    """<M x, g> from ``smplfit_transfer_f32`` equals <x, M^T g> from ``smplfit_transfer_backward_f32`` on the synthetic
    transfer matrices, both accumulated in fp64 on the host, within the two calls' rounding bounds summed over all
    elements."""
    from smplfitter_amd import _lib

    m = util.load_transfer_csr(data_root_fat, tag)
    m.sort_indices()
    vout, vin = m.shape
    tr = _lib.Transfer(vin, vout, m.indptr, m.indices, m.data)
    rs = np.random.RandomState(12)
    B = 2
    x, g = rs.randn(B, vin, 3).astype(np.float32), rs.randn(B, vout, 3).astype(np.float32)
    xd, gd = t(x, dev), t(g, dev)
    mx, mtg = torch.full((B, vout, 3), 7.0, device=dev), torch.full((B, vin, 3), 7.0, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    tr.forward(xd.data_ptr(), B, mx.data_ptr(), stream)
    tr.backward(gd.data_ptr(), B, mtg.data_ptr(), stream)
    lhs = float((mx.cpu().numpy().astype(np.float64) * g).sum())
    rhs = float((mtg.cpu().numpy().astype(np.float64) * x).sum())
    m_abs = abs(m.astype(np.float64)).tocsr()
    rows, cols = np.diff(m.indptr), np.bincount(m.indices, minlength=vin)
    fwd = (rows + 1)[None, :, None] * EPS * np.stack([m_abs @ np.abs(xb) for xb in x.astype(np.float64)])
    bound = float((fwd * np.abs(g)).sum() + (backward_bound(m_abs.T.tocsr(), cols, g) * np.abs(x)).sum())
    print(f'[convert-grad] adjoint identity {tag}: <Mx, g> {lhs:.9e} <x, M^T g> {rhs:.9e} diff {abs(lhs - rhs):.2e} bound {bound:.2e}')
    assert abs(lhs - rhs) <= bound


def test_convert_vertices_autograd(model_root, dev, data_root_fat, monkeypatch):
    """``convert_vertices`` of an input that requires grad (before: NotImplementedError): the results have the no-gradient
    call's bits, the gradient the native call's; a float64 input gets a float64 gradient in its own shape; no ``grad_fn``
    without gradients; a same-topology pair is the identity for autograd."""
    from smplfitter_amd.pt import BodyConverter

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    conv = get_converter(model_root, 's2x', dev)
    vout, vin = conv.vertex_converter_csr.shape
    rs = np.random.RandomState(13)
    v0, g0 = rs.randn(3, vin, 3).astype(np.float32), rs.randn(3, vout, 3).astype(np.float32)
    plain = conv.convert_vertices(t(v0, dev))
    assert plain.grad_fn is None and not plain.requires_grad
    v = t(v0, dev, grad=True)
    out = conv.convert_vertices(v)
    assert out.requires_grad and torch.equal(out.detach(), plain)
    out.backward(t(g0, dev))
    native = torch.full((3, vin, 3), 7.0, device=dev)
    conv._transfer(dev).backward(t(g0, dev).data_ptr(), 3, native.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert v.grad.shape == v.shape and v.grad.dtype == torch.float32 and torch.equal(v.grad, native)
    v64 = t(v0.astype(np.float64), dev, grad=True)
    out64 = conv.convert_vertices(v64)
    assert torch.equal(out64.detach(), plain)
    (out64 * t(g0, dev)).sum().backward()  # (the cotangent arrives through a product: not the tensor handed in above)
    assert v64.grad.dtype == torch.float64 and torch.equal(v64.grad, native.double())
    with torch.no_grad():
        quiet = conv.convert_vertices(v)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, plain)
    empty = conv.convert_vertices(torch.zeros((0, vin, 3), device=dev, requires_grad=True))
    assert empty.shape == (0, vout, 3)
    ms = get_model(model_root, 'smpl', dev)
    same = BodyConverter(ms, ms)
    w = t(v0, dev, grad=True)
    assert same.convert_vertices(w) is w


@pytest.mark.parametrize('case', list(cu.CASES))
@pytest.mark.parametrize('tag', list(cu.DIRS))
def test_gradients_against_arbiter(tag, case, model_root, gold, dev, data_root_fat, monkeypatch):
    """Every fixture case in both directions: per tensor max |ours - fp64| <= max(2e-4 max |fp64|, 2 max |reference fp32 -
    fp64|) (the gate of DESIGN.md §17 / §18), and the results within ``util.check_convert``'s gates of the fixture's."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    assert util.csr_digest(util.load_transfer_csr(data_root_fat, tag)) == str(gold[f'{tag}.csr_sha256'])
    x, cot, _, g64 = arbiter(model_root, data_root_fat, gold, tag, case)
    o, grads = run_case(get_converter(model_root, tag, dev), case, x, cot, dev)
    p = f'{tag}.{case}.'
    bad = []
    for k in cu.grad_names(case):
        err, bound = cu.gate(grads[k], g64[k], gold[p + 'g32.' + k])
        print(f'[convert-grad] {tag} {case} {k}: |ours - fp64| {err:.2e} bound {bound:.2e} max |fp64| {np.abs(g64[k]).max():.2e} '
              f'ours vs reference fp32 {np.abs(grads[k] - gold[p + "g32." + k]).max():.2e}')
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, (tag, case, bad)
    # the fixture under the key names check_convert reads (<tag>.<case>.<result>, <tag>.<kshape|kpose>.<name>_in)
    gc = {p + k[len(p) + 4:]: v for k, v in gold.items() if k.startswith(p + 'out.')}
    gc[f'{tag}.kshape.betas_in'], gc[f'{tag}.kpose.pose_in'] = x['known_output_shape_betas'], x['known_output_pose_rotvecs']
    name = cu.DIRS[tag][1]
    om_out = util.O.OracleModel(util.load_md(model_root, name)[1], np.float64, 'smplx' if name.startswith('smplx') else 'smpl')
    util.check_convert(om_out, tag, case, o, gc)


@pytest.mark.parametrize('B', [1, 64, 65])
def test_batch_edges(B, model_root, gold, dev, data_root_fat, monkeypatch):
    """The stage kernels work in blocks of 64 instances: case it1, direction x2s, the two fixture instances tiled to 1, 64
    and 65; every row against the arbiter's gradient of its instance under the gate of ``test_gradients_against_arbiter``
    (the arbiter runs once, at B = 2)."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    tag, case = 'x2s', 'it1'
    x, cot, _, g64 = arbiter(model_root, data_root_fat, gold, tag, case)
    idx = np.arange(B) % cu.B
    _, grads = run_case(get_converter(model_root, tag, dev), case, {k: v[idx] for k, v in x.items()},
                        {k: v[idx] for k, v in cot.items()}, dev)
    for k in cu.grad_names(case):
        g32 = gold[f'{tag}.{case}.g32.{k}']
        assert grads[k].shape == (B,) + g64[k].shape[1:]
        err = float(np.abs(grads[k] - g64[k][idx]).max())
        _, bound = cu.gate(g64[k], g64[k], g32)
        print(f'[convert-grad] batch {B} {k}: |ours - fp64| {err:.2e} bound {bound:.2e}')
        assert err <= bound, (B, k, err, bound)


def test_end_to_end(model_root, gold, dev, data_root_fat, monkeypatch):
    """``convert`` with one input requiring grad: the bits of the same three calls made without gradients, within the
    fused-versus-unfused gates (vertex L2 < 1e-4 m, trans 2e-5) of the fused no-gradient ``convert``; that input gets a
    gradient, ``kid_factor`` — also requiring grad — none; no warning; a second run gives the same bits.  With every
    tensor input requiring grad, the three parameters get gradients and ``kid_factor`` still none."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    tag = 's2x'
    conv = get_converter(model_root, tag, dev)
    assert conv._plan(dev) is not None
    x = cu.fixture_inputs(gold, tag)
    pose, trans = t(x['pose_rotvecs'], dev), t(x['trans'], dev)
    mesh = conv.convert_vertices(conv.body_model_in(pose, t(x['shape_betas'], dev), trans)['vertices'])
    three = conv.fitter.fit(mesh, num_iter=2, beta_regularizer=0.0, final_adjust_rots=False, kid_regularizer=0.0,
                            requested_keys=['pose_rotvecs', 'shape_betas'])
    runs = []
    for _ in range(2):
        betas, kid = t(x['shape_betas'], dev, grad=True), t(x['kid_factor'], dev, grad=True)
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)
            r = conv.convert(pose, betas, trans, kid_factor=kid, num_iter=2)
            assert set(r) == {'pose_rotvecs', 'shape_betas', 'trans', 'kid_factor'}
            assert all(v.grad_fn is not None for v in r.values())
            loss = sum((v * v).sum() for v in r.values())
            g_betas, g_kid = torch.autograd.grad(loss, [betas, kid], allow_unused=True)
        assert g_kid is None and g_betas is not None and g_betas.shape == betas.shape
        assert torch.isfinite(g_betas).all() and g_betas.abs().max().item() > 0
        runs.append((to_np(r), g_betas.cpu().numpy()))
    # who receives a gradient, with every tensor input a leaf that requires grad: the three parameters do, kid_factor —
    # which only selects the kid ridge weight — does not; the results are still the three calls' bits
    leaves = {k: t(x[k], dev, grad=True) for k in cu.INPUTS + ('kid_factor',)}
    r = conv.convert(**leaves, num_iter=2)
    loss = sum((v * v).sum() for v in r.values())
    gs = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)))
    assert gs['kid_factor'] is None
    for k in cu.INPUTS:
        assert gs[k] is not None and gs[k].shape == leaves[k].shape and gs[k].dtype == leaves[k].dtype, k
        assert torch.isfinite(gs[k]).all() and gs[k].abs().max().item() > 0, k
    for k, v in to_np(r).items():
        assert np.array_equal(v, runs[0][0][k]), k
    for k, v in runs[0][0].items():
        assert np.array_equal(v, three[k].cpu().numpy()), k
        assert np.array_equal(v, runs[1][0][k]), k
    assert np.array_equal(runs[0][1], runs[1][1])
    # against the fused call, on the branch test_convert_fused_matches_unfused compares (no kid_factor: with the kid ridge
    # at 0 beside a beta ridge of 0 only the mesh is pinned, see util.check_convert)
    fused = to_np(conv.convert(pose, t(x['shape_betas'], dev), trans, num_iter=2))
    a = conv.convert(pose, t(x['shape_betas'], dev, grad=True), trans, num_iter=2)
    assert all(v.grad_fn is not None for v in a.values())
    a = to_np(a)
    name = cu.DIRS[tag][1]
    om = util.O.OracleModel(util.load_md(model_root, name)[1], np.float64, 'smplx')
    assert util.vertex_l2(om, a, fused) < 1e-4
    assert np.abs(a['trans'] - fused['trans']).max() < 2e-5


def test_broadcast_trans(model_root, gold, dev, data_root_fat, monkeypatch):
    """A ``trans`` of shape (1, 3) applies to every instance and gets the summed gradient: against the per-row gradients of
    the same call with that row repeated (B = 2), added in fp64.  The broadcast gradient is the fp32 sum of the same two
    rows: one rounding, gated at 2^-23 (|g_0| + |g_1|) per component; the results of the two calls have the same bits."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    tag, case = 'x2s', 'it1'
    conv = get_converter(model_root, tag, dev)
    x = cu.fixture_inputs(gold, tag)
    cot = cu.cotangents(int(gold[f'{tag}.{case}.seed']), case, x['known_output_pose_rotvecs'].shape[1] // 3)
    res = {}
    for name, tr in (('broadcast', x['trans'][:1]), ('rows', np.repeat(x['trans'][:1], cu.B, 0))):
        pose, betas, trans = t(x['pose_rotvecs'], dev), t(x['shape_betas'], dev), t(tr, dev, grad=True)
        r = conv.convert(pose, betas, trans, num_iter=1)
        loss = sum((r[k] * t(c, dev)).sum() for k, c in cot.items())
        (g,) = torch.autograd.grad(loss, [trans])
        assert g.shape == trans.shape and g.dtype == torch.float32
        res[name] = to_np(r), g.cpu().numpy().astype(np.float64)
    for k, v in res['rows'][0].items():
        assert np.array_equal(v, res['broadcast'][0][k]), k
    g1, g2 = res['broadcast'][1], res['rows'][1]
    assert g1.shape == (1, 3) and g2.shape == (cu.B, 3) and np.abs(g2).min() > 0
    err, bound = np.abs(g1[0] - g2.sum(0)), EPS * np.abs(g2).sum(0)
    print(f'[convert-grad] broadcast trans: gradient {g1[0]}, sum of rows {g2.sum(0)}, |difference| {err}, bound {bound}')
    assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize('tag', list(cu.DIRS))
def test_direction_check(tag, model_root, gold, dev, data_root_fat, monkeypatch):
    """As tests/test_autograd_fit.py checks the fit: the autograd directional derivative of case it2 against central
    differences (eps 1e-2) of the fused no-gradient ``convert``, within 5 %."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    case = 'it2'
    conv = get_converter(model_root, tag, dev)
    assert conv._plan(dev) is not None
    x = cu.fixture_inputs(gold, tag)
    cot = cu.cotangents(int(gold[f'{tag}.{case}.seed']), case, x['known_output_pose_rotvecs'].shape[1] // 3)
    _, grads = run_case(conv, case, x, cot, dev)
    rs = np.random.RandomState(14)
    d = {k: rs.randn(*x[k].shape) for k in cu.INPUTS}
    norm = np.sqrt(sum((v * v).sum() for v in d.values()))
    d = {k: (v / norm).astype(np.float32) for k, v in d.items()}
    ag = sum(float((grads[k].astype(np.float64) * d[k]).sum()) for k in cu.INPUTS)

    def loss(sign, eps=1e-2):
        with torch.no_grad():
            r = to_np(conv.convert(*(t(x[k] + np.float32(sign * eps) * d[k], dev) for k in cu.INPUTS), num_iter=2))
        return sum(float((r[k].astype(np.float64) * c).sum()) for k, c in cot.items())

    fd = (loss(1) - loss(-1)) / (2 * 1e-2)
    print(f'[convert-grad] direction check {tag}: autograd {ag:.6e} central differences {fd:.6e}')
    assert abs(ag - fd) / max(abs(ag), abs(fd), 1e-3) < 5e-2, (ag, fd)


def test_more_than_17_unknowns(model_root, gold, dev):
    """An output model with more than 17 shape unknowns (32 betas + kid), same topology (the transfer is the identity): the
    default branch takes ``fit``'s PyTorch route, with its warning, and gives finite non-zero gradients; the known-pose
    branch raises what ``fit_with_known_pose`` raises."""
    from smplfitter_amd.pt import BodyConverter

    ms, mb = get_model(model_root, 'smpl', dev), get_model(model_root, 'smpl_b32', dev)
    conv = BodyConverter(ms, mb)
    assert conv.vertex_converter_csr is None
    x = cu.fixture_inputs(gold, 's2x')
    ts = {k: t(x[k], dev, grad=True) for k in cu.INPUTS}
    with pytest.warns(RuntimeWarning, match='PyTorch'):
        r = conv.convert(**ts)
    assert r['shape_betas'].shape == (cu.B, 32)
    loss = sum((v * v).sum() for v in r.values())
    for g in torch.autograd.grad(loss, list(ts.values())):
        assert torch.isfinite(g).all() and g.abs().max().item() > 0
    with pytest.raises(NotImplementedError, match='17 shape unknowns'):
        conv.convert(**ts, known_output_pose_rotvecs=t(x['pose_rotvecs'], dev))


def test_empty_batch(model_root, dev, data_root_fat, monkeypatch):
    """An empty batch whose inputs require grad: empty results, no error."""
    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    conv = get_converter(model_root, 'x2s', dev)
    mi, mo = conv.body_model_in, conv.body_model_out
    z = lambda *s: torch.zeros(s, device=dev, requires_grad=True)  # noqa: E731
    r = conv.convert(z(0, 3 * mi.num_joints), z(0, 10), z(0, 3))
    assert {k: tuple(v.shape) for k, v in r.items()} == dict(pose_rotvecs=(0, 3 * mo.num_joints), shape_betas=(0, 10),
                                                              trans=(0, 3))
