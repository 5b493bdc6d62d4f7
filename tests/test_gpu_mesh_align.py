"""-m gpu: the aligned errors — ``BodyModel.mesh_error(align=..., align_on=..., vertex_weights=...,
joint_weights=...)`` (smplfit_mesh_error_aligned_f32) and ``smplfitter_amd.pt.align_points`` (smplfit_align_points_f32).

Inputs: parameters ``util.forward_inputs`` (row ``util.FWD_FAR`` ~1000 m away); targets the same bodies at a perturbed
pose under a seeded similarity about the row's own translation — scale 0.7 .. 1.4, a random rotation, a shift of a few
metres, 2 mm of noise —, so the far row's target stays ~1000 m away; one family of cases mirrors the targets in x.

Arbiter: ``util.forward64`` at the fp32 parameters, then the table of §24 in fp64 (tests/align_util.py).  Every tested
row has cond = (sigma_2 + d sigma_3) / sigma_1 >= 0.05 in the arbiter, asserted on the arbiter's own numbers.

Gates (``check``):
  errors, per element   |ours - ref_e| <= C g,  C = 2,  g = ``error_gate`` of tests/test_gpu_fit_recon.py with the larger
                        of the point's aligned-model and target coordinates;
  transforms            by their effect: the returned transform applied in fp64 to the fp64 mesh gives errors inside
                        the same gate; |R^T R - I|_max <= 1e-6 and det R > 0;
  means                 the weighted mean of the per-element gates plus one ulp32 of the result.
Each case prints its worst ratio to g as an ``[align]`` line before it asserts.  Observed on one MI355X over all cases:
errors at most 0.71 g (SMPL-X-fat; SMPL 0.49 g, of which 0.41 g is the unaligned step's own), the transforms' effect at
most 0.45 g, means at most 0.03 g, ``align_points`` on exact inputs 0.04 g (DESIGN.md §24 has the table)."""

import ctypes as C

import numpy as np
import pytest
import torch

import align_util as A
import util
from test_gpu_fit_recon import error_gate
from test_gpu_forward import _model, _ref, _slice

pytestmark = pytest.mark.gpu

GATE_C = 2.0
COND_MIN = 0.05
BMAX = {'smpl': 129, 'smplxfat': 67, 'smpl1024': 67, 'smpl_b32': 5, 'smpl_w12': 5}
SOLVED = ('translation', 'rigid', 'similarity')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


_cache = {}


def _rotation(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q * np.sign(np.linalg.det(q))


def case_data(name, om, form='pose', mirrored=False, seed=3):
    """Everything a case needs of one model, computed once and never written to: the Ref64 of the parameters (its .dev the
    device inputs), the fp64 mesh and joints of all BMAX rows, the fp32 targets and weights (numpy and device)."""
    key = (name, form, mirrored, seed)
    if key in _cache:
        return _cache[key]
    B = BMAX[name]
    r = _ref(name, om, B, form)
    rows = r.rows(np.arange(B))
    rs = np.random.RandomState(seed + (100 if mirrored else 0))
    p = {k: v.cpu().numpy() for k, v in r.dev.items()}
    pert = dict(p, pose_rotvecs=(p['pose_rotvecs'] + rs.randn(*p['pose_rotvecs'].shape) * 0.05).astype(np.float32))
    other = util.forward64(om, **pert)
    centre = p['trans'].astype(np.float64)[:, None]
    tgt = {}
    s, shift = rs.uniform(0.7, 1.4, B), rs.randn(B, 3) * 3
    R = np.stack([_rotation(rs) for _ in range(B)])
    for k in ('vertices', 'joints'):
        q = other[k] - centre
        if mirrored:
            q = q * (-1.0, 1.0, 1.0)
        y = s[:, None, None] * np.einsum('brc,bnc->bnr', R, q) + centre + shift[:, None] + rs.randn(*q.shape) * 0.002
        tgt[k] = y.astype(np.float32)
    V, J = rows['vertices'].shape[1], rows['joints'].shape[1]
    w = dict(vertices=rs.uniform(0.0, 2.0, (B, V)).astype(np.float32), joints=rs.uniform(0.1, 2.0, (B, J)).astype(np.float32))
    w['vertices'][:, ::7] = 0.0  # (zero weights inside a row are ordinary)
    t = lambda a: torch.from_numpy(a).to('cuda:0')  # noqa: E731
    d = dict(ref=r, rows=rows, tgt=tgt, w=w, tgt_dev={k: t(v) for k, v in tgt.items()}, w_dev={k: t(v) for k, v in w.items()})
    _cache[key] = d
    return d


def arbiter(d, B, align, align_on, weighted, joints):
    """The fp64 transforms, errors and means of a case: dict set -> dict(tf, e, mean, moved)."""
    sets = ['vertices'] + (['joints'] if joints else [])
    x = {k: d['rows'][k][:B] for k in sets}
    y = {k: d['tgt'][k][:B].astype(np.float64) for k in sets}
    w = {k: d['w'][k][:B] if weighted else None for k in sets}
    if align == 'none':
        tf = {k: A.identity64(B) for k in sets}
    elif align == 'root':
        one = A.root64(x['joints'], y['joints'], w['joints'])
        tf = {k: one for k in sets}
    else:
        src = dict(each=None, vertices='vertices', joints='joints')[align_on]
        solved = {k: A.procrustes64(x[k], y[k], w[k], align) for k in sets if src in (None, k)}
        tf = {k: solved[src or k] for k in sets}
        if align in ('rigid', 'similarity'):
            for k, v in solved.items():
                assert np.nanmin(v['cond']) >= COND_MIN, (k, v['cond'])
    out = {}
    for k in sets:
        e = A.errors64(x[k], y[k], tf[k])
        out[k] = dict(tf=tf[k], e=e, mean=A.row_mean64(e, w[k]), moved=A.move64(x[k], tf[k]), x=x[k], y=y[k], w=w[k])
    return out


def gate(a):
    return GATE_C * error_gate(np.concatenate([a['moved'], a['y']], -1), a['e'])


def ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def check(res, arb, align, align_on, tag, plain=False):
    """The gates of the module docstring on the result of one call; prints the worst ratios, then asserts.  ``plain``: the
    call had the default arguments, so it returns the errors alone."""
    worst = {}
    for k, name in (('vertices', 'vertex'), ('joints', 'joint')):
        if k not in arb:
            assert f'{name}_error' not in res and f'mean_{name}_error' not in res
            continue
        a = arb[k]
        g = gate(a)
        ours = res[f'{name}_error'].cpu().numpy().astype(np.float64)
        assert ours.shape == a['e'].shape and np.isfinite(ours).all(), (tag, k)
        worst[f'{name}_error'] = float((np.abs(ours - a['e']) / (g / GATE_C)).max())
        if plain:
            continue
        mean = res[f'mean_{name}_error'].cpu().numpy().astype(np.float64)
        mg = A.row_mean64(g, a['w']) + ulp32(a['mean'])
        worst[f'mean_{name}'] = float((np.abs(mean - a['mean']) / (mg / GATE_C)).max())
    if plain:
        assert not any('align' in k or 'mean' in k for k in res), sorted(res)
    sets = [] if plain else [('align', 'joints' if (align == 'root' or (align_on == 'joints' and align != 'none')) else 'vertices')]
    if plain:
        pass
    elif 'joints' in arb and align_on == 'each' and align in SOLVED:
        sets.append(('joint_align', 'joints'))
    else:
        assert not any(k.startswith('joint_align') for k in res)
    for prefix, k in sets:
        a = arb[k]
        tf = dict(s=res[f'{prefix}_scale'].cpu().numpy(), R=res[f'{prefix}_rotation'].cpu().numpy(),
                  t=res[f'{prefix}_translation'].cpu().numpy())
        R = tf['R'].astype(np.float64)
        assert np.abs(np.einsum('bkr,bkc->brc', R, R) - np.eye(3)).max() <= 1e-6 and (np.linalg.det(R) > 0).all(), (tag, prefix)
        mine = A.errors64(a['x'], a['y'], tf)
        worst[f'{prefix}_effect'] = float((np.abs(mine - a['e']) / (gate(a) / GATE_C)).max())
    print(f'[align] {tag}: ' + ', '.join(f'{k} {v:.3f} g' for k, v in worst.items()) + f' (gate {GATE_C:g} g)')
    for k, v in worst.items():
        assert v <= GATE_C, (tag, k, v)
    return worst


def run_case(name, B, align, align_on, weighted, joints, model_root, golden, dev, form='pose', mirrored=False, tag=None, **kw):
    m, om = _model(name, model_root, golden, dev)
    d = case_data(name, om, form, mirrored)
    params = _slice(d['ref'].dev, B)
    tv, tj = d['tgt_dev']['vertices'][:B], d['tgt_dev']['joints'][:B] if joints else None
    vw = d['w_dev']['vertices'][:B] if weighted else None
    jw = d['w_dev']['joints'][:B] if weighted and joints else None
    res = m.mesh_error(tv, tj, align=align, align_on=align_on, vertex_weights=vw, joint_weights=jw, **params, **kw)
    arb = arbiter(d, B, align, align_on, weighted, joints)
    tag = tag or f'{name} B = {B} {align}/{align_on}{" weighted" if weighted else ""}{"" if joints else " no joints"}' \
                 f'{" mirrored" if mirrored else ""}'
    check(res, arb, align, align_on, tag, plain=align == 'none' and not weighted and not kw)
    return m, d, params, res, arb


@pytest.mark.parametrize('B', [1, 3, 65, 129])
def test_smpl_batch_edges(B, model_root, golden, dev, smplfit_env):
    """SMPL on the batch-major route at partial 64- and 128-instance blocks: PA-PVE / PA-MPJPE with weights, the far row
    included from B = 3 on."""
    smplfit_env('SMPLFIT_BM', None)
    m, _, _, res, _ = run_case('smpl', B, 'similarity', 'each', True, True, model_root, golden, dev)
    assert m.kernel_path() == 'batch-major'
    assert res['vertex_error'].shape == (B, m.num_vertices) and res['mean_joint_error'].shape == (B,)
    assert res['align_rotation'].shape == (B, 3, 3) and res['joint_align_translation'].shape == (B, 3)


@pytest.mark.parametrize('align', ['none', 'root', 'translation', 'rigid', 'similarity'])
@pytest.mark.parametrize('align_on', ['each', 'vertices', 'joints'])
@pytest.mark.parametrize('weighted', [False, True])
def test_modes(align, align_on, weighted, model_root, golden, dev):
    """Every align x align_on, with and without weights, SMPL at B = 3 (the far row is row 2)."""
    run_case('smpl', 3, align, align_on, weighted, True, model_root, golden, dev)


@pytest.mark.parametrize('align', ['none', 'translation', 'rigid', 'similarity'])
@pytest.mark.parametrize('weighted', [False, True])
def test_without_target_joints(align, weighted, model_root, golden, dev):
    m, d, params, res, _ = run_case('smpl', 3, align, 'each', weighted, False, model_root, golden, dev)
    assert 'joint_error' not in res and 'mean_joint_error' not in res
    with pytest.raises(ValueError):
        m.mesh_error(d['tgt_dev']['vertices'][:3], align='root', **params)


@pytest.mark.parametrize('align,align_on', [('rigid', 'each'), ('similarity', 'each'), ('similarity', 'vertices'),
                                            ('rigid', 'joints')])
def test_mirrored_targets(align, align_on, model_root, golden, dev):
    """x-mirrored targets: the best orthogonal fit is a reflection, the result is the best proper rotation."""
    run_case('smpl', 8, align, align_on, False, True, model_root, golden, dev, mirrored=True)


@pytest.mark.parametrize('name,B', [('smplxfat', 67), ('smpl1024', 67), ('smpl_b32', 5), ('smpl_w12', 5)])
def test_models_and_routes(name, B, model_root, golden, dev):
    """SMPL-X-fat, the 1024-vertex subset (one moments slab), and the general path."""
    run_case(name, B, 'similarity', 'each', True, True, model_root, golden, dev)
    run_case(name, 3, 'rigid', 'vertices', False, True, model_root, golden, dev)


def test_wave_route(model_root, golden, dev, smplfit_env):
    """SMPL with SMPLFIT_BM=0: the wave-per-instance forward pass writes the mesh the alignment reads."""
    smplfit_env('SMPLFIT_BM', '0')
    run_case('smpl', 67, 'similarity', 'each', True, True, model_root, golden, dev, tag='smpl wave B = 67')


def test_kid(model_root, golden, dev):
    run_case('smpl', 65, 'similarity', 'each', False, True, model_root, golden, dev, form='kid', tag='smpl kid B = 65')


def _c_call(m, dev, params, tv, tj, al, outs, ws=None, kid=False):
    """smplfit_mesh_error_aligned_f32 on caller-made outputs (``outs``: names of both structs -> tensors) and workspace."""
    from smplfitter_amd import _lib

    B = tv.shape[0]
    h = m._native(dev, kid=kid)
    if ws is None:
        ws = torch.empty(h.mesh_error_aligned_workspace_bytes(B), dtype=torch.uint8, device=dev)
    recon = {k: v.data_ptr() for k, v in outs.items() if k in _lib.RECON_KEYS}
    rest = {k: v.data_ptr() for k, v in outs.items() if k not in _lib.RECON_KEYS}
    args = _lib.MeshErrorArgs(
        pose_rotvecs=params['pose_rotvecs'].data_ptr(), shape_betas=params['shape_betas'].data_ptr(),
        num_betas_given=params['shape_betas'].shape[1], trans=params['trans'].data_ptr(), batch=B,
        target_vertices=tv.data_ptr(), target_joints=None if tj is None else tj.data_ptr(), workspace=ws.data_ptr(),
        workspace_bytes=ws.numel(), hip_stream=torch.cuda.current_stream(dev).cuda_stream, **recon)
    rc = _lib.load().smplfit_mesh_error_aligned_f32(h.ptr, C.byref(args), C.byref(_lib.MeshAlignArgs(**al, **rest)))
    torch.cuda.synchronize()
    return rc


def _all_outputs(B, V, J, dev, fill=float('nan')):
    new = lambda *s: torch.full(s, fill, dtype=torch.float32, device=dev)  # noqa: E731
    return dict(vertices=new(B, V, 3), joints=new(B, J, 3), vertex_error=new(B, V), joint_error=new(B, J),
                mean_vertex_error=new(B), mean_joint_error=new(B), scale=new(B), rotation=new(B, 3, 3), translation=new(B, 3),
                joint_scale=new(B), joint_rotation=new(B, 3, 3), joint_translation=new(B, 3))


def test_identities(model_root, golden, dev):
    """Default arguments give the bits of the mesh-error step; align='none' those bits plus the means; 'vertices' is
    forward's; two runs give the same bits."""
    m, om = _model('smpl', model_root, golden, dev)
    d = case_data('smpl', om)
    B = 65
    params = _slice(d['ref'].dev, B)
    tv, tj = d['tgt_dev']['vertices'][:B], d['tgt_dev']['joints'][:B]
    vw, jw = d['w_dev']['vertices'][:B], d['w_dev']['joints'][:B]
    keys = ['vertex_error', 'joint_error', 'vertices', 'joints']
    direct = m._recon_direct(keys, tv, tj, **params)
    plain = m.mesh_error(tv, tj, return_mesh=True, **params)
    assert sorted(plain) == sorted(keys)
    fw = m(**params)
    for k in keys:
        assert torch.equal(plain[k], direct[k]), k
    none = m.mesh_error(tv, tj, return_mesh=True, vertex_weights=vw, joint_weights=jw, **params)
    for k in keys:
        assert torch.equal(none[k], direct[k]), k
    assert 'mean_vertex_error' in none and 'mean_joint_error' in none
    assert torch.equal(none['align_rotation'], torch.eye(3, device=dev).expand(B, 3, 3)) and bool((none['align_scale'] == 1).all())
    for align, on in (('similarity', 'each'), ('rigid', 'joints'), ('root', 'each')):
        a = m.mesh_error(tv, tj, return_mesh=True, align=align, align_on=on, vertex_weights=vw, joint_weights=jw, **params)
        b = m.mesh_error(tv, tj, return_mesh=True, align=align, align_on=on, vertex_weights=vw, joint_weights=jw, **params)
        assert sorted(a) == sorted(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (align, k)
        assert torch.equal(a['vertices'], fw['vertices']) and torch.equal(a['joints'], fw['joints'])
        lean = m.mesh_error(tv, tj, align=align, align_on=on, vertex_weights=vw, joint_weights=jw, **params)
        assert 'vertices' not in lean
        for k in lean:  # (the mesh in the workspace instead of the caller's)
            assert torch.equal(lean[k], a[k]), (align, k)


@pytest.mark.parametrize('smplfit_bm', [None, '0'])
def test_workspace_outputs_and_single_requests(smplfit_bm, model_root, golden, dev, smplfit_env):
    """NaN-filled outputs are fully overwritten; a zeroed and a NaN-filled workspace give the same bits; every output
    asked for on its own has the bits of the full request; a refused call leaves NaN-filled outputs NaN."""
    from smplfitter_amd import _lib

    smplfit_env('SMPLFIT_BM', smplfit_bm)
    m, om = _model('smpl', model_root, golden, dev)
    d = case_data('smpl', om)
    B, V, J = 5, m.num_vertices, m.num_joints
    params = _slice(d['ref'].dev, B)
    tv, tj = d['tgt_dev']['vertices'][:B].contiguous(), d['tgt_dev']['joints'][:B].contiguous()
    vw = d['w_dev']['vertices'][:B].contiguous()
    n = m._native(dev).mesh_error_aligned_workspace_bytes(B)
    for mode, on in ((4, 0), (3, 1), (3, 2), (1, 0), (0, 0)):
        al = dict(align=mode, align_on=on, vertex_weights=vw.data_ptr())
        skip = {'joint_scale', 'joint_rotation', 'joint_translation'} if (on or mode < 2) else set()
        skip |= {'scale', 'rotation', 'translation'} if mode == 0 else set()
        runs = []
        for fill in (0x00, 0xFF):
            outs = {k: v for k, v in _all_outputs(B, V, J, dev).items() if k not in skip}
            ws = torch.full((n,), fill, dtype=torch.uint8, device=dev)
            assert _c_call(m, dev, params, tv, tj, al, outs, ws) == _lib.SMPLFIT_OK, _lib.load().smplfit_last_error()
            assert all(bool(torch.isfinite(v).all()) for v in outs.values()), (mode, on)
            runs.append(outs)
        for k in runs[0]:
            assert torch.equal(runs[0][k], runs[1][k]), (mode, on, k)
        for k in runs[0]:
            one = {k: _all_outputs(B, V, J, dev)[k]}
            assert _c_call(m, dev, params, tv, tj, al, one) == _lib.SMPLFIT_OK, (k, _lib.load().smplfit_last_error())
            assert torch.equal(one[k], runs[0][k]), (mode, on, k)
        # a call that is given the mesh and both error buffers leaves their three regions off the workspace: the same
        # bits; without the buffers that size is refused and nothing is written
        r256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
        small = n - r256(12 * B * V) - r256(4 * B * V) - r256(4 * B * J)
        outs = {k: v for k, v in _all_outputs(B, V, J, dev).items() if k not in skip}
        ws = torch.full((small,), 0xFF, dtype=torch.uint8, device=dev)
        assert _c_call(m, dev, params, tv, tj, al, outs, ws) == _lib.SMPLFIT_OK, _lib.load().smplfit_last_error()
        for k in outs:
            assert torch.equal(outs[k], runs[0][k]), (mode, on, k)
        lean = {'mean_vertex_error': _all_outputs(B, V, J, dev)['mean_vertex_error']}
        assert _c_call(m, dev, params, tv, tj, al, lean, ws) == _lib.SMPLFIT_ERR_WORKSPACE
        assert bool(torch.isnan(lean['mean_vertex_error']).all())
    # refusals: nothing is enqueued, the outputs stay NaN
    full = _all_outputs(B, V, J, dev)
    for al, tjx, outs in ((dict(align=5), tj, full), (dict(align=4, align_on=3), tj, full),
                          (dict(align=1), None, {k: full[k] for k in ('vertex_error', 'mean_vertex_error', 'translation')}),
                          (dict(align=4, align_on=2), None, {k: full[k] for k in ('vertex_error', 'scale')}),
                          (dict(align=4), None, {k: full[k] for k in ('vertex_error', 'mean_joint_error')}),
                          (dict(align=4), None, {k: full[k] for k in ('vertex_error', 'joint_rotation')}),
                          (dict(align=0), tj, {k: full[k] for k in ('vertex_error', 'scale')}),
                          (dict(align=4, align_on=1), tj, {k: full[k] for k in ('vertex_error', 'joint_scale')}),
                          (dict(align=4), tj, {})):
        assert _c_call(m, dev, params, tv, tjx, al, outs) == _lib.SMPLFIT_ERR_BAD_ARG, (al, _lib.load().smplfit_last_error())
        assert all(bool(torch.isnan(v).all()) for v in full.values()), al


def test_row_independence(model_root, golden, dev):
    """A NaN target row and a zero-weight row are NaN in that row, under the transform that set gives, and every other
    row keeps the bits of the clean call."""
    m, om = _model('smpl', model_root, golden, dev)
    d = case_data('smpl', om)
    B, nan_row, zero_row = 67, 5, 64
    params = _slice(d['ref'].dev, B)
    tv, tj = d['tgt_dev']['vertices'][:B].clone(), d['tgt_dev']['joints'][:B]
    vw, jw = d['w_dev']['vertices'][:B].clone(), d['w_dev']['joints'][:B]
    kw = dict(align='similarity', align_on='each', joint_weights=jw, **params)
    clean = m.mesh_error(tv, tj, vertex_weights=vw, **kw)
    tv[nan_row, 17, 1] = float('nan')
    vw[zero_row] = 0.0
    res = m.mesh_error(tv, tj, vertex_weights=vw, **kw)
    keep = torch.ones(B, dtype=torch.bool, device=dev)
    keep[[nan_row, zero_row]] = False
    for k in res:
        if k.startswith('joint') or k == 'mean_joint_error':  # (the joints' own alignment never saw the vertices)
            assert torch.equal(res[k], clean[k]), k
        else:
            assert torch.equal(res[k][keep], clean[k][keep]), k
            assert bool(torch.isnan(res[k][~keep]).all()), k
    neg = vw.clone()
    neg[1, 3] = -1.0
    res = m.mesh_error(tv, tj, vertex_weights=neg, **kw)
    assert bool(torch.isnan(res['vertex_error'][1]).all()) and bool(torch.isnan(res['align_scale'][1]))
    assert bool(torch.isfinite(res['vertex_error'][0]).all())


def test_with_rototranslate(model_root, golden, dev):
    """The returned rigid (R, t) moves the parameters: ``mesh_error(align='none')`` at ``rototranslate``'s result meets
    the sum of the two gates against the aligned errors."""
    m, d, params, res, arb = run_case('smpl', 8, 'rigid', 'vertices', False, True, model_root, golden, dev)
    pose, trans = m.rototranslate(res['align_rotation'], res['align_translation'], params['pose_rotvecs'],
                                  params['shape_betas'], params['trans'])
    tv, tj = d['tgt_dev']['vertices'][:8], d['tgt_dev']['joints'][:8]
    moved = m.mesh_error(tv, tj, pose_rotvecs=pose, shape_betas=params['shape_betas'], trans=trans)
    worst = {}
    for k, name in (('vertices', 'vertex'), ('joints', 'joint')):
        a = arb[k]
        g = gate(a) + error_gate(np.concatenate([a['moved'], a['y']], -1), a['e'])
        worst[name] = float((np.abs(moved[f'{name}_error'].cpu().numpy() - a['e']) / g).max())
    print('[align] rototranslate: ' + ', '.join(f'{k} {v:.3f} of the summed gates' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_gradient_route(model_root, golden, dev):
    """An input that requires grad: the same keys from forward and PyTorch arithmetic, inside the same gates, and a
    gradient reaches the parameters."""
    m, om = _model('smpl', model_root, golden, dev)
    d = case_data('smpl', om)
    B = 3
    params = {k: v.clone() for k, v in _slice(d['ref'].dev, B).items()}
    params['trans'].requires_grad_()
    tv, tj = d['tgt_dev']['vertices'][:B], d['tgt_dev']['joints'][:B]
    vw, jw = d['w_dev']['vertices'][:B], d['w_dev']['joints'][:B]
    for align, on in (('similarity', 'each'), ('rigid', 'joints'), ('root', 'each'), ('none', 'each')):
        res = m.mesh_error(tv, tj, align=align, align_on=on, vertex_weights=vw, joint_weights=jw, **params)
        assert res['vertex_error'].grad_fn is not None
        check({k: v.detach() for k, v in res.items()}, arbiter(d, B, align, on, True, True), align, on, f'grad route {align}/{on}')
    res['mean_vertex_error'].sum().backward()
    assert bool(torch.isfinite(params['trans'].grad).all()) and float(params['trans'].grad.abs().max()) > 0


def test_compile_route(model_root, golden, dev):
    m, om = _model('smpl', model_root, golden, dev)
    d = case_data('smpl', om)
    B = 3
    params = _slice(d['ref'].dev, B)
    tv, tj = d['tgt_dev']['vertices'][:B], d['tgt_dev']['joints'][:B]

    def fn(tv, tj, pose, betas, trans):
        return m.mesh_error(tv, tj, pose_rotvecs=pose, shape_betas=betas, trans=trans, align='similarity')

    res = torch.compile(fn, backend='aot_eager', fullgraph=True)(tv, tj, params['pose_rotvecs'], params['shape_betas'], params['trans'])
    check(res, arbiter(d, B, 'similarity', 'each', False, True), 'similarity', 'each', 'compile route')


@pytest.mark.parametrize('align', SOLVED)
@pytest.mark.parametrize('N', [1, 24, 2048, 2049, 6890])
def test_align_points(align, N, model_root, golden, dev):
    """``align_points`` on raw points — N vertices of the SMPL case, so one point, one slab, the slab edge and several
    slabs — against the arbiter, the far row included; two runs give the same bits; a zero-weight row is NaN."""
    from smplfitter_amd.pt import align_points

    m, om = _model('smpl', model_root, golden, dev)
    d = case_data('smpl', om)
    B = 5
    idx = torch.from_numpy(np.linspace(0, m.num_vertices - 1, N).astype(np.int64))  # (spread over the body)
    x64 = d['rows']['vertices'][:B][:, idx.numpy()]
    x = torch.from_numpy(x64.astype(np.float32)).to(dev)
    y, w = d['tgt_dev']['vertices'][:B][:, idx.to(dev)].contiguous(), d['w_dev']['vertices'][:B][:, idx.to(dev)] + 0.1
    w[3] = 0.0
    res = align_points(x, y, w, align=align)
    again = align_points(x, y, w, align=align)
    for k in res:  # (bit patterns: row 3 is NaN)
        assert torch.equal(res[k].view(torch.int32), again[k].view(torch.int32)), k
    wn, yn = w.cpu().numpy(), y.cpu().numpy().astype(np.float64)
    xs = x.cpu().numpy().astype(np.float64)
    ref = A.procrustes64(xs, yn, wn, align)
    live = np.array([0, 1, 2, 4])
    ours = {k: v.cpu().numpy().astype(np.float64) for k, v in res.items()}
    dead_keys = ours if not (N == 1 and align == 'similarity') else {}
    for k in dead_keys:
        assert np.isnan(ours[k][3]).all(), k
    if N == 1 and align == 'similarity':  # (one point has no spread: every row is NaN)
        assert all(np.isnan(v).all() for v in ours.values())
        return
    if N >= 24 and align != 'translation':
        assert np.nanmin(ref['cond'][live]) >= COND_MIN, ref['cond']
    if N == 1 and align != 'translation':
        return  # (the rotation of a single point is free; its error is covered by the translation case)
    e = A.errors64(xs, yn, ref)
    a = dict(moved=A.move64(xs, ref)[live], y=yn[live], e=e[live])
    ratio = float((np.abs(ours['error'][live] - e[live]) / (gate(a) / GATE_C)).max())
    mg = A.row_mean64(gate(a), wn[live]) + ulp32(A.row_mean64(e, wn)[live])
    mratio = float((np.abs(ours['mean_error'][live] - A.row_mean64(e, wn)[live]) / (mg / GATE_C)).max())
    print(f'[align] align_points {align} N = {N}: error {ratio:.3f} g, mean {mratio:.3f} g')
    assert ratio <= GATE_C and mratio <= GATE_C
