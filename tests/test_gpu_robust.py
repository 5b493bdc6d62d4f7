"""-m gpu: ``k_robust_reweight`` on its own against numpy, ``BodyFitter.fit_robust`` against the same loop written with
the public calls (same bits), against the fp64 arbiter of tests/robust_util.py, on what it is for (targets with gross
outliers), and its refusals."""

import ctypes as C

import numpy as np
import pytest
import torch

import robust_util as R
import util

pytestmark = pytest.mark.gpu

FIT_KEYS = ('pose_rotvecs', 'shape_betas', 'trans', 'orientations', 'relative_orientations')
ROBUST_KEYS = ('robust_vertex_weights', 'robust_joint_weights', 'robust_scale')
SENTINEL = -7.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


_models = {}


def get_fitter(model_root, golden, dev, name, kid=False):
    """(BodyModel, BodyFitter) of 'smpl', 'smplx', 'smpl1024' (the 1024-vertex subset) or 'smpl_b32' (general path)."""
    from smplfitter_amd.pt import BodyFitter, BodyModel

    if (name, kid) not in _models:
        if name == 'smpl_b32':
            m = BodyModel('smpl', 'neutral', model_root=f'{model_root}/smpl_b32', num_betas=32, device=dev)
        else:
            kw = dict(vertex_subset=golden(name)['vertex_subset']) if name == 'smpl1024' else {}
            m = BodyModel('smplx' if name == 'smplx' else 'smpl', 'neutral', model_root=f'{model_root}/{util.model_dir(name)}',
                          num_betas=10, device=dev, **kw)
        _models[name, kid] = (m, BodyFitter(m, enable_kid=kid))
    return _models[name, kid]


def t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def n(x):
    return None if x is None else x.cpu().numpy()


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------
def padded(B, N, dev, pad=3):
    """A (B, N) view in the middle of a sentinel-filled buffer, and the buffer."""
    buf = torch.full((B * N + 2 * pad,), SENTINEL, dtype=torch.float32, device=dev)
    return buf[pad:pad + B * N].view(B, N), buf, pad


def run_step(f, dev, ev, ej, w0v, w0j, **kw):
    """``_robust_weights`` into padded outputs; asserts the padding is untouched; numpy results."""
    B, Nv = ev.shape
    outs = dict(robust_vertex_weights=padded(B, Nv, dev), robust_scale=padded(B, 1, dev))
    if ej is not None:
        outs['robust_joint_weights'] = padded(B, ej.shape[1], dev)
    views = {k: (v[0] if k != 'robust_scale' else v[0].view(B)) for k, v in outs.items()}
    r = f._robust_weights(t(ev, dev), t(ej, dev), t(w0v, dev), t(w0j, dev), _out=views, **kw)
    assert set(r) == set(outs)
    for k, (view, buf, pad) in outs.items():
        assert r[k].data_ptr() == view.data_ptr()
        assert torch.all(buf[:pad] == SENTINEL) and torch.all(buf[-pad:] == SENTINEL), k
    return {k: n(v) for k, v in r.items()}


def check_step(r, ev, ej, w0v, w0j, loss, tuning, scale=None, scale_floor=1e-3):
    """``robust_scale`` to the bit (fp32: one product and a max); the weights within 2e-6 * w0 of numpy fp64 on the same
    fp32 inputs — derived, not measured: at most seven fp32 roundings (tuning * sigma, the quotient, u * u, 1 + ., the
    square, the reciprocal, the product with w0) of a quantity <= w0, 7 * 2^-24 = 4.2e-7, with a threefold margin and
    rounded up —; a zero prior weight gives exactly 0, Tukey from u = 1 on exactly 0."""
    sigma = R.scale_of(ev, w0v, scale, scale_floor)
    assert r['robust_scale'].dtype == np.float32
    assert np.array_equal(r['robust_scale'].view(np.uint32), sigma.astype(np.float32).view(np.uint32))
    for e, w0, key in ((ev, w0v, 'robust_vertex_weights'), (ej, w0j, 'robust_joint_weights')):
        if e is None:
            assert key not in r
            continue
        want = R.weights_of(e, w0, loss, tuning, sigma)
        bound = 2e-6 * (1.0 if w0 is None else np.abs(w0.astype(np.float64)))
        err = np.abs(r[key] - want)
        assert np.all(err <= bound), (key, loss, float((err - bound).max()))
        if w0 is not None:
            assert np.all(r[key][w0 == 0] == 0)
        if loss == 'tukey':
            u = e.astype(np.float64) / (tuning * sigma.astype(np.float64)[:, None])
            assert np.all(r[key][u >= 1 + 1e-6] == 0)  # (u itself carries two fp32 roundings)


def step_inputs(B, Nv, Nj, seed, priors):
    rs = np.random.RandomState(seed)
    ev = (np.abs(rs.randn(B, Nv)) * 0.01 * np.exp(rs.randn(B, 1))).astype(np.float32)
    ev[rs.rand(B, Nv) < 0.1] *= 30  # outliers
    ej = (np.abs(rs.randn(B, Nj)) * 0.02).astype(np.float32) if Nj else None
    w0v = w0j = None
    if priors:
        w0v = np.where(rs.rand(B, Nv) < 1 / 3, 0, rs.rand(B, Nv) + 0.05).astype(np.float32)
        w0j = np.where(rs.rand(B, Nj) < 1 / 3, 0, rs.rand(B, Nj) + 0.05).astype(np.float32) if Nj else None
    return ev, ej, w0v, w0j


@pytest.mark.parametrize('Nv', [1, 2, 63, 64, 65, 255, 256, 257, 6890, 12288, 12289, 20000])
def test_kernel_alone(Nv, model_root, golden, dev):
    """Seeded errors at B in {1, 3, 65}, N_j in {0, 24}, with and without prior weights (a third of them zero), all
    four losses and the three scale sources; N_v = 20000 takes the branch that reads the errors again in every pass
    instead of staging them in LDS; 12288 and 12289 are the last staged size (48 KB of keys) and the first that is
    not."""
    _, f = get_fitter(model_root, golden, dev, 'smpl')
    case = 0
    for B in (1, 3, 65):
        rows = (np.random.RandomState(B).rand(B) * 0.05 + 0.002).astype(np.float32)
        for loss in R.LOSSES:
            for mode in ('median', 'fixed', 'rows'):
                case += 1
                Nj, priors = (0, 24)[case % 2], (case // 2) % 2 == 1
                ev, ej, w0v, w0j = step_inputs(B, Nv, Nj, 1000 * Nv + case, priors)
                tuning = R.TUNING[loss] * (1 if case % 3 else 0.4)
                scale = dict(median=None, fixed=0.0125, rows=rows)[mode]
                r = run_step(f, dev, ev, ej, w0v, w0j, loss=loss, tuning=tuning,
                             scale=t(scale, dev) if mode == 'rows' else scale, scale_floor=1e-3)
                check_step(r, ev, ej, w0v, w0j, loss, tuning, scale, 1e-3)


@pytest.mark.parametrize('Nv', [1, 2, 64, 257, 6890, 20000])
def test_kernel_ties_and_floor(Nv, model_root, golden, dev):
    """All errors equal, half of them zero, all zero (the floor is active), every entry ineligible (the floor again);
    Tukey with e = tuning * sigma exactly gives exactly 0, Huber exactly 1 there."""
    _, f = get_fitter(model_root, golden, dev, 'smpl')
    B = 3
    rs = np.random.RandomState(Nv)
    half = np.where(np.arange(Nv) % 2 == 0, 0, rs.rand(B, Nv) * 0.1).astype(np.float32)
    for name, ev in (('equal', np.full((B, Nv), 0.0123, np.float32)), ('halfzero', half), ('zero', np.zeros((B, Nv), np.float32))):
        for loss in R.LOSSES:
            r = run_step(f, dev, ev, None, None, None, loss=loss, scale_floor=2e-3)
            check_step(r, ev, None, None, None, loss, R.TUNING[loss], None, 2e-3)
            if name == 'zero':
                assert np.all(r['robust_scale'] == np.float32(2e-3)) and np.all(r['robust_vertex_weights'] == 1)
    ev = np.full((B, Nv), 0.5, np.float32)
    r = run_step(f, dev, ev, None, np.zeros((B, Nv), np.float32), None, loss='cauchy', scale_floor=0.25)
    assert np.all(r['robust_scale'] == 0.25) and np.all(r['robust_vertex_weights'] == 0)
    ev = np.full((B, Nv), 2.0, np.float32)
    assert np.all(run_step(f, dev, ev, None, None, None, loss='tukey', tuning=4.0, scale=0.5)['robust_vertex_weights'] == 0)
    assert np.all(run_step(f, dev, ev, None, None, None, loss='huber', tuning=4.0, scale=0.5)['robust_vertex_weights'] == 1)


@pytest.mark.parametrize('Nv', [65, 6890, 12288, 12289, 20000])
def test_kernel_nonfinite_row(Nv, model_root, golden, dev):
    """A NaN or an inf among a row's vertex or joint errors: that row's scale and weights are NaN, every other row has
    the bits of the call without it — for every scale source."""
    _, f = get_fitter(model_root, golden, dev, 'smpl')
    B = 4
    ev, ej, w0v, w0j = step_inputs(B, Nv, 24, Nv, True)
    w0v[1, Nv // 2] = 0  # (not even an entry that the median skips may hide a non-finite error)
    rows = t(np.full(B, 0.02, np.float32), dev)
    for scale in (None, 0.02, rows):
        clean = run_step(f, dev, ev, ej, w0v, w0j, loss='geman_mcclure', scale=scale)
        for where, value in (('v', np.nan), ('v', np.inf), ('j', np.nan)):
            ev2, ej2 = ev.copy(), ej.copy()
            if where == 'v':
                ev2[1, Nv // 2] = value
            else:
                ej2[1, 5] = value
            r = run_step(f, dev, ev2, ej2, w0v, w0j, loss='geman_mcclure', scale=scale)
            for k in r:
                assert np.all(np.isnan(r[k][1])), (k, where, value)
                assert np.array_equal(np.delete(r[k], 1, 0), np.delete(clean[k], 1, 0)), (k, where, value)


@pytest.mark.parametrize('Nv', [65, 20000])
def test_kernel_bad_row_scale(Nv, model_root, golden, dev):
    """A per-row scale that is zero, negative, NaN or inf — seen on the device alone — gives its row NaN scale and NaN
    weights throughout, zero prior weights included; every other row has the bits of the call with a good scale there."""
    _, f = get_fitter(model_root, golden, dev, 'smpl')
    B = 6
    ev, ej, w0v, w0j = step_inputs(B, Nv, 24, Nv + 1, True)
    good = np.full(B, 0.02, np.float32)
    clean = run_step(f, dev, ev, ej, w0v, w0j, loss='tukey', scale=t(good, dev))
    rows = good.copy()
    rows[[0, 2, 3, 5]] = [0.0, -0.02, np.nan, np.inf]
    r = run_step(f, dev, ev, ej, w0v, w0j, loss='tukey', scale=t(rows, dev))
    for k in r:
        assert np.all(np.isnan(r[k][[0, 2, 3, 5]])), k
        assert np.array_equal(r[k][[1, 4]], clean[k][[1, 4]]), k


# ---- 2. the same bits as the loop of public calls ------------------------------------------------------------------
def fit_targets(m, B, dev, seed, joints=True, frac=0.1):
    """Seeded bodies with 5 mm noise and a tenth of the vertices displaced by N(0, 0.3 m)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    rnd = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
    fw = m(pose_rotvecs=(rnd(B, m.num_joints * 3) * 0.2).to(dev), shape_betas=(rnd(B, m.num_betas) * 0.5).to(dev),
           trans=(rnd(B, 3) * 0.5).to(dev))
    V = m.num_vertices
    mask = (torch.rand(B, V, 1, generator=g) < frac).float()
    tv = fw['vertices'] + (rnd(B, V, 3) * 0.005 + mask * rnd(B, V, 3) * 0.3).to(dev)
    tj = fw['joints'] + (rnd(B, m.num_joints, 3) * 0.005).to(dev) if joints else None
    return tv, tj


def composed(f, tv, tj, w0v, w0j, num_rounds, num_iter, round_num_iter, robust_kw, fit_kw):
    """The loop with the calls that exist without fit_robust, fed with the kernel's own weights."""
    errs = ['vertex_error'] + (['joint_error'] if tj is not None else [])
    r = f.fit(tv, tj, w0v, w0j, num_iter=num_iter, requested_keys=['pose_rotvecs'] + errs, **fit_kw)
    w = {}
    for _ in range(num_rounds):
        w = f._robust_weights(r['vertex_error'], r.get('joint_error'), w0v, w0j if tj is not None else None, **robust_kw)
        r = f.fit(tv, tj, w['robust_vertex_weights'], w.get('robust_joint_weights'), num_iter=round_num_iter,
                  initial_pose_rotvecs=r['pose_rotvecs'], requested_keys=['pose_rotvecs'] + errs, **fit_kw)
    r.update(w)
    return r


def assert_same_bits(a, b, keys):
    for k in keys:
        assert (k in a) == (k in b), k
        if k in a:
            assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())


BITS_CASES = {
    # name: (model, kid, B, joints, priors, fit options, robust options)
    'smpl_j': ('smpl', False, 5, True, False, {}, {}),
    'smpl_nj': ('smpl', False, 5, False, False, {}, dict(loss='huber')),
    'smpl_j_w': ('smpl', False, 5, True, True, dict(beta_regularizer=0.0), dict(loss='tukey')),
    'smpl_nj_w': ('smpl', False, 5, False, True, {}, dict(loss='cauchy', scale=0.02)),
    'smpl_kid': ('smpl', True, 5, True, False, {}, {}),
    'smplx': ('smplx', False, 3, True, False, {}, {}),
    'smpl_b32': ('smpl_b32', False, 3, True, False, {}, {}),
    'smpl1024': ('smpl1024', False, 5, True, False, {}, {}),
    'segments': ('smpl', False, 5, True, False, dict(share_beta_segments=[2, 3]), {}),
    'share_beta': ('smpl', False, 5, True, True, dict(share_beta=True, final_adjust_rots=False), dict(tuning=2.0)),
}


@pytest.mark.parametrize('num_rounds', [1, 2])
@pytest.mark.parametrize('case', list(BITS_CASES))
def test_same_bits_as_composition(case, num_rounds, model_root, golden, dev):
    """``fit_robust`` equals, key by key with ``torch.equal`` (the weights and the scale included), the loop
    ``fit(requested_keys=[errors])`` -> ``_robust_weights`` -> ``fit(vertex_weights, joint_weights, initial_pose_rotvecs
    = previous pose, num_iter = round_num_iter)``: SMPL on the batch-major route with and without target joints and prior
    weights, with the kid unknown, SMPL-X, the general path, the 1024-vertex subset, segments and share_beta."""
    name, kid, B, joints, priors, fit_kw, robust_kw = BITS_CASES[case]
    m, f = get_fitter(model_root, golden, dev, name, kid)
    if name == 'smpl':
        assert m.kernel_path() == 'batch-major'
    if name == 'smpl_b32':
        assert m.kernel_path() == 'general'
    tv, tj = fit_targets(m, B, dev, 11, joints)
    w0v = w0j = None
    if priors:
        g = torch.Generator(device='cpu').manual_seed(3)
        w0v = (torch.rand(B, m.num_vertices, generator=g) * (torch.rand(B, m.num_vertices, generator=g) > 0.2)).to(dev)
        w0j = torch.rand(B, m.num_joints, generator=g).to(dev) if joints else None
    ours = f.fit_robust(tv, tj, w0v, w0j, num_rounds=num_rounds, num_iter=2, round_num_iter=1,
                        requested_keys=['pose_rotvecs'], **fit_kw, **robust_kw)
    ref = composed(f, tv, tj, w0v, w0j, num_rounds, 2, 1, robust_kw, fit_kw)
    keys = FIT_KEYS + ROBUST_KEYS + ('kid_factor',)
    assert ('kid_factor' in ours) == kid and ('robust_joint_weights' in ours) == joints
    assert_same_bits(ours, ref, keys)
    for k in keys:
        if k in ours:
            assert torch.isfinite(ours[k]).all(), k
    # the default round_num_iter is num_iter
    a = f.fit_robust(tv, tj, w0v, w0j, num_rounds=1, num_iter=2, **fit_kw, **robust_kw)
    assert_same_bits(a, composed(f, tv, tj, w0v, w0j, 1, 2, 2, robust_kw, fit_kw), keys)


def test_zero_rounds_recon_and_workspaces(model_root, golden, dev):
    """``num_rounds=0`` is ``fit`` (the prior weights, or ones, and NaN scales come back); the reconstruction keys are
    ``mesh_error`` at the results; run to run, and with a zero-filled and a NaN-filled caller workspace, the bits are
    the same; ``pose_rotvecs`` only when requested."""
    m, f = get_fitter(model_root, golden, dev, 'smpl')
    B = 5
    tv, tj = fit_targets(m, B, dev, 12)
    w0v = torch.rand(B, m.num_vertices, generator=torch.Generator().manual_seed(1)).to(dev)
    w0j = torch.rand(B, m.num_joints, generator=torch.Generator().manual_seed(2)).to(dev)
    for pv, pj in ((None, None), (w0v, w0j)):
        z = f.fit_robust(tv, tj, pv, pj, num_rounds=0, num_iter=2)
        assert_same_bits(z, f.fit(tv, tj, pv, pj, num_iter=2), FIT_KEYS)
        assert torch.equal(z['robust_vertex_weights'], pv if pv is not None else torch.ones_like(w0v))
        assert torch.equal(z['robust_joint_weights'], pj if pj is not None else torch.ones_like(w0j))
        assert torch.isnan(z['robust_scale']).all()
    keys = ['pose_rotvecs', 'vertices', 'joints', 'vertex_error', 'joint_error']
    a = f.fit_robust(tv, tj, num_rounds=2, requested_keys=keys)
    me = m.mesh_error(tv, tj, glob_rotmats=a['orientations'], shape_betas=a['shape_betas'], trans=a['trans'], return_mesh=True)
    assert_same_bits(a, me, keys[1:])
    assert 'pose_rotvecs' not in f.fit_robust(tv, tj, num_rounds=1, requested_keys=['vertex_error'])
    h = m._native(dev)
    nbytes = h.fit_robust_workspace_bytes(B)
    assert nbytes >= h.fit_recon_workspace_bytes(B)
    all_keys = tuple(keys) + FIT_KEYS + ROBUST_KEYS
    assert_same_bits(a, f.fit_robust(tv, tj, num_rounds=2, requested_keys=keys), all_keys)
    for fill in (0, 0xFF):  # (0xFF bytes: every float of the workspace a NaN)
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
        assert_same_bits(a, f.fit_robust(tv, tj, num_rounds=2, requested_keys=keys, _workspace=ws), all_keys)
    with pytest.raises(Exception, match='workspace'):
        f.fit_robust(tv, tj, _workspace=torch.zeros(nbytes - 256, dtype=torch.uint8, device=dev))


# ---- 3. against fp64 -----------------------------------------------------------------------------------------------
_arb = {}


def arbiter_setup(model_root, frac=0.15, sigma=0.3):
    if (frac, sigma) not in _arb:
        md = util.load_md(model_root, 'smpl')[1]
        om64, om32 = util.O.OracleModel(md, np.float64, 'smpl'), util.O.OracleModel(md, np.float32, 'smpl')
        _arb[frac, sigma] = (om64, om32) + R.outlier_inputs(om64, 4, frac, sigma)
    return _arb[frac, sigma]


@pytest.mark.parametrize('cfg', [(0.0, 1), (1.0, 2)], ids=['reg0_it1', 'reg1_it2'])
@pytest.mark.parametrize('joints', [True, False], ids=['j', 'nj'])
@pytest.mark.parametrize('loss', R.LOSSES)
def test_against_fp64(loss, joints, cfg, model_root, golden, dev):
    """Two rounds on 15 % outliers of 0.3 m against the rounds written on the fp64 oracle: the vertex distance of the
    two fits is below max(2 * floor, 3e-5), floor = the distance of the same rounds on the fp32 oracle to the fp64 ones
    (the form of tests/test_gpu_parity.py::test_general_full_size).  Measured on an MI355X over the 16 cases: floor
    1.6e-5 ... 4.4e-5 m, ours 2.6e-6 ... 9.3e-6 m."""
    om64, om32, _, tv, tj = arbiter_setup(model_root)
    _, f = get_fitter(model_root, golden, dev, 'smpl')
    reg, num_iter = cfg
    kw = dict(loss=loss, num_rounds=2, num_iter=num_iter, beta_regularizer=reg)
    a64 = R.fit_robust(om64, tv, tj if joints else None, **kw)
    a32 = R.fit_robust(om32, tv, tj if joints else None, **kw)
    o = {k: n(v) for k, v in f.fit_robust(t(tv, dev), t(tj, dev) if joints else None, **kw).items()}
    err, floor = util.vertex_l2(om64, o, a64), util.vertex_l2(om64, a32, a64)
    print(f'[robust fp64] {loss} joints={joints} reg={reg} it={num_iter}: ours {err:.2e} floor {floor:.2e}')
    assert err < max(2 * floor, 3e-5)
    # the lower median moves by no more than the largest change of an error, and the errors of the round before by no
    # more than that round's vertex distance, which the gate above holds below 1e-4 m: 1.4826 * 1e-4, rounded up
    assert np.abs(o['robust_scale'] - a64['robust_scale']).max() < 1.5e-4


# ---- 4. it does what it is for ------------------------------------------------------------------------------------
@pytest.mark.parametrize('frac,sigma', [(0.15, 0.3), (0.05, 1.0)])
def test_rejects_outliers(frac, sigma, model_root, golden, dev):
    """Targets with gross outliers, target joints, no ridge, three iterations, Geman-McClure, two rounds: the largest
    per-row mean distance to the uncorrupted mesh is at most half the plain fit's (the fp64 arbiter: 0.29 and 0.16)."""
    om64, _, clean, tv, tj = arbiter_setup(model_root, frac, sigma)
    _, f = get_fitter(model_root, golden, dev, 'smpl')
    kw = dict(num_iter=3, beta_regularizer=0.0)
    plain = {k: n(v) for k, v in f.fit(t(tv, dev), t(tj, dev), **kw).items()}
    rob = {k: n(v) for k, v in f.fit_robust(t(tv, dev), t(tj, dev), loss='geman_mcclure', num_rounds=2, **kw).items()}
    dp, dr = R.mean_distance(om64, plain, clean), R.mean_distance(om64, rob, clean)
    print(f'[robust purpose] {frac} x {sigma} m: plain {dp * 1e3:.2f} mm, robust {dr * 1e3:.2f} mm, ratio {dr / dp:.3f}')
    assert dr <= 0.5 * dp


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs(model_root, golden, dev):
    """The scale options, a bad loss, warm starts, a negative round count and a too small workspace are refused by the
    native call before anything is enqueued: pre-filled outputs keep their contents; gradients, ``share_beta_group`` and
    the scale options raise in Python."""
    from smplfitter_amd import _lib

    m, f = get_fitter(model_root, golden, dev, 'smpl')
    B, V, J = 3, m.num_vertices, m.num_joints
    tv, tj = fit_targets(m, B, dev, 13)
    h = m._native(dev)
    ws = torch.empty(h.fit_robust_workspace_bytes(B), dtype=torch.uint8, device=dev)
    new = lambda *sh: torch.full(sh, SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
    outs = dict(pose_rotvecs=new(B, 3 * J), shape_betas=new(B, 10), trans=new(B, 3), orientations=new(B, J, 3, 3),
                relative_orientations=new(B, J, 3, 3), scale_corr=new(B))
    rob = dict(vertex_weights=new(B, V), joint_weights=new(B, J), scale_out=new(B))
    rec = dict(vertex_error=new(B, V), joint_error=new(B, J))
    lib = _lib.load()

    def call(fit_change, robust_change):
        fa = dict(target_vertices=tv.data_ptr(), target_joints=tj.data_ptr(), batch=B, num_iter=1, beta_regularizer=1.0,
                  kid_regularizer=1.0, final_adjust_rots=1, workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                  hip_stream=torch.cuda.current_stream(dev).cuda_stream, **{k: v.data_ptr() for k, v in outs.items()})
        ra = dict(loss=2, tuning=3.0, scale_floor=1e-3, num_rounds=1, **{k: v.data_ptr() for k, v in rob.items()})
        args, rargs = _lib.FitArgs(**{**fa, **fit_change}), _lib.FitRobustArgs(**{**ra, **robust_change})
        rr = _lib.FitReconArgs(**{k: v.data_ptr() for k, v in rec.items()})
        rc = lib.smplfit_fit_robust_f32(h.ptr, C.byref(args), None, C.byref(rr), C.byref(rargs))
        torch.cuda.synchronize(dev)
        return rc

    init = tv.new_zeros(B, 3 * J)
    for fit_change, robust_change, want in (
            (dict(scale_mode=1), {}, _lib.SMPLFIT_ERR_UNSUPPORTED), (dict(scale_mode=2), {}, _lib.SMPLFIT_ERR_UNSUPPORTED),
            ({}, dict(loss=4), _lib.SMPLFIT_ERR_BAD_ARG), ({}, dict(loss=-1), _lib.SMPLFIT_ERR_BAD_ARG),
            ({}, dict(tuning=0.0), _lib.SMPLFIT_ERR_BAD_ARG), ({}, dict(num_rounds=-1), _lib.SMPLFIT_ERR_BAD_ARG),
            ({}, dict(round_num_iter=-1), _lib.SMPLFIT_ERR_BAD_ARG), ({}, dict(scale_floor=0.0), _lib.SMPLFIT_ERR_BAD_ARG),
            (dict(initial_pose_rotvecs=init.data_ptr()), {}, _lib.SMPLFIT_ERR_BAD_ARG),
            (dict(initial_shape_betas=init.data_ptr(), num_initial_betas=10), {}, _lib.SMPLFIT_ERR_BAD_ARG),
            (dict(workspace_bytes=ws.numel() - 256), {}, _lib.SMPLFIT_ERR_WORKSPACE),
            (dict(target_joints=None), {}, _lib.SMPLFIT_ERR_BAD_ARG)):
        assert call(fit_change, robust_change) == want, (fit_change, robust_change, lib.smplfit_last_error())
        for k, v in {**outs, **rob, **rec}.items():
            assert torch.all(v == SENTINEL), (k, fit_change, robust_change)
    assert call({}, {}) == 0  # (the same arguments unchanged are served)
    assert not any(torch.any(v == SENTINEL) for k, v in {**outs, **rob, **rec}.items() if k != 'scale_corr')
    for kw in (dict(scale_target=True), dict(scale_fit=True), dict(share_beta=True, share_beta_group=object()),
               dict(vertex_weights=torch.ones(B, V, device=dev, requires_grad=True))):
        with pytest.raises(NotImplementedError):
            f.fit_robust(tv, tj, **kw)
    with pytest.raises(ValueError, match='loss'):
        f.fit_robust(tv, tj, loss='welsch')
    with pytest.raises(ValueError, match='loss'):
        f._robust_weights(tv[..., 0], loss='welsch')
