"""Host checks (no GPU) of the robust reweighting and ``BodyFitter.fit_robust``: the per-element functions
of sf_math.h that ``k_robust_reweight`` calls, compiled for the host (tests/hostemu/hostemu_robust.cpp), against numpy;
a serial radix select built from the same key / digit functions against ``np.sort``, also as a stand-alone program
under AddressSanitizer + UBSan; the C-ABI of the three new entry points on a host-only handle; the argument errors of
``BodyFitter`` with CPU tensors."""

import ctypes as C
import os
import os.path as osp
import re
import subprocess

import numpy as np
import pytest
import torch

import robust_util as R
import util
from smplfitter_amd import _lib, build

HERE = osp.dirname(osp.abspath(__file__))
CSRC = osp.join(HERE, '..', 'smplfitter_amd', 'csrc')
SRC = osp.join(HERE, 'hostemu', 'hostemu_robust.cpp')
BUILD = osp.join(HERE, 'hostemu', '_build')
SO = osp.join(BUILD, 'libhostemu_robust.so')
EXE = osp.join(BUILD, 'robust_select_asan_static')
SYMBOLS = ('smplfit_robust_weights_f32', 'smplfit_fit_robust_workspace_bytes', 'smplfit_fit_robust_f32')
U = np.array([0, 1e-6, 0.5, 1 - 1e-7, 1, 1 + 1e-7, 10, 1e6], np.float32)


def _stale(out, deps):
    return not osp.exists(out) or any(osp.getmtime(d) > osp.getmtime(out) for d in deps)


@pytest.fixture(scope='module')
def emu():
    """The host build of the SF_HD functions, as the other host emulations are built (g++, -ffp-contract=off)."""
    if _stale(SO, [SRC, osp.join(CSRC, 'sf_math.h')]):
        os.makedirs(BUILD, exist_ok=True)
        tmp = SO + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', SRC, '-o', tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    vp, i32, f32, u32 = C.c_void_p, C.c_int, C.c_float, C.c_uint32
    lib.hostemu_robust_keys.argtypes = [vp, vp, i32]
    lib.hostemu_robust_digit.argtypes = [u32, i32]
    lib.hostemu_robust_digit.restype = u32
    lib.hostemu_robust_scale.argtypes = [f32, f32]
    lib.hostemu_robust_scale.restype = f32
    lib.hostemu_robust_psi.argtypes = [i32, vp, vp, i32]
    lib.hostemu_robust_weight.argtypes = [i32, vp, vp, i32]
    lib.hostemu_robust_select.argtypes = [vp, vp, i32, C.POINTER(f32)]
    lib.hostemu_robust_select.restype = i32
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize('loss', R.LOSSES)
def test_weight_functions(emu, loss):
    """psi(u) of the host build against numpy fp64 at the edges of every branch.  Bound: psi <= 1 and at most four fp32
    roundings (u * u, 1 + ., the square, the quotient), each <= 2^-24 relative: 4 * 6e-8 = 2.4e-7, gated at 5e-7
    absolute; Tukey is exactly 0 from u = 1 on, Huber exactly 1 up to u = 1; the dispatch the kernel calls gives the
    same bits as the four functions."""
    w, w2 = np.full(U.shape, np.nan, np.float32), np.full(U.shape, np.nan, np.float32)
    emu.hostemu_robust_psi(_lib.ROBUST_LOSSES[loss], _p(U), _p(w), len(U))
    emu.hostemu_robust_weight(_lib.ROBUST_LOSSES[loss], _p(U), _p(w2), len(U))
    want = R.psi(loss, U.astype(np.float64))
    print(loss, w, np.abs(w - want).max())
    assert np.array_equal(w, w2)
    assert np.abs(w - want).max() <= 5e-7
    if loss == 'tukey':
        assert np.all(w[U >= 1] == 0) and w[0] == 1
    if loss == 'huber':
        assert np.all(w[U <= 1] == 1)
    assert np.all((w >= 0) & (w <= 1))
    assert R.TUNING == _lib.ROBUST_TUNING and tuple(_lib.ROBUST_LOSSES) == R.LOSSES


def test_key_order(emu):
    """On sorted non-negative floats — zero, denormals, normals, inf — the keys are sorted as unsigned integers, equal
    exactly where the floats are; NaN lies above inf; the four digits of a key, most significant first, rebuild it;
    the sign bit is dropped."""
    rs = np.random.RandomState(1)
    tiny = np.float32(1e-45)
    x = np.concatenate([[0.0, tiny, 2 * tiny, np.finfo(np.float32).tiny, np.finfo(np.float32).max, np.inf],
                        rs.rand(500), np.exp(rs.randn(500) * 20), rs.rand(50) * 1e-40]).astype(np.float32)
    x = np.sort(np.concatenate([x, x[:100]]))
    keys = np.zeros(x.shape, np.uint32)
    emu.hostemu_robust_keys(_p(x), _p(keys), len(x))
    assert np.all(np.diff(keys.astype(np.int64)) >= 0)
    assert np.array_equal(keys[1:] == keys[:-1], x[1:] == x[:-1])
    assert np.array_equal(keys, x.view(np.uint32))
    special = np.array([np.inf, np.nan, -0.0, -1.5], np.float32)
    k = np.zeros(4, np.uint32)
    emu.hostemu_robust_keys(_p(special), _p(k), 4)
    assert k[1] > k[0] == 0x7F800000 and k[2] == 0 and k[3] == np.float32(1.5).view(np.uint32)
    for key in (0, 1, 0x3F800000, 0x7F800000, 0x12345678):
        d = [emu.hostemu_robust_digit(key, p) for p in range(4)]
        assert (d[0] << 24 | d[1] << 16 | d[2] << 8 | d[3]) == key and all(v < 256 for v in d)
    assert emu.hostemu_robust_scale(1.0, 1e-3) == np.float32(1.4826) * np.float32(1.0)
    assert emu.hostemu_robust_scale(1e-6, 1e-3) == np.float32(1e-3) and emu.hostemu_robust_scale(0.0, 0.25) == 0.25


@pytest.mark.parametrize('n', [1, 2, 3, 64, 65, 6890])
def test_radix_select(emu, n):
    """The serial select over four 8-bit digits equals ``np.sort(x)[(n - 1) // 2]`` to the bit: seeded errors, heavy
    ties, all equal, half zeros, and with prior weights a third of which are zero."""
    rs = np.random.RandomState(n)
    cases = dict(random=(rs.rand(n) ** 2 * 0.3), ties=np.floor(rs.rand(n) * 4) / 4, equal=np.full(n, 0.0123),
                 halfzero=np.where(np.arange(n) % 2, rs.rand(n), 0.0), zero=np.zeros(n))
    for name, x in cases.items():
        x = x.astype(np.float32)
        for w0 in (None, np.where(np.arange(n) % 3 == 0, 0.0, rs.rand(n) + 0.1).astype(np.float32)):
            med = C.c_float(-1)
            cnt = emu.hostemu_robust_select(_p(x), _p(w0), n, C.byref(med))
            want, wcnt = R.lower_median(x[None], None if w0 is None else w0[None])
            assert cnt == wcnt[0], (name, n)
            if cnt:
                assert np.float32(med.value).view(np.uint32) == want[0].view(np.uint32), (name, n, med.value, want[0])


def test_radix_select_sanitized():
    """The same select in a stand-alone program under -fsanitize=address,undefined (runtimes linked statically): every
    buffer holds exactly n floats, so an index past the row is a report.  Nothing loaded into Python is sanitized."""
    if _stale(EXE, [SRC, osp.join(CSRC, 'sf_math.h')]):
        os.makedirs(BUILD, exist_ok=True)
        tmp = EXE + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O1', '-g', '-DROBUST_MAIN', '-fsanitize=address,undefined', '-static-libasan',
                        '-static-libubsan', '-fno-omit-frame-pointer', '-fno-sanitize-recover=undefined', '-std=c++17',
                        '-ffp-contract=off', SRC, '-o', tmp], check=True)
        os.replace(tmp, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'FAIL' not in r.stdout and r.stdout.count('ok   select ') == 36


@pytest.fixture(scope='module')
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_cabi(lib):
    """The new symbols are declared in the header, exported and bound; the ABI version and the argument struct of the fit
    are unchanged; the step refuses bad options before it looks at a pointer's contents, the fit before it looks at a
    handle."""
    hdr = open(osp.join(HERE, '..', 'include', 'smplfit.h')).read()
    assert '#define SMPLFIT_ABI_VERSION 7' in hdr and lib.smplfit_abi_version() == 7
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(rf'\b{s}\s*\(', hdr), s
    assert re.search(r'smplfit_fit_robust_f32\(const smplfit_handle\* h, const smplfit_fit_args\* args,', hdr)
    bad = _lib.SMPLFIT_ERR_BAD_ARG
    assert lib.smplfit_robust_weights_f32(None) == bad
    ok = dict(batch=2, num_vertex_errors=5, vertex_error=1 << 20, out_vertex_weights=1 << 21, loss=2, tuning=3.0,
              scale_floor=1e-3)
    for change, text in ((dict(batch=0), b'batch'), (dict(num_vertex_errors=0), b'num_vertex_errors'),
                         (dict(vertex_error=None), b'required'), (dict(out_vertex_weights=None), b'required'),
                         (dict(loss=4), b'loss'), (dict(loss=-1), b'loss'), (dict(tuning=0.0), b'tuning'),
                         (dict(tuning=float('nan')), b'tuning'), (dict(scale=-1.0), b'scale'),
                         (dict(scale=1.0, scale_rows=1 << 22), b'scale_rows'), (dict(scale_floor=0.0), b'scale_floor'),
                         (dict(joint_error=1 << 22), b'num_joint_errors'),
                         (dict(joint_error=1 << 22, num_joint_errors=3), b'out_joint_weights'),
                         (dict(joint_weights=1 << 22), b'joint_error')):
        a = _lib.RobustWeightsArgs(**{**ok, **change})
        assert lib.smplfit_robust_weights_f32(C.byref(a)) == bad, change
        assert text in lib.smplfit_last_error(), (change, lib.smplfit_last_error())
    fa, ra = _lib.FitArgs(batch=4), _lib.FitRobustArgs(loss=2, tuning=3.0, scale_floor=1e-3, num_rounds=1)
    assert lib.smplfit_fit_robust_f32(None, None, None, None, C.byref(ra)) == bad
    assert lib.smplfit_fit_robust_f32(None, C.byref(fa), None, None, None) == bad
    assert lib.smplfit_fit_robust_f32(None, C.byref(fa), None, None, C.byref(ra)) == bad  # (null handle)
    assert b'handle' in lib.smplfit_last_error()
    p = _lib.ShareSegments([2, 3], host_only=True)
    assert lib.smplfit_fit_robust_f32(None, C.byref(fa), p.ptr, None, C.byref(ra)) == bad
    assert b"plan's" in lib.smplfit_last_error()
    assert lib.smplfit_fit_robust_workspace_bytes(None, 4, None) == 0
    p.close()


def test_workspace_query_host_only(lib, model_root):
    """On a host-only handle: the query is the reconstruction's plus the errors, weights, scales and the carried pose
    (256-byte aligned regions), with and without a plan of segments, and 0 for a batch that is not the plan's."""
    md = util.load_md(model_root, 'smpl', None)[1]
    desc, keep = _lib.make_desc(md.v_template, md.shapedirs, md.posedirs, md.weights, md.J_template, md.J_shapedirs,
                                md.kintree_parents, md.J_regressor_post_lbs)
    h = _lib.Handle(desc, host_only=True)
    p = _lib.ShareSegments([2, 3], host_only=True)
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    V, J = md.num_vertices, md.num_joints
    for B, plan in ((5, None), (5, p), (64, None)):
        own = 2 * up(B * V * 4) + 2 * up(B * J * 4) + up(B * 4) + up(B * J * 3 * 4)
        assert h.fit_robust_workspace_bytes(B, plan) == h.fit_recon_workspace_bytes(B, plan) + own
        assert h.fit_robust_workspace_bytes(B, plan) >= h.fit_recon_workspace_bytes(B, plan) > 0
    assert h.fit_robust_workspace_bytes(6, p) == 0 and h.fit_robust_workspace_bytes(0) == 0
    p.close()
    del keep


@pytest.fixture(scope='module')
def cpu_fitter(model_root):
    from smplfitter_amd.pt import BodyFitter, BodyModel

    m = BodyModel('smpl', 'neutral', model_root=f'{model_root}/{util.model_dir("smpl")}', num_betas=10)
    return m, BodyFitter(m)


def test_python_argument_errors(cpu_fitter):
    """``fit_robust`` and ``_robust_weights`` with CPU tensors, no device: wrong shapes, an unknown loss and bad numbers
    are ValueError; the scale options, ``share_beta_group`` and inputs that require grad NotImplementedError — all
    before the device is looked at."""
    m, f = cpu_fitter
    B, V, J = 4, m.num_vertices, m.num_joints
    tv, tj = torch.zeros(B, V, 3), torch.zeros(B, J, 3)
    for kw in (dict(loss='l2'), dict(loss=None), dict(tuning=0), dict(tuning=-1.0), dict(tuning=float('inf')),
               dict(scale=0.0), dict(scale=-2.0), dict(scale=float('nan')), dict(scale=torch.ones(B + 1)),
               dict(scale=torch.ones(B, 1)), dict(scale=torch.ones(B, dtype=torch.int64)), dict(scale_floor=0.0),
               dict(scale_floor=-1e-3), dict(num_rounds=-1), dict(num_iter=0), dict(round_num_iter=0),
               dict(vertex_weights=torch.ones(B, V + 1)), dict(joint_weights=torch.ones(B, J + 1)),
               dict(target_joints=torch.zeros(B, J + 1, 3)), dict(share_beta_segments=[3, 2]),
               dict(requested_keys=['joint_error'])):
        with pytest.raises(ValueError):
            f.fit_robust(tv, **kw)
    with pytest.raises(ValueError):
        f.fit_robust(torch.zeros(B, V + 1, 3))
    for kw in (dict(scale_target=True), dict(scale_fit=True), dict(share_beta=True, share_beta_group=object()),
               dict(vertex_weights=torch.ones(B, V, requires_grad=True)),
               dict(scale=torch.ones(B, requires_grad=True))):
        with pytest.raises(NotImplementedError):
            f.fit_robust(tv, tj, **kw)
    with pytest.raises(NotImplementedError):
        f.fit_robust(tv.clone().requires_grad_(True))
    ev = torch.zeros(B, 7)
    for args, kw in (((torch.zeros(7),), {}), ((torch.zeros(B, 0),), {}), ((ev, torch.zeros(B + 1, 3)), {}),
                     ((ev, None, torch.ones(B, 6)), {}), ((ev, None, None, torch.ones(B, 3)), {}),
                     ((ev, torch.zeros(B, 3), None, torch.ones(B, 4)), {}), ((ev,), dict(loss='welsch')),
                     ((ev,), dict(tuning=0.0)), ((ev,), dict(scale=torch.ones(B - 1))), ((ev,), dict(scale_floor=0.0))):
        with pytest.raises(ValueError):
            f._robust_weights(*args, **kw)
    # (a fixed or per-row scale needs no floor)
    assert f._robust_options('tukey', None, 0.5, 0.0, B) == (3, 4.685, 0.5, None, 0.0)
    assert f._robust_options('huber', 2.0, None, 1e-3, B)[:3] == (0, 2.0, 0.0)
