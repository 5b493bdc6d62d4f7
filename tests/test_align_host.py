"""Host checks (no GPU) of the aligned errors: ``sf::align_solve`` of sf_rigid.h compiled for the host
(tests/hostemu/hostemu_align_points.cpp) against numpy's fp64 SVD Procrustes, also as a stand-alone program under
AddressSanitizer + UBSan; the C-ABI of the four new entry points on a host-only handle and their refusals; the argument
errors of ``BodyModel.mesh_error`` and ``align_points`` with CPU tensors; ``align_points`` on CPU tensors against numpy.

Bound of the solve (``solve_bound``): the moments are fp64 sums of exact fp32 differences, so what is left is the fp32
copy of K handed to the projection and the fp32 rotation it returns.  Rounding K entrywise (2^-24 relative) perturbs it
by at most 3 * 2^-24 * sigma_1 in Frobenius norm, which turns R by at most that over the gap sigma_2 + d sigma_3, i.e.
1.8e-7 / cond rad; the fp32 rounding of R's entries adds sqrt(3) * 2^-24 = 1.0e-7.  The aligned points therefore lie
within s * (1.8e-7 / cond + 1.0e-7) * (largest distance to the centroid) of the arbiter's, plus, for fp32 inputs far
from the origin, nothing: the differences are exact.  Collinear clouds: the rotation about the line is free and does
not move the points, the gap that matters is sigma_1 itself (cond = 1)."""

import ctypes as C
import os
import os.path as osp
import re
import subprocess

import numpy as np
import pytest
import torch

import align_util as A
import hostemu_util as H
import util
from smplfitter_amd import _lib, build

HERE = osp.dirname(osp.abspath(__file__))
CSRC = osp.join(HERE, '..', 'smplfitter_amd', 'csrc')
SRC = osp.join(HERE, 'hostemu', 'hostemu_align_points.cpp')
BUILD = osp.join(HERE, 'hostemu', '_build')
SO = osp.join(BUILD, 'libhostemu_align_points.so')
EXE = osp.join(BUILD, 'align_solve_asan_static')
DEPS = [SRC] + [osp.join(CSRC, f) for f in ('sf_rigid.h', 'sf_math.h', 'sf_stages.h')]
SYMBOLS = ('smplfit_mesh_error_aligned_workspace_bytes', 'smplfit_mesh_error_aligned_f32',
           'smplfit_align_points_workspace_bytes', 'smplfit_align_points_f32')
SOLVE_MODES = ('translation', 'rigid', 'similarity')


def _stale(out, deps):
    return not osp.exists(out) or any(osp.getmtime(d) > osp.getmtime(out) for d in deps)


@pytest.fixture(scope='module')
def emu():
    """The host build of the SF_HD solve, as the other host emulations are built (g++, -ffp-contract=off)."""
    if _stale(SO, DEPS):
        os.makedirs(BUILD, exist_ok=True)
        tmp = SO + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', SRC, '-o', tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    vp, i32 = C.c_void_p, C.c_int
    lib.hostemu_align_points.argtypes = [i32, vp, vp, vp, i32, vp]
    lib.hostemu_align_points.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def emu_solve(emu, mode, x, y, w):
    """(s, R, t, c) of the host build for one cloud x, y (N, 3) fp32."""
    out = np.full(16, 7.0)
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    w = None if w is None else np.ascontiguousarray(w, np.float32)
    emu.hostemu_align_points(_lib.ALIGN_MODES[mode], _p(x), _p(y), _p(w), len(x), _p(out))
    return out[0], out[1:10].reshape(3, 3), out[10:13], out[13:16]


def rotation(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q * np.sign(np.linalg.det(q))


def clouds(kind, n, rs):
    """(x, y, w, collinear) fp32: y is x under a seeded similarity plus 1 % noise."""
    p = rs.randn(n, 3) * (1.0, 0.6, 0.3)
    if kind == 'coplanar':
        p[:, 2] = 0.0
    if kind == 'collinear':
        p[:, 1:] = 0.0
    R, s, t = rotation(rs), rs.uniform(0.7, 1.4), rs.randn(3) * 3
    q = p * (-1.0, 1.0, 1.0) if kind == 'mirrored' else p
    y = s * q @ R.T + t + rs.randn(n, 3) * (0.0 if kind in ('coplanar', 'collinear') else 0.01)
    x = p @ rotation(rs).T
    if kind == 'far':
        x, y = x + (1000.0, -1000.0, 1000.0), y + (-1000.0, 1000.0, 1000.0)
    w = None if kind == 'unweighted' else rs.uniform(0.1, 2.0, n)
    return x.astype(np.float32), y.astype(np.float32), w if w is None else w.astype(np.float32), kind == 'collinear'


def solve_bound(s, cond, size):
    return s * (1.8e-7 / cond + 1.0e-7) * size


@pytest.mark.parametrize('kind', ['random', 'unweighted', 'mirrored', 'coplanar', 'collinear', 'far'])
@pytest.mark.parametrize('mode', SOLVE_MODES)
def test_solve_against_svd(emu, kind, mode):
    """The aligned points of the host build against those of the fp64 SVD arbiter, inside ``solve_bound``; det R = +1 and
    R^T R = I to 1e-6; the centred offset c reproduces t (t = c + oy - s R ox).  Every case but the collinear one has
    cond >= 0.05, asserted on the arbiter's numbers."""
    rs = np.random.RandomState(len(kind) * 7 + len(mode))
    for n in (3, 8, 24, 1000):
        x, y, w, collinear = clouds(kind, n, rs)
        if n == 3 and kind != 'collinear':
            continue  # (three seeded points can lie almost on a line, where cond is not bounded below)
        ref = A.procrustes64(x[None], y[None], None if w is None else w[None], mode)
        s, R, t, c = emu_solve(emu, mode, x, y, w)
        cond = 1.0 if collinear or mode == 'translation' else float(ref['cond'][0])
        assert cond >= 0.05, (kind, n, cond)
        x64 = x.astype(np.float64)
        xm = x64.mean(0) if w is None else (w[:, None] * x64).sum(0) / w.sum()
        size = np.linalg.norm(x64 - xm, axis=-1).max()
        ours = s * x64 @ R.T + t
        want = A.move64(x[None], ref)[0]
        worst, bound = np.linalg.norm(ours - want, axis=-1).max(), solve_bound(ref['s'][0], cond, size)
        print(f'[align-host] {kind} {mode} n = {n}: cond {cond:.3f}, worst {worst:.2e} m, bound {bound:.2e} m')
        assert worst <= bound, (kind, mode, n, worst, bound)
        assert np.linalg.det(R) > 0 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-6
        ox, oy = x[0].astype(np.float64), y[0].astype(np.float64)
        assert np.abs(c + oy - s * R @ ox - t).max() <= 1e-9 * max(1.0, np.abs(t).max())
        if mode != 'similarity':
            assert s == 1.0
        if mode == 'translation':
            assert np.array_equal(R, np.eye(3))


@pytest.mark.parametrize('mode', SOLVE_MODES)
def test_solve_nan_rows(emu, mode):
    """Zero total weight, a negative weight's NaN sum, a non-finite point: every output NaN.  No spread: NaN under
    'similarity' alone."""
    rs = np.random.RandomState(5)
    x, y = rs.randn(6, 3).astype(np.float32), rs.randn(6, 3).astype(np.float32)
    for w in (np.zeros(6, np.float32), np.array([1, 1, np.nan, 1, 1, 1], np.float32)):
        assert all(np.isnan(v).all() for v in emu_solve(emu, mode, x, y, w)), mode
    bad = x.copy()
    bad[2, 1] = np.inf
    assert all(np.isnan(v).all() for v in emu_solve(emu, mode, bad, y, None))
    assert all(np.isnan(v).all() for v in emu_solve(emu, mode, x, bad, None))
    same = np.tile(x[:1], (6, 1))
    out = emu_solve(emu, mode, same, y, None)
    assert all(np.isnan(v).all() for v in out) if mode == 'similarity' else all(np.isfinite(v).all() for v in out)


def test_solve_sanitized():
    """The same solve in a stand-alone program under -fsanitize=address,undefined (runtimes linked statically), in
    buffers of exactly n points.  Nothing loaded into Python is sanitized."""
    if _stale(EXE, DEPS):
        os.makedirs(BUILD, exist_ok=True)
        tmp = EXE + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O1', '-g', '-DALIGN_MAIN', '-fsanitize=address,undefined', '-static-libasan',
                        '-static-libubsan', '-fno-omit-frame-pointer', '-fno-sanitize-recover=undefined', '-std=c++17',
                        '-ffp-contract=off', SRC, '-o', tmp], check=True)
        os.replace(tmp, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'FAIL' not in r.stdout and r.stdout.count('ok   solve ') == 46


@pytest.fixture(scope='module')
def lib():
    build.build(verbose=False)
    return _lib.load()


def header_fields(hdr, name):
    body = re.search(r'typedef struct ' + name + r' \{(.*?)\} ' + name + ';', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        names = re.sub(r'^\s*(const\s+)?\w+\s*\**', '', decl.strip())
        fields += [n.strip(' *') for n in names.split(',') if n.strip(' *')]
    return fields


def test_symbols_and_structs(lib):
    """The new symbols are declared, exported and bound; the ABI version is unchanged; the binding's structs have the
    header's fields in the header's order; the mode numbers are the header's."""
    hdr = open(osp.join(HERE, '..', 'include', 'smplfit.h')).read()
    assert '#define SMPLFIT_ABI_VERSION 7' in hdr and lib.smplfit_abi_version() == 7 == _lib.SMPLFIT_ABI_VERSION
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(rf'\b{s}\s*\(', hdr), s
    for name, cls in (('smplfit_mesh_align_args', _lib.MeshAlignArgs), ('smplfit_align_points_args', _lib.AlignPointsArgs)):
        assert header_fields(hdr, name) == [f[0] for f in cls._fields_], name
    for k, v in _lib.ALIGN_MODES.items():
        assert re.search(rf'SMPLFIT_ALIGN_{k.upper()} = {v},', hdr), k
    for k, v in _lib.ALIGN_ON.items():
        assert re.search(rf'SMPLFIT_ALIGN_ON_{k.upper()} = {v},', hdr), k
    assert tuple(_lib.ALIGN_MODES) == A.MODES


def test_workspace_queries(lib, model_root, golden):
    """On a host-only handle: the aligned step takes the mesh-error step's workspace, then the mesh, both error arrays,
    the slab moments (17 doubles per slab of 2048 points and row) and the two records (18 floats a row), each 256-byte
    aligned.  The point query is the moments, the record and the errors.  0 for counts that are not served."""
    kind, md = util.load_md(model_root, 'smpl', golden('smpl'))
    desc, keep = H.desc_from_md(md, kind)
    h = _lib.Handle(desc, host_only=True)
    r = lambda n: (n + 255) // 256 * 256  # noqa: E731
    V, J = h.info.num_vertices, h.info.num_joints
    slabs = lambda n: (n + 2047) // 2048  # noqa: E731
    for B in (1, 64, 65, 129, 1795):
        own = r(12 * B * V) + r(4 * B * V) + r(4 * B * J) + r(8 * 17 * slabs(V) * B) + r(8 * 17 * slabs(J) * B) + 2 * r(72 * B)
        assert h.mesh_error_aligned_workspace_bytes(B) == r(h.mesh_error_workspace_bytes(B)) + own
        for N in (1, 17, 2048, 2049, 6890):
            assert lib.smplfit_align_points_workspace_bytes(B, N) == r(8 * 17 * slabs(N) * B) + r(72 * B) + r(4 * B * N)
    assert h.mesh_error_aligned_workspace_bytes(0) == 0 and lib.smplfit_mesh_error_aligned_workspace_bytes(None, 4) == 0
    for B, N in ((0, 5), (5, 0), (-1, 5), (5, (1 << 26) + 1), ((1 << 12) + 1, 1 << 26)):
        assert lib.smplfit_align_points_workspace_bytes(B, N) == 0
    h.close()
    del keep


def test_refusals(lib, model_root, golden):
    """Every refusal of the two entries, none of which needs a device: they are answered before the handle's device is
    asked for (a host-only handle then gives SMPLFIT_ERR_HIP where the arguments are in order)."""
    kind, md = util.load_md(model_root, 'smpl', golden('smpl'))
    desc, keep = H.desc_from_md(md, kind)
    h = _lib.Handle(desc, host_only=True)
    bad, fn = _lib.SMPLFIT_ERR_BAD_ARG, lib.smplfit_mesh_error_aligned_f32
    P = 1 << 20  # (a pointer value that is never followed)
    base = dict(batch=4, target_vertices=P, target_joints=P, vertex_error=P)
    ok = dict(align=4, align_on=0)
    cases = [
        (base, dict(ok, align=5), b'unknown align'), (base, dict(ok, align=-1), b'unknown align'),
        (base, dict(ok, align_on=3), b'align_on'), (base, dict(ok, align_on=-1), b'align_on'),
        (dict(base, target_vertices=None), ok, b'target_vertices'),
        (dict(base, target_joints=None), dict(ok, align=1), b'root'),
        (dict(base, target_joints=None), dict(ok, align_on=2), b'align_on = joints'),
        (dict(base, target_joints=None, joint_error=P), ok, b'target_joints'),
        (dict(base, target_joints=None), dict(ok, mean_joint_error=P), b'target_joints'),
        (dict(base, target_joints=None), dict(ok, joint_rotation=P), b'target_joints'),
        (dict(base, target_joints=None), dict(ok, joint_weights=P), b'target_joints'),
        (dict(base, vertex_error=None), ok, b'at least one output'),
        (base, dict(ok, align=0, scale=P), b'none'),
        (base, dict(ok, align_on=1, joint_scale=P), b'each'), (base, dict(ok, align=1, joint_translation=P), b'each'),
    ]
    for a, al, text in cases:
        rc = fn(h.ptr, C.byref(_lib.MeshErrorArgs(**a)), C.byref(_lib.MeshAlignArgs(**al)))
        assert rc == bad and text in lib.smplfit_last_error(), (a, al, lib.smplfit_last_error())
    assert fn(h.ptr, None, C.byref(_lib.MeshAlignArgs(**ok))) == bad
    assert fn(None, C.byref(_lib.MeshErrorArgs(**base)), C.byref(_lib.MeshAlignArgs(**ok))) == bad  # (null handle)
    assert fn(h.ptr, C.byref(_lib.MeshErrorArgs(**base)), C.byref(_lib.MeshAlignArgs(**ok))) == _lib.SMPLFIT_ERR_HIP
    assert fn(h.ptr, C.byref(_lib.MeshErrorArgs(**base)), None) == _lib.SMPLFIT_ERR_HIP  # (smplfit_mesh_error_f32)
    assert fn(h.ptr, None, None) == bad
    h.close()
    del keep
    fp, okp = lib.smplfit_align_points_f32, dict(batch=2, num_points=5, source=P, target=P, align=4, error=P)
    for change, text in ((dict(batch=0), b'batch'), (dict(num_points=0), b'num_points'), (dict(source=None), b'required'),
                         (dict(target=None), b'required'), (dict(align=0), b'align'), (dict(align=1), b'align'),
                         (dict(align=5), b'align'), (dict(error=None), b'at least one output'),
                         (dict(num_points=(1 << 26) + 1), b'num_points'),
                         (dict(batch=(1 << 12) + 1, num_points=1 << 26), b'2^38')):
        assert fp(C.byref(_lib.AlignPointsArgs(**{**okp, **change}))) == bad, change
        assert text in lib.smplfit_last_error(), (change, lib.smplfit_last_error())
    assert fp(None) == bad
    assert fp(C.byref(_lib.AlignPointsArgs(**okp))) == _lib.SMPLFIT_ERR_WORKSPACE  # (no workspace: still nothing enqueued)
    assert fp(C.byref(_lib.AlignPointsArgs(**okp, workspace=P, workspace_bytes=256))) == _lib.SMPLFIT_ERR_WORKSPACE


@pytest.fixture(scope='module')
def cpu_model(model_root):
    from smplfitter_amd.pt import BodyModel

    return BodyModel('smpl', 'neutral', model_root=f'{model_root}/{util.model_dir("smpl")}', num_betas=10)


def test_python_argument_errors(cpu_model):
    """``mesh_error`` and ``align_points`` with CPU tensors: unknown strings, 'root' / 'joints' without target joints and
    wrong shapes are ValueError before a device is looked at."""
    from smplfitter_amd.pt import align_points

    m = cpu_model
    B, J, V = 4, m.num_joints, m.num_vertices
    tv, tj, pose = torch.zeros(B, V, 3), torch.zeros(B, J, 3), torch.zeros(B, 3 * J)
    for kw in (dict(align='procrustes'), dict(align=None), dict(align='rigid', align_on='both'), dict(align='root'),
               dict(align='rigid', align_on='joints'), dict(joint_weights=torch.ones(B, J)),
               dict(vertex_weights=torch.ones(B, V + 1)), dict(align='rigid', vertex_weights=torch.ones(B + 1, V)),
               dict(vertex_weights=torch.ones(V))):
        with pytest.raises(ValueError):
            m.mesh_error(tv, pose_rotvecs=pose, **kw)
    for kw in (dict(joint_weights=torch.ones(B, J + 1)), dict(align='similarity', joint_weights=torch.ones(B))):
        with pytest.raises(ValueError):
            m.mesh_error(tv, tj, pose_rotvecs=pose, **kw)
    with pytest.raises(ValueError):
        m.mesh_error(tv[:, :-1], tj, pose_rotvecs=pose, align='rigid')
    with pytest.raises(ValueError):
        m.mesh_error(tv, tj[:, :-1], pose_rotvecs=pose, align='root')
    with pytest.raises(ValueError, match='Only one rotation input'):
        m.mesh_error(tv, tj, pose_rotvecs=pose, glob_rotmats=torch.zeros(B, J, 3, 3), align='rigid')
    with pytest.raises(TypeError):
        m.mesh_error(tv, tj, pose_rotvecs=pose, align='rigid', vertex_weights=np.ones((B, V)))
    x = torch.zeros(B, 7, 3)
    for args, kw in (((x, x), dict(align='none')), ((x, x), dict(align='root')), ((x, x), dict(align='affine')),
                     ((x[0], x[0]), {}), ((x, x[:, :-1]), {}), ((x, x[:-1]), {}), ((x, x, torch.ones(B, 6)), {}),
                     ((x, x, torch.ones(B)), {}), ((x[:, :0], x[:, :0]), {}), ((torch.zeros(B, 7, 2), torch.zeros(B, 7, 2)), {})):
        with pytest.raises(ValueError):
            align_points(*args, **kw)
    with pytest.raises(TypeError):
        align_points(x.numpy(), x)


@pytest.mark.parametrize('mode', SOLVE_MODES)
def test_align_points_cpu(mode):
    """``align_points`` on CPU float32 tensors (the composed route: fp64 inside) against numpy fp64, 1e-5 relative on the
    errors, means and the transform's effect; a zero-weight row and a NaN row are NaN in that row alone."""
    from smplfitter_amd.pt import align_points

    rs = np.random.RandomState(3)
    B, N = 5, 40
    x = rs.randn(B, N, 3).astype(np.float32)
    y = np.stack([rs.uniform(0.7, 1.4) * x[b] @ rotation(rs).T + rs.randn(3) * 3 for b in range(B)]) + rs.randn(B, N, 3) * 0.01
    y = y.astype(np.float32)
    w = rs.uniform(0.1, 2.0, (B, N)).astype(np.float32)
    w[3] = 0.0
    y[4, 7, 1] = np.nan
    for weights in (None, w):
        res = align_points(torch.from_numpy(x), torch.from_numpy(y), None if weights is None else torch.from_numpy(weights), align=mode)
        assert sorted(res) == ['error', 'mean_error', 'rotation', 'scale', 'translation']
        assert all(v.dtype == torch.float32 for v in res.values())
        ref = A.procrustes64(x, y, weights, mode)
        e = A.errors64(x, y, ref)
        dead = [4] if weights is None else [3, 4]
        live = [b for b in range(B) if b not in dead]
        ours = {k: v.numpy().astype(np.float64) for k, v in res.items()}
        for k in ours:
            assert np.isnan(ours[k][dead]).all() and np.isfinite(ours[k][live]).all(), (mode, k)
        assert np.allclose(ours['error'][live], e[live], rtol=1e-5, atol=0)
        assert np.allclose(ours['mean_error'][live], A.row_mean64(e, weights)[live], rtol=1e-5, atol=0)
        mine = A.errors64(x, y, dict(s=ours['scale'], R=ours['rotation'], t=ours['translation']))
        # (the fp32 transform moves a point of size ~3 by up to 3e-7 * 3; the errors are ~2e-2)
        assert np.allclose(mine[live], e[live], rtol=1e-4, atol=0)
