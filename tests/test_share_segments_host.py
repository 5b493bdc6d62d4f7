"""Host checks (no GPU) of ``share_beta`` over segments of the batch: the table builder and the order of
the segmented sum in a stand-alone program under AddressSanitizer + UBSan, the C-ABI of the new entry points on a
host-only plan, and the argument errors of ``BodyFitter`` with CPU tensors."""

import copy
import ctypes as C
import os
import os.path as osp
import re
import subprocess

import numpy as np
import pytest
import torch

import util
from smplfitter_amd import _lib, build

HERE = osp.dirname(osp.abspath(__file__))
CSRC = osp.join(HERE, '..', 'smplfitter_amd', 'csrc')
MAIN = osp.join(HERE, 'hostemu', 'share_segments_main.cpp')
EXE = osp.join(HERE, 'hostemu', '_build', 'share_segments_asan_static')
MIXED = [1, 63, 64, 65, 7, 129, 8, 2]
SYMBOLS = ('smplfit_share_segments_create', 'smplfit_share_segments_destroy', 'smplfit_share_segments_batch',
           'smplfit_share_segments_get_table', 'smplfit_share_segments_workspace_bytes', 'smplfit_fit_segments_f32',
           'smplfit_shape_solve_segments_f32')


@pytest.fixture(scope='module')
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def program():
    """The stand-alone program, built with -fsanitize=address,undefined, and its output."""
    deps = [MAIN, osp.join(CSRC, 'sf_tables.cpp'), osp.join(CSRC, 'sf_tables.h'), osp.join(CSRC, 'sf_math.h')]
    if not osp.exists(EXE) or any(osp.getmtime(d) > osp.getmtime(EXE) for d in deps):
        os.makedirs(osp.dirname(EXE), exist_ok=True)
        tmp = EXE + f'.tmp{os.getpid()}'
        # the sanitizer runtimes are linked in statically: the program then runs in whatever environment it is given
        subprocess.run(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan',
                        '-fno-omit-frame-pointer', '-fno-sanitize-recover=undefined', '-std=c++17', MAIN,
                        osp.join(CSRC, 'sf_tables.cpp'), '-o', tmp], check=True)
        os.replace(tmp, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    return r


def test_tables_sanitized(program):
    """``sf::build_share_segments`` on ``[1]``, ``[4096]``, ``[1] * 4096``, ``[1,63,64,65,7,129,8,2]`` and six seeded
    layouts: every table index in range, the blocks tile each segment in order without gap or overlap, block counts =
    ceil(n / 64); bad sizes refused and nothing left behind.  A wrong index here would be an out-of-bounds read of a
    kernel, so it is settled on the host."""
    assert program.returncode == 0, program.stdout + program.stderr
    assert 'FAIL' not in program.stdout
    assert program.stdout.count('ok   tables ') == 10 and 'ok   refusals' in program.stdout


def test_sum_order_sanitized(program):
    """The segmented two-level sum over random fp64 records (the driver's walk of the block list, blocks and segments
    summed by the kernels' own ``sf::sum_rows_f64``) equals, bit for bit, the same sum of every segment alone —
    whatever the room of the system buffer (the general path's 256-row chunk among them) — and the single segment
    equals the table-free arithmetic of a call without a plan."""
    assert program.returncode == 0, program.stdout + program.stderr
    assert program.stdout.count('ok   sum ') == 5


def test_python_tables_match_definition():
    """The getters (``_lib.ShareSegments.table``) return the tables of the definition, computed here in numpy."""
    rs = np.random.RandomState(3)
    for sizes in ([1], [4096], [1] * 70, MIXED, list(rs.randint(1, 200, 30))):
        p = _lib.ShareSegments(sizes, host_only=True)
        assert p.batch == sum(sizes)
        nb = [(n + 63) // 64 for n in sizes]
        first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        np.testing.assert_array_equal(p.table('row_seg'), np.repeat(np.arange(len(sizes)), sizes))
        np.testing.assert_array_equal(p.table('seg_blk').reshape(-1, 2),
                                      np.stack([np.concatenate([[0], np.cumsum(nb)[:-1]]), nb], 1))
        blk = [(f + 64 * k, min(64, n - 64 * k)) for f, n, b in zip(first, sizes, nb) for k in range(b)]
        np.testing.assert_array_equal(p.table('blk_rows').reshape(-1, 2), np.array(blk))
        p.close()
        p.close()  # (idempotent)


def test_cabi(lib):
    """The new symbols are declared in the header, exported and bound; the ABI version is still 7 and the argument
    structs of the two _ex calls are the ones the new entry points take; bad sizes are SMPLFIT_ERR_BAD_ARG on a
    host-only plan; a host-only plan, a batch that is not the plan's and a share_allreduce callback are refused."""
    hdr = open(osp.join(HERE, '..', 'include', 'smplfit.h')).read()
    assert '#define SMPLFIT_ABI_VERSION 7' in hdr and _lib.SMPLFIT_ABI_VERSION == 7 and lib.smplfit_abi_version() == 7
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(rf'\b{s}\s*\(', hdr), s
    assert re.search(r'smplfit_fit_segments_f32\(const smplfit_handle\* h, const smplfit_fit_args\* args,', hdr)
    assert re.search(r'smplfit_shape_solve_segments_f32\(const smplfit_handle\* h, const smplfit_shape_solve_args\* args,', hdr)

    def create(sizes, count=None):
        a = np.ascontiguousarray(sizes, dtype=np.int32)
        p = C.c_void_p()
        rc = lib.smplfit_share_segments_create(a.ctypes.data_as(_lib._ip), len(a) if count is None else count,
                                               _lib.SMPLFIT_CREATE_HOST_ONLY, C.byref(p))
        if rc:
            assert not p.value
        return rc, p

    for bad in ([0], [3, 0, 2], [-1], [5, -2], [2**31 - 1, 1], [2**30, 2**30]):
        assert create(bad)[0] == _lib.SMPLFIT_ERR_BAD_ARG, bad
    assert create([5], count=0)[0] == _lib.SMPLFIT_ERR_BAD_ARG
    assert create([5], count=-3)[0] == _lib.SMPLFIT_ERR_BAD_ARG
    p = C.c_void_p()
    assert lib.smplfit_share_segments_create(None, 1, _lib.SMPLFIT_CREATE_HOST_ONLY, C.byref(p)) == _lib.SMPLFIT_ERR_BAD_ARG
    with pytest.raises(ValueError):
        _lib.ShareSegments([4, 0], host_only=True)
    rc, p = create(MIXED)
    assert rc == 0 and lib.smplfit_share_segments_batch(p) == sum(MIXED)
    assert lib.smplfit_share_segments_batch(None) == 0
    n = C.c_size_t()
    assert lib.smplfit_share_segments_get_table(p, 3, None, 0, C.byref(n)) == _lib.SMPLFIT_ERR_BAD_ARG
    assert lib.smplfit_share_segments_get_table(None, 0, None, 0, C.byref(n)) == _lib.SMPLFIT_ERR_BAD_ARG
    # the calls: refused before a handle is looked at when the batch or the callback is wrong, or the plan has no device
    fa, sa = _lib.FitArgs(batch=sum(MIXED) + 1), _lib.ShapeSolveArgs(batch=sum(MIXED) + 1)
    assert lib.smplfit_fit_segments_f32(None, C.byref(fa), p) == _lib.SMPLFIT_ERR_BAD_ARG
    assert b"plan's" in lib.smplfit_last_error()
    assert lib.smplfit_shape_solve_segments_f32(None, C.byref(sa), p) == _lib.SMPLFIT_ERR_BAD_ARG
    cb = _lib.ShareAllreduceFn(lambda *a: 0)
    fa, sa = _lib.FitArgs(batch=sum(MIXED), share_allreduce=cb), _lib.ShapeSolveArgs(batch=sum(MIXED), share_allreduce=cb)
    assert lib.smplfit_fit_segments_f32(None, C.byref(fa), p) == _lib.SMPLFIT_ERR_BAD_ARG
    assert b'share_allreduce' in lib.smplfit_last_error()
    assert lib.smplfit_shape_solve_segments_f32(None, C.byref(sa), p) == _lib.SMPLFIT_ERR_BAD_ARG
    fa, sa = _lib.FitArgs(batch=sum(MIXED)), _lib.ShapeSolveArgs(batch=sum(MIXED))
    assert lib.smplfit_fit_segments_f32(None, C.byref(fa), p) == _lib.SMPLFIT_ERR_HIP
    assert b'host-only' in lib.smplfit_last_error()
    assert lib.smplfit_shape_solve_segments_f32(None, C.byref(sa), p) == _lib.SMPLFIT_ERR_HIP
    assert lib.smplfit_fit_segments_f32(None, None, p) == _lib.SMPLFIT_ERR_BAD_ARG
    # a NULL plan: the _ex calls (here: their refusal of a null handle)
    assert lib.smplfit_fit_segments_f32(None, C.byref(fa), None) == lib.smplfit_fit_ex_f32(None, C.byref(fa)) == _lib.SMPLFIT_ERR_BAD_ARG
    assert lib.smplfit_share_segments_workspace_bytes(None, 8, None) == lib.smplfit_workspace_bytes(None, 8) == 0
    lib.smplfit_share_segments_destroy(p)
    lib.smplfit_share_segments_destroy(None)


def test_workspace_query_host_only(lib, model_root):
    """With a NULL plan the query is ``smplfit_workspace_bytes``; with a plan it adds the plan's partial rows and sums
    (256-byte aligned regions) and answers 0 for a batch that is not the plan's."""
    md = util.load_md(model_root, 'smpl', None)[1]
    desc, keep = _lib.make_desc(md.v_template, md.shapedirs, md.posedirs, md.weights, md.J_template, md.J_shapedirs,
                                md.kintree_parents, md.J_regressor_post_lbs)
    h = _lib.Handle(desc, host_only=True)
    p = _lib.ShareSegments(MIXED, host_only=True)
    B, NC = sum(MIXED), 10 * 10 + 10
    base = h.workspace_bytes(B)
    assert lib.smplfit_share_segments_workspace_bytes(h.ptr, B, None) == base
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    assert p.workspace_bytes(h) == base + up(11 * NC * 8) + up(8 * NC * 8)
    assert lib.smplfit_share_segments_workspace_bytes(h.ptr, B + 1, p.ptr) == 0
    del keep


@pytest.fixture(scope='module')
def cpu_fitter(model_root):
    from smplfitter_amd.pt import BodyFitter, BodyModel

    m = BodyModel('smpl', 'neutral', model_root=f'{model_root}/{util.model_dir("smpl")}', num_betas=10)
    return m, BodyFitter(m)


def test_python_argument_errors(cpu_fitter):
    """``share_beta_segments`` of ``fit`` and ``fit_with_known_pose`` with CPU tensors, no device: sizes that do not sum to
    B, a size < 1, segments together with ``share_beta_group`` -> ValueError; inputs that require grad ->
    NotImplementedError with the text ``share_beta`` gives today."""
    m, f = cpu_fitter
    B = 6
    tv = torch.zeros(B, m.num_vertices, 3)
    pose = torch.zeros(B, m.num_joints * 3)
    calls = (lambda **kw: f.fit(tv, **kw), lambda **kw: f.fit_with_known_pose(pose, tv, **kw))
    for call in calls:
        for bad in ([3, 2], [3, 4], [6, 0], [7, -1], [], torch.tensor([2, 2]), torch.tensor([3, 3, 0]),
                    torch.tensor([3.0, 3.0])):
            with pytest.raises(ValueError, match='share_beta_segments'):
                call(share_beta_segments=bad)
        with pytest.raises(ValueError, match='share_beta_group'):
            call(share_beta_segments=[3, 3], share_beta_group=object())
        with pytest.raises(ValueError, match='share_beta_group'):
            call(share_beta_segments=torch.tensor([3, 3], dtype=torch.int32), share_beta=True, share_beta_group=object())
    want = {}
    for name, call in zip(('fit', 'known_pose'), calls):
        for key in ('share_beta', 'share_beta_segments'):
            with pytest.raises(NotImplementedError) as e:
                call(**{key: True if key == 'share_beta' else [2, 4]}, vertex_weights=torch.ones(B, m.num_vertices, requires_grad=True))
            want[name, key] = str(e.value)
        assert want[name, 'share_beta'] == want[name, 'share_beta_segments'] and 'share_beta' in want[name, 'share_beta']
    tvg = tv.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match='share_beta'):
        f.fit(tvg, share_beta_segments=[6])


def test_plan_cache_not_copied(cpu_fitter):
    """The cache of native plans is bounded and is dropped by pickling and deepcopy (a copy must not free, or share, the
    original's native objects)."""
    from smplfitter_amd.pt import BodyFitter

    m, _ = cpu_fitter
    f = BodyFitter(m)
    assert f.MAX_SEGMENT_PLANS >= 1
    f._segment_plans[(0, (1, 2))] = object()  # (a stand-in: no device here)
    g = copy.deepcopy(f)
    assert len(g._segment_plans) == 0 and len(f._segment_plans) == 1 and g.n_betas == f.n_betas
    assert len(f.__getstate__()['_segment_plans']) == 0
