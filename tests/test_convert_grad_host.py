"""Host checks (no GPU) of the differentiable ``BodyConverter``: the transposed-matrix builder behind
``smplfit_transfer_backward_f32`` under AddressSanitizer + UBSan, the C-ABI of the new call, and the fp64 arbiter of the
gradient tests against the reference's own fp32 autograd gradients (tests/golden/make_golden_convert_grad.py)."""

import ctypes as C
import os
import os.path as osp
import subprocess

import numpy as np
import pytest

import convert_grad_util as cu
import util
from smplfitter_amd import _lib, build

HERE = osp.dirname(osp.abspath(__file__))
CSRC = osp.join(HERE, '..', 'smplfitter_amd', 'csrc')
MAIN = osp.join(HERE, 'hostemu', 'transfer_transpose_main.cpp')
EXE = osp.join(HERE, 'hostemu', '_build', 'transfer_transpose_asan_static')


@pytest.fixture(scope='module')
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def gold():
    return np.load(osp.join(HERE, 'golden', 'golden_convert_grad.npz'))


def test_transpose_csr_sanitized():
    """``sf::transpose_csr`` (sf_tables.cpp) in a stand-alone program built with -fsanitize=address,undefined and run as a
    child process: seeded matrices — rows of 0 to 7 entries, empty columns, repeated columns in a row, one column of 2000
    entries, V_in = 1, V_out = 1 — against a dense transpose: exact values, ``indptr`` monotone and ending at nnz, every
    index in range, the entries of a column in ascending row order.  A wrong index in this table would be an
    out-of-bounds read of the kernel, so it is checked here, before any GPU run."""
    deps = [MAIN, osp.join(CSRC, 'sf_tables.cpp'), osp.join(CSRC, 'sf_tables.h')]
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
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count('ok ') == 7 and 'FAIL' not in r.stdout


def test_backward_symbol_and_refusals(lib):
    """``smplfit_transfer_backward_f32`` is exported and bound; null pointers and a negative batch are BAD_ARG, a
    host-only matrix gives the forward's error; a batch of 0 is SMPLFIT_OK before the matrix is looked at (the one
    documented difference from the forward, which refuses a host-only matrix first: include/smplfit.h)."""
    assert 'smplfit_transfer_backward_f32' in _lib.EXPORTED_SYMBOLS
    fn = lib.smplfit_transfer_backward_f32
    indptr = np.array([0, 2, 2, 3], np.int32)
    indices = np.array([0, 4, 1], np.int32)
    values = np.array([0.5, 0.5, 1.0], np.float32)
    tr = _lib.Transfer(5, 3, indptr, indices, values, host_only=True)
    p = C.c_void_p(16)  # (never dereferenced: every call below is refused, or has nothing to do)
    assert fn(None, p, 1, p, None) == _lib.SMPLFIT_ERR_BAD_ARG
    assert fn(tr.ptr, None, 1, p, None) == _lib.SMPLFIT_ERR_BAD_ARG
    assert fn(tr.ptr, p, 1, None, None) == _lib.SMPLFIT_ERR_BAD_ARG
    assert fn(tr.ptr, p, -1, p, None) == _lib.SMPLFIT_ERR_BAD_ARG
    rc_fwd = lib.smplfit_transfer_f32(tr.ptr, p, 1, p, None)
    rc_bwd = fn(tr.ptr, p, 1, p, None)
    assert rc_bwd == rc_fwd and rc_bwd not in (_lib.SMPLFIT_OK, _lib.SMPLFIT_ERR_BAD_ARG)
    assert b'host-only' in lib.smplfit_last_error()
    with pytest.raises(_lib.SmplfitError):
        tr.backward(16, 1, 16)
    assert fn(tr.ptr, p, 0, p, None) == _lib.SMPLFIT_OK
    assert lib.smplfit_transfer_f32(tr.ptr, p, 0, p, None) == rc_fwd  # (the forward: host-only comes first)
    assert lib.smplfit_abi_version() == 7  # a new symbol, no changed struct


@pytest.mark.parametrize('case', list(cu.CASES))
@pytest.mark.parametrize('tag', list(cu.DIRS))
def test_arbiter_matches_reference(tag, case, gold, model_root, data_root_fat):
    """The fp64 arbiter (tests/convert_grad_util.py) reproduces the reference's fp32 autograd gradients of ``convert``: per
    tensor, relative to max |fp64|, within twice the largest figure the fixture's generator printed for that tensor
    (``REF_REL_LARGEST``: pose_rotvecs 3.1e-4, shape_betas 4.9e-5, trans 4.7e-5, known_output_shape_betas 5.8e-5,
    known_output_pose_rotvecs 5.1e-6); its results lie within twice the fp32 distances the generator printed
    (``REF_OUT_LARGEST``) of the reference's."""
    assert util.csr_digest(util.load_transfer_csr(data_root_fat, tag)) == str(gold[f'{tag}.csr_sha256'])
    x = cu.fixture_inputs(gold, tag)
    assert set(x) == set(cu.make_inputs(tag, 1, 1))
    p = f'{tag}.{case}.'
    n_joints_out = x['known_output_pose_rotvecs'].shape[1] // 3
    cot = cu.cotangents(int(gold[p + 'seed']), case, n_joints_out)
    out, grads = cu.arbiter(model_root, data_root_fat, tag, case, x, cot)
    assert set(grads) == {k[len(p) + 4:] for k in gold.files if k.startswith(p + 'g32.')} == set(cu.grad_names(case))
    assert set(out) == {k[len(p) + 4:] for k in gold.files if k.startswith(p + 'out.')}
    for k in cot:
        d = np.abs(out[k].reshape(cot[k].shape) - gold[p + 'out.' + k]).max()
        print(f'[convert-grad] arbiter {tag} {case} result {k}: |fp64 - reference fp32| {d:.2e}')
        assert d <= 2 * cu.REF_OUT_LARGEST[k], (tag, case, k, d)
    for k, v in grads.items():
        rel = np.abs(gold[p + 'g32.' + k] - v).max() / np.abs(v).max()
        print(f'[convert-grad] arbiter {tag} {case} {k}: reference fp32 vs fp64, relative {rel:.2e}, max |fp64| {np.abs(v).max():.2e}')
        assert rel <= cu.REF_REL_CAP
        assert rel <= 2 * cu.REF_REL_LARGEST[k], (tag, case, k, rel)
