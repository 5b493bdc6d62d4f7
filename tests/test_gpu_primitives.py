"""-m gpu: the rotation primitives of sf_math.h as compiled for the DEVICE (v_rsq_f64 / v_rcp_f64 seeds with Newton steps,
FMA contraction, the device's sinf / cosf / atan2f) on the hard-input families of tests/prim_util.py, under the gates the
host build passes in tests/test_hostemu.py — the same arrays, through smplfit_primitives_f32 (ops 0 - 4), one launch of a
few thousand elements per primitive.  tests/test_gpu_evidence.py::test_device_primitives keeps the reference's goldens."""

import ctypes as C

import numpy as np
import pytest
import torch

import prim_util as P
from test_gpu_evidence import _prim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture
def run(dev):
    return lambda op, a, b, out_shape: _prim(op, a, b, out_shape, dev)


def test_proj_so3_hard_families(run, capsys):
    """Proper rotation, optimality deficit <= 5e-7 and conditioned distance to the fp64 SVD's rotation <= 5e-7 on every
    input, the degenerate ones included; a NaN or an Inf in any one position gives an all-NaN row beside untouched ones.
    (host build and device build: deficit 8.9e-8, distance 3.0e-8 observed)"""
    with capsys.disabled():
        print()
        P.check_proj_so3(run, 'device')
    P.check_proj_nonfinite(run, 'device')


def test_mat2rotvec_branches(run, capsys):
    """All four branches of the log map at their boundaries: trace = 0, diagonal ties, angle -> 0 and -> pi."""
    with capsys.disabled():
        print()
        P.check_mat2rotvec(run, 'device')


def test_rotvec2mat_angles(run, capsys):
    """Zero, denormal, tiny, near-pi and very large (100 pi) angles against fp64 Rodrigues."""
    with capsys.disabled():
        print()
        P.check_rotvec2mat(run, 'device')


def test_align_near_parallel(run, capsys):
    """Unit pairs approaching parallel and antiparallel, identical and exactly opposite ones."""
    with capsys.disabled():
        print()
        P.check_align(run, 'device')


def test_swing_twist_near_parallel(run, capsys):
    """Bones approaching parallel and antiparallel, zero bones, a zero covariance, twists at +-(pi - 10^-k)."""
    with capsys.disabled():
        print()
        P.check_swing_twist(run, 'device')


def test_launch_edges(dev):
    """n = 1, 63, 64, 65 (one thread, a wave short of one lane, a full wave, a second block of one lane): the first n
    rows equal those of the full launch bit for bit and nothing behind row n is written (a NaN-pattern guard)."""
    from smplfitter_amd import _lib

    lib = _lib.load()
    A = P.proj_families()['near_rot'][0][::7][:128]
    full = _prim(0, A, None, A.shape, dev)
    ta = torch.from_numpy(A).to(dev)
    for n in (1, 63, 64, 65):
        out = torch.full((128, 3, 3), float('nan'), dtype=torch.float32, device=dev)
        out.view(torch.int32).fill_(0x7FC00000 | 0x1234)
        _lib.check(lib.smplfit_primitives_f32(0, C.c_void_p(ta.data_ptr()), C.c_void_p(0), C.c_void_p(out.data_ptr()), n,
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        torch.cuda.synchronize()
        assert np.array_equal(out[:n].cpu().numpy(), full[:n]), n
        assert bool((out[n:].view(torch.int32) == (0x7FC00000 | 0x1234)).all()), n
