"""-m gpu: the two front ends of k_posedirs_gemm_bf16x3 give the same bits.

A fit's prologue kernel (k_prologue_bm) writes the pose features in one of two forms: as the split-bf16 planes the GEMM
multiplies, in the GEMM's fragment order (ws.rpP, sf::plane_off; the default), which the GEMM of every shape solve then
just loads; or, with SMPLFIT_GEMM_PLANES=0, as fp32 rows (ws.rp) that the GEMM splits itself, as it always did.  Both
sides split with sf::split_bf16x3 and the kernel is the same code from its first barrier on, so a whole fit must return
IDENTICAL tensors either way — compared with torch.equal, no tolerance.

The route needs k_prologue_bm, i.e. k_solve_bm, i.e. the coarse cell tables: batches up to 768 take the fine ones by
default, so the small cases force the coarse tables with SMPLFIT_FINE_B=0 (as tests/test_gpu_stages_hard.py does for
k_solve_bm).  Which front end ran is not visible in the results; the library counts the GEMM launches that read planes
(smplfit_gemm_plane_launches), and every case asserts that count: num_iter launches with the planes on, none with
them off.  Where the planes are not used at all (a build or model without the route) the case skips.

Batches (Mp = the batch rounded up to 128; a GEMM wave holds 32 instances, a workgroup 8 waves; k_prologue_bm runs 64
lanes a workgroup and its pad lanes write the zero planes of the pad instances):
  1     Mp = 128: one lane of one 32-group, every other column of the planes is padding; one GEMM workgroup whose last
        four waves are idle (m0 >= Mp)
  33    the second 32-group of a prologue wave
  129   Mp = 256: a full GEMM workgroup; its fifth wave holds one instance, the last three only the zero planes
  257   Mp = 384: a second GEMM workgroup row, with idle waves
  1001  the coarse tables by default, a ragged last block
"""

import numpy as np
import pytest
import torch

from smplfitter_amd import _lib
from test_gpu_parity import get_model, t

pytestmark = pytest.mark.gpu

NUM_ITER = 3
BATCHES = [1, 33, 129, 257, 1001]
_targets = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def targets(B, m, g, dev):
    """B targets: the golden poses cycled, every row with its own shape and translation (seeded); computed once per
    batch by the model's forward, shared by both cases of the batch, read only."""
    if B not in _targets:
        rng = np.random.RandomState(B)
        rows = np.arange(B) % g['pose'].shape[0]
        pose = (g['pose'][rows] * rng.uniform(0.5, 1.0, (B, 1))).astype(np.float32)
        betas = rng.normal(0, 1.5, (B, 10)).astype(np.float32)
        trans = rng.normal(0, 0.5, (B, 3)).astype(np.float32)
        fw = m(t(pose, dev), t(betas, dev), t(trans, dev))
        _targets[B] = (fw['vertices'].clone(), fw['joints'].clone())
    return _targets[B]


@pytest.mark.parametrize('with_joints', [True, False], ids=['joints', 'no_joints'])
@pytest.mark.parametrize('B', BATCHES)
def test_fit_bits_planes_vs_fp32_front_end(B, with_joints, model_root, golden, dev, smplfit_env):
    g = golden('smpl')
    m, f = get_model(model_root, 'smpl', g, dev)
    tv, tj = targets(B, m, g, dev)
    if B <= 768:
        smplfit_env('SMPLFIT_FINE_B', '0')
    out, launches = {}, {}
    for planes in ('1', '0'):
        smplfit_env('SMPLFIT_GEMM_PLANES', planes)
        before = _lib.gemm_plane_launches()
        out[planes] = f.fit(tv, tj if with_joints else None, num_iter=NUM_ITER)
        torch.cuda.synchronize()
        launches[planes] = _lib.gemm_plane_launches() - before
    print(f'\n[gemm planes] B={B} joints={with_joints}: plane GEMM launches {launches}')
    if launches['1'] == 0:
        pytest.skip('the GEMM does not read feature planes on this route (k_prologue_bm / k_posedirs_gemm_bf16x3 not taken)')
    assert launches['1'] == NUM_ITER, launches  # one GEMM per shape solve, one chunk
    assert launches['0'] == 0, launches
    assert set(out['1']) == set(out['0']) >= {'pose_rotvecs', 'shape_betas', 'trans', 'orientations', 'relative_orientations'}
    for k, v in out['1'].items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, out['0'][k]), (k, float((v - out['0'][k]).abs().max()))
