"""-m gpu: the two forms of the part-rotation kernel K1r give the same bits.

k_rotations_spread (what fit calls of up to 4096 instances run) gives every joint a wave of its own and spreads the
joints of a block of 64 instances over ceil(J / 8) workgroups; a toe's wave fits its foot's part itself.
SMPLFIT_ROT_SPREAD=0 runs the kernels it replaces there: k_rotations_bm (up to 32 joints: three or four joints a wave, every rotation through LDS, the toes behind a
barrier) or k_rotations_bm_rounds (33 .. 64 joints).  All three run the same per-lane code on the same inputs and add the
part-sum rows in the same order, so a whole fit must return IDENTICAL tensors either way — torch.equal, no tolerance.

Which form ran does not show in the results and both count under the same stage id; the library counts the launches of
the spread form (smplfit_rotation_spread_launches).  Every case asserts num_iter launches with the switch on, none
with it off, and stage counters that do not differ between the two runs.  The in-tree build must take the lane =
instance rotation kernel on both models (neither counter moving is a failure); only another build loaded through
SMPLFIT_LIB, which may lack the route, skips.

The route needs k_prologue_bm, i.e. the coarse cell tables: batches up to 768 take the fine ones by default, so the
small cases force the coarse tables with SMPLFIT_FINE_B=0.

Batches (a workgroup holds 64 instances, Mp = the batch rounded up to 128):
  1     one lane, every other one clamped
  63    a ragged block
  65    a second block of one instance
  129   Mp = 256: a third block, one instance, the pad columns behind it
  1001  the coarse tables by default, a ragged last block
SMPL-shaped model (24 joints): 3 workgroups a block; the toes 10 and 11 sit in the second (joints 8 .. 15), with foot 8
and without foot 7.  SMPL-X-shaped model (55 joints): 7 workgroups a block, the last one with an idle wave.
Variants: target joints omitted (the rows of the all-slots table), joint weights (the multi-joint Kabsch), a warm start
(the first pass composes with the instance-major rotations of the initial pose); joint weights and a warm start once on
the SMPL-X-shaped model too, whose partner is the kernel with rounds.
"""

import os

import numpy as np
import pytest
import torch

from smplfitter_amd import _lib
from test_gpu_parity import get_model, t

pytestmark = pytest.mark.gpu

NUM_ITER = 3
_targets = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def targets(name, B, m, g, dev):
    """B targets of one model: the golden poses cycled and scaled, every row with its own shape and translation (seeded);
    computed once per (model, batch) by the model's forward, shared by the cases of that batch, read only.  With them the
    pose and shape of a warm start (the truth, perturbed) and joint weights."""
    if (name, B) not in _targets:
        rng = np.random.RandomState(1000 + B)
        rows = np.arange(B) % g['pose'].shape[0]
        pose = (g['pose'][rows] * rng.uniform(0.5, 1.0, (B, 1))).astype(np.float32)
        betas = rng.normal(0, 1.5, (B, 10)).astype(np.float32)
        trans = rng.normal(0, 0.5, (B, 3)).astype(np.float32)
        fw = m(t(pose, dev), t(betas, dev), t(trans, dev))
        J = fw['joints'].shape[1]
        _targets[name, B] = dict(
            tv=fw['vertices'].clone(), tj=fw['joints'].clone(),
            pose0=t((pose + rng.normal(0, 0.05, pose.shape)).astype(np.float32), dev),
            betas0=t((betas + rng.normal(0, 0.3, betas.shape)).astype(np.float32), dev),
            jw=t(rng.uniform(0.2, 1.0, (B, J)).astype(np.float32), dev))
    return _targets[name, B]


def fit_kwargs(variant, tg):
    if variant == 'joints':
        return dict(target_joints=tg['tj'])
    if variant == 'no_joints':
        return dict(target_joints=None)
    if variant == 'joint_weights':
        return dict(target_joints=tg['tj'], joint_weights=tg['jw'])
    assert variant == 'warm'
    return dict(target_joints=tg['tj'], initial_pose_rotvecs=tg['pose0'], initial_shape_betas=tg['betas0'])


CASES = ([('smpl', B, 'joints') for B in (1, 63, 65, 129, 1001)] +
         [('smpl', B, v) for B in (65, 129) for v in ('no_joints', 'joint_weights', 'warm')] +
         [('smplx', B, v) for B in (65, 129) for v in ('joints', 'no_joints')] +
         [('smplx', 65, 'joint_weights'), ('smplx', 65, 'warm')])


@pytest.mark.parametrize('name,B,variant', CASES, ids=[f'{n}-B{B}-{v}' for n, B, v in CASES])
def test_fit_bits_spread_vs_block_form(name, B, variant, model_root, golden, dev, smplfit_env):
    g = golden(name)
    m, f = get_model(model_root, name, g, dev)
    tg = targets(name, B, m, g, dev)
    kw = fit_kwargs(variant, tg)
    if B <= 768:
        smplfit_env('SMPLFIT_FINE_B', '0')
    out, spread, stages = {}, {}, {}
    for on in ('1', '0'):
        smplfit_env('SMPLFIT_ROT_SPREAD', on)
        s0, c0 = _lib.rotation_spread_launches(), _lib.stage_launches()
        out[on] = f.fit(tg['tv'], num_iter=NUM_ITER, **kw)
        torch.cuda.synchronize()
        spread[on] = _lib.rotation_spread_launches() - s0
        stages[on] = {k: v - c0[k] for k, v in _lib.stage_launches().items()}
    print(f'\n[rot spread] {name} B={B} {variant}: spread launches {spread}, stages {stages["1"]}')
    rot = 'rotations_bm' if m.num_joints <= 32 else 'rotations_bm_rounds'
    if os.environ.get('SMPLFIT_LIB') and stages['0'][rot] == 0 and spread['1'] == 0:
        pytest.skip(f'the loaded build does not run the lane = instance rotation kernel on this route: {stages["0"]}')
    assert spread['1'] == NUM_ITER, (spread, stages)  # one rotation pass per iteration
    assert spread['0'] == 0, spread
    assert stages['1'][rot] == NUM_ITER and stages['1'] == stages['0'], stages
    assert set(out['1']) == set(out['0']) >= {'pose_rotvecs', 'shape_betas', 'trans', 'orientations', 'relative_orientations'}
    for k, v in out['1'].items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, out['0'][k]), (k, float((v - out['0'][k]).abs().max()))


def test_batch_limit_counts_the_whole_call(model_root, golden, dev, smplfit_env):
    """The batch limit of the spread form (SMPLFIT_ROT_SPREAD_B; 4096 by default) is about what runs side by side on
    the chip, so it counts the instances of the whole call, not those of one of its concurrent chunks.  The
    SMPL-X-shaped model cuts a call of 1792 instances into two chunks of 896: with a limit of 1000 neither chunk may
    take the spread form although each is below it, with a limit of 1792 every rotation launch takes it; the bits are
    the same."""
    name, B = 'smplx', 1792
    g = golden(name)
    m, f = get_model(model_root, name, g, dev)
    tg = targets(name, B, m, g, dev)
    out, spread, rot = {}, {}, {}
    for limit in ('1000', '1792'):
        smplfit_env('SMPLFIT_ROT_SPREAD_B', limit)
        s0, c0 = _lib.rotation_spread_launches(), _lib.stage_launches()
        out[limit] = f.fit(tg['tv'], tg['tj'], num_iter=NUM_ITER)
        torch.cuda.synchronize()
        spread[limit] = _lib.rotation_spread_launches() - s0
        rot[limit] = _lib.stage_launches()['rotations_bm_rounds'] - c0['rotations_bm_rounds']
    print(f'\n[rot spread] {name} B={B}: limit -> spread launches {spread}, rotation launches {rot}')
    if os.environ.get('SMPLFIT_LIB') and rot['1792'] == 0:
        pytest.skip('the loaded build does not run the lane = instance rotation kernel on this route')
    assert rot['1000'] == rot['1792'] >= NUM_ITER, rot  # (once per chunk and iteration)
    assert spread['1000'] == 0 and spread['1792'] == rot['1792'], (spread, rot)
    for k, v in out['1000'].items():
        assert torch.equal(v, out['1792'][k]), (k, float((v - out['1792'][k]).abs().max()))
