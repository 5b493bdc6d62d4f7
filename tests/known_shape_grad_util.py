"""Cases, shared inputs and the fp64 arbiter of the ``BodyFitter.fit_with_known_shape`` gradient tests
(tests/test_known_shape_grad_host.py, tests/test_gpu_known_shape_grad.py, tests/golden/make_golden_known_shape_grad.py).

The arbiter is the project's own restatement, ``TorchFit.fit_with_known_shape`` (smplfitter_amd/pt/_autograd.py, pinned
to the reference's ``knownshape.*`` fixtures by tests/test_known_shape_grad_host.py), run in fp64 on the CPU;
``torch.autograd.grad`` gives the gradients.
"""

import numpy as np
import torch

from fit_grad_util import SUBSET, subset, torchfit64  # noqa: F401  (shared with the fit's gradient tests)

# the cases of golden_known_shape_grad.npz
CASES = dict(
    A=dict(joints=True, vw=True, jw=True, num_iter=1, refine=False),
    B=dict(joints=True, vw=True, jw=True, num_iter=1, refine=True),
    C=dict(joints=True, vw=True, jw=True, num_iter=3, refine=True),
    D=dict(joints=False, vw=True, jw=False, num_iter=2, refine=True),
    E=dict(joints=False, vw=False, jw=False, num_iter=3, refine=True),
    F=dict(joints=True, vw=True, jw=False, num_iter=2, refine=False),  # (vertex weights alone: the alignment is unweighted)
    G=dict(joints=True, vw=True, jw=True, num_iter=2, refine=True, kid=True),
)
FIXTURE_CASES = dict(smpl='ABCDEFG', smplxfat='AC')
TENSORS = ('shape_betas', 'kid_factor', 'target_vertices', 'target_joints', 'vertex_weights', 'joint_weights')
VERTEX_SIZED = ('target_vertices', 'vertex_weights')


def case_inputs(g, case, B=2, seed=0):
    """The tensor inputs (numpy fp32) and the options of ``fit_with_known_shape`` of a case from a golden set ``g``
    (golden_<kind>.npz): its first ``B`` rows of betas and targets (the ``kid.*`` targets with ``g['kid']`` for the kid
    case), seeded weights in [0.5, 1.5) where the set has none; rows beyond the set's repeat them with seeded noise on the
    targets and the betas.  -> (x, kw)"""
    cfg = CASES[case]
    kid = bool(cfg.get('kid'))
    pre = 'kid.' if kid else ''
    n = g['target_vertices'].shape[0]
    idx = np.arange(B) % n
    rs = np.random.RandomState(3000 + seed + ord(case))
    V, J = g['target_vertices'].shape[1], g['target_joints'].shape[1]
    far = (np.arange(B) >= n)
    x = dict(shape_betas=(g['betas'][idx] + far[:, None] * 0.1 * rs.randn(B, g['betas'].shape[1])).astype(np.float32))
    if kid:
        x['kid_factor'] = g['kid'][idx].astype(np.float32)
    x['target_vertices'] = (g[pre + 'target_vertices'][idx] + far[:, None, None] * 0.01 * rs.randn(B, V, 3)).astype(np.float32)
    if cfg['joints']:
        x['target_joints'] = (g[pre + 'target_joints'][idx] + far[:, None, None] * 0.01 * rs.randn(B, J, 3)).astype(np.float32)
    if cfg['vw']:
        x['vertex_weights'] = (g['vertex_weights'][idx] if 'vertex_weights' in g else rs.uniform(0.5, 1.5, (B, V))).astype(np.float32)
    if cfg['jw']:
        x['joint_weights'] = (g['joint_weights'][idx] if 'joint_weights' in g else rs.uniform(0.5, 1.5, (B, J))).astype(np.float32)
    return x, dict(num_iter=cfg['num_iter'], final_adjust_rots=cfg['refine'])


def cotangents(seed, B, J):
    """Seeded cotangents of the results (not stored in the fixture)."""
    rs = np.random.RandomState(seed)
    return dict(pose_rotvecs=rs.randn(B, J * 3).astype(np.float32), trans=rs.randn(B, 3).astype(np.float32))


def arbiter(tf, x, kw, cot):
    """fp64 results and gradients of sum(cot . results) w.r.t. every tensor of ``x`` (numpy in, numpy out)."""
    torch.set_num_threads(8)
    ts = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in x.items()}
    out = tf.fit_with_known_shape(**ts, **kw)
    loss = sum((out[k] * torch.as_tensor(np.asarray(c, np.float64))).sum() for k, c in cot.items())
    names = list(ts)
    gs = torch.autograd.grad(loss, [ts[k] for k in names], allow_unused=True)
    grads = {k: (np.zeros(ts[k].shape) if g is None else g.numpy()) for k, g in zip(names, gs)}
    return {k: v.detach().numpy() for k, v in out.items()}, grads
