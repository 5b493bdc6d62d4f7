"""Cases, shared inputs and the fp64 arbiter of the ``BodyFitter.fit`` gradient tests (tests/test_fit_grad_host.py,
tests/test_gpu_fit_grad.py, tests/golden/make_golden_fit_grad.py).

The arbiter is the project's own restatement of the fit, ``TorchFit`` (smplfitter_amd/pt/_autograd.py, pinned to the
reference's fixtures by tests/test_autograd_fit.py), run in fp64 on the CPU; ``torch.autograd.grad`` gives the gradients.
"""

import numpy as np
import torch

import util

# the cases of golden_fit_grad.npz
CASES = dict(
    A=dict(joints=True, vw=True, jw=True, num_iter=1, refine=False),
    B=dict(joints=True, vw=True, jw=True, num_iter=1, refine=True),
    C=dict(joints=True, vw=True, jw=True, num_iter=3, refine=True, beta_regularizer2=0.5),
    D=dict(joints=False, vw=True, jw=False, num_iter=2, refine=True),
    E=dict(joints=False, vw=False, jw=False, num_iter=3, refine=True, beta_regularizer=0.1),
    F=dict(joints=True, vw=True, jw=False, num_iter=2, refine=False),
    G=dict(joints=True, vw=True, jw=True, num_iter=2, refine=True, kid=True, kid_regularizer=2.0),
)
FIXTURE_CASES = dict(smpl='ABCDEFG', smplxfat='AC')
TENSORS = ('target_vertices', 'target_joints', 'vertex_weights', 'joint_weights')
SUBSET = 512  # vertices on which the fixture stores the vertex-sized gradients (tests/known_pose_grad_util.py)


def subset(V, seed=0):
    return np.sort(np.random.RandomState(seed).permutation(V)[:SUBSET]) if V > SUBSET else np.arange(V)


def case_inputs(g, case, B=2, seed=0):
    """The tensor inputs (numpy fp32) and the options of ``fit`` of a case from a golden set ``g`` (golden_<kind>.npz):
    its first ``B`` rows of targets, seeded weights in [0.5, 1.5) where the set has none; rows beyond the set's repeat them
    with seeded noise on the targets.  -> (x, kw, kid)"""
    cfg = CASES[case]
    n = g['target_vertices'].shape[0]
    idx = np.arange(B) % n
    rs = np.random.RandomState(2000 + seed + ord(case))
    V, J = g['target_vertices'].shape[1], g['target_joints'].shape[1]
    far = (np.arange(B) >= n)[:, None, None]
    x = dict(target_vertices=(g['target_vertices'][idx] + far * 0.01 * rs.randn(B, V, 3)).astype(np.float32))
    if cfg['joints']:
        x['target_joints'] = (g['target_joints'][idx] + far * 0.01 * rs.randn(B, J, 3)).astype(np.float32)
    if cfg['vw']:
        x['vertex_weights'] = (g['vertex_weights'][idx] if 'vertex_weights' in g else rs.uniform(0.5, 1.5, (B, V))).astype(np.float32)
    if cfg['jw']:
        x['joint_weights'] = (g['joint_weights'][idx] if 'joint_weights' in g else rs.uniform(0.5, 1.5, (B, J))).astype(np.float32)
    kw = dict(num_iter=cfg['num_iter'], beta_regularizer=cfg.get('beta_regularizer', 1.0),
              beta_regularizer2=cfg.get('beta_regularizer2', 0.0), final_adjust_rots=cfg['refine'])
    if 'kid_regularizer' in cfg:
        kw['kid_regularizer'] = cfg['kid_regularizer']
    return x, kw, bool(cfg.get('kid'))


def cotangents(seed, B, J, nb, kid):
    """Seeded cotangents of the results (not stored in the fixture)."""
    rs = np.random.RandomState(seed)
    c = dict(pose_rotvecs=rs.randn(B, J * 3).astype(np.float32), shape_betas=rs.randn(B, nb).astype(np.float32),
             trans=rs.randn(B, 3).astype(np.float32))
    if kid:
        c['kid_factor'] = rs.randn(B).astype(np.float32)
    return c


_tf = {}


def torchfit64(model_root, name, g, kid):
    """``TorchFit(dtype=float64)`` of a golden set's model on the CPU (built once)."""
    if (name, kid) not in _tf:
        from smplfitter_amd.pt import BodyModel
        from smplfitter_amd.pt._autograd import TorchFit

        kind = 'smplx' if name.startswith('smplx') else 'smpl'
        kw = dict(vertex_subset=g['vertex_subset']) if 'vertex_subset' in g else {}
        bm = BodyModel(kind, 'neutral', model_root=f'{model_root}/{util.model_dir(name)}', num_betas=10, **kw)
        _tf[name, kid] = TorchFit(bm, enable_kid=kid, dtype=torch.float64)
    return _tf[name, kid]


def arbiter(tf, x, kw, cot):
    """fp64 results and gradients of sum(cot . results) w.r.t. every tensor of ``x`` (numpy in, numpy out)."""
    torch.set_num_threads(8)
    ts = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in x.items()}
    out = tf.fit(ts['target_vertices'], ts.get('target_joints'), ts.get('vertex_weights'), ts.get('joint_weights'), **kw)
    loss = sum((out[k] * torch.as_tensor(np.asarray(c, np.float64))).sum() for k, c in cot.items())
    names = list(ts)
    gs = torch.autograd.grad(loss, [ts[k] for k in names], allow_unused=True)
    grads = {k: (np.zeros(ts[k].shape) if g is None else g.numpy()) for k, g in zip(names, gs)}
    return {k: v.detach().numpy() for k, v in out.items()}, grads
