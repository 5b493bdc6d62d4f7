"""fp64 torch restatement of ``BodyModel.forward`` for the gradient tests (tests/test_forward_grad_host.py,
tests/test_gpu_forward_grad.py): blend shapes, the kinematic chain and linear blend skinning as differentiable torch
operations, so that ``torch.autograd.grad`` gives the fp64 vector-Jacobian product to compare the HIP backward with.
Rotation vectors use a Rodrigues form whose derivative is exact at r = 0 (the series of sin(t)/t and (1 - cos t)/t^2).
"""

import numpy as np
import torch


class Model64:
    """The constants of a ``modelio.ModelData`` as fp64 CPU tensors."""

    def __init__(self, md, dtype=torch.float64):
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
        self.v_template, self.shapedirs, self.posedirs = t(md.v_template), t(md.shapedirs), t(md.posedirs)
        self.J_template, self.J_shapedirs, self.weights = t(md.J_template), t(md.J_shapedirs), t(md.weights)
        self.kid_shapedir, self.kid_J_shapedir = t(md.kid_shapedir), t(md.kid_J_shapedir)
        self.parents = [int(p) for p in md.kintree_parents]
        self.J, self.S, self.dtype = len(self.parents), self.shapedirs.shape[2], dtype


def mm(a, b):
    """Batched 3 x 3 products as elementwise multiply-and-sum (no batched GEMM over millions of tiny matrices)."""
    return (a[..., :, :, None] * b[..., None, :, :]).sum(-2)


def mv(a, v):
    return (a * v[..., None, :]).sum(-1)


def _coef(t2):
    """sin(t)/t and (1 - cos t)/t^2 of t^2, smooth through t = 0."""
    small = t2 < 1e-4
    ts = torch.where(small, torch.ones_like(t2), t2)
    th = torch.sqrt(ts)
    a = torch.where(small, 1 - t2 / 6 + t2 * t2 / 120, torch.sin(th) / th)
    b = torch.where(small, 0.5 - t2 / 24 + t2 * t2 / 720, (1 - torch.cos(th)) / ts)
    return a, b


def rotvec2mat(r):
    """(..., 3) -> (..., 3, 3): R = I + a K + b K^2."""
    a, b = _coef((r * r).sum(-1))
    z = torch.zeros_like(r[..., 0])
    K = torch.stack([z, -r[..., 2], r[..., 1], r[..., 2], z, -r[..., 0], -r[..., 1], r[..., 0], z], -1)
    K = K.reshape(*r.shape[:-1], 3, 3)
    eye = torch.eye(3, dtype=r.dtype).expand_as(K)
    return eye + a[..., None, None] * K + b[..., None, None] * mm(K, K)


def forward(m, pose_rotvecs=None, shape_betas=None, trans=None, kid_factor=None, rel_rotmats=None,
            glob_rotmats=None, return_vertices=True):
    """The forward of the reference's BodyModel (pose features rel[:, 1:] or parent^T glob, joints from betas and the
    kid direction, FK of positions, LBS), on tensors of ``m.dtype``."""
    J, par = m.J, m.parents
    first = next(a for a in (pose_rotvecs, shape_betas, trans, rel_rotmats, glob_rotmats) if a is not None)
    B = first.shape[0]
    if pose_rotvecs is not None:
        rel_rotmats = rotvec2mat(pose_rotvecs.reshape(B, J, 3))
    elif rel_rotmats is not None:
        rel_rotmats = rel_rotmats.reshape(B, J, 3, 3)
    elif glob_rotmats is None:
        rel_rotmats = torch.eye(3, dtype=m.dtype).expand(B, J, 3, 3)
    if glob_rotmats is None:
        g = [rel_rotmats[:, 0]]
        for j in range(1, J):
            g.append(mm(g[par[j]], rel_rotmats[:, j]))
        glob_rotmats = torch.stack(g, 1)
    p1 = torch.tensor(par[1:])
    if rel_rotmats is None:
        feat = mm(glob_rotmats[:, p1].transpose(-1, -2), glob_rotmats[:, 1:])
    else:
        feat = rel_rotmats[:, 1:]
    betas = shape_betas if shape_betas is not None else torch.zeros((B, 0), dtype=m.dtype)
    nb = min(betas.shape[1], m.S)
    betas = betas[:, :nb]
    kid = torch.zeros((1,), dtype=m.dtype) if kid_factor is None else kid_factor.reshape(-1)
    jr = (m.J_template + torch.einsum('jcs,bs->bjc', m.J_shapedirs[:, :, :nb], betas)
          + torch.einsum('jc,b->bjc', m.kid_J_shapedir, kid))
    rb = mv(glob_rotmats[:, p1], jr[:, 1:] - jr[:, p1])
    pos = [jr[:, 0]]
    for j in range(1, J):
        pos.append(pos[par[j]] + rb[:, j - 1])
    pos = torch.stack(pos, 1)
    tr = torch.zeros((1, 3), dtype=m.dtype) if trans is None else trans.reshape(-1, 3)
    out = dict(joints=pos + tr[:, None], orientations=glob_rotmats)
    if not return_vertices:
        return out
    vp = (m.v_template + torch.einsum('vcs,bs->bvc', m.shapedirs[:, :, :nb], betas)
          + torch.einsum('vcp,bp->bvc', m.posedirs, feat.reshape(B, -1))
          + torch.einsum('vc,b->bvc', m.kid_shapedir, kid))
    t = pos - mv(glob_rotmats, jr)
    # blended per-vertex transforms first, applied elementwise (no batched 3 x 3 matmul over B x V instances)
    blend = (m.weights @ torch.cat([glob_rotmats.reshape(B, J, 9), t], -1)).reshape(B, -1, 4, 3)
    out['vertices'] = (blend[:, :, :3] * vp[:, :, None, :]).sum(-1) + blend[:, :, 3] + tr[:, None]
    return out


INPUT_NAMES = ('pose_rotvecs', 'shape_betas', 'trans', 'kid_factor', 'rel_rotmats', 'glob_rotmats')


def grads(m, inputs, cot, return_vertices=True):
    """fp64 gradients of sum(cot[k] * forward(**inputs)[k]) w.r.t. every tensor of ``inputs`` (numpy in, numpy out)."""
    ts = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in inputs.items() if v is not None}
    out = forward(m, **ts, return_vertices=return_vertices)
    loss = sum((out[k] * torch.as_tensor(np.asarray(c, np.float64))).sum() for k, c in cot.items()
               if c is not None and k in out)
    names = list(ts)
    if not isinstance(loss, torch.Tensor) or not loss.requires_grad:  # (no cotangent reaches an input)
        return {k: np.zeros(ts[k].shape) for k in names}
    gs = torch.autograd.grad(loss, [ts[k] for k in names], allow_unused=True)
    return {k: (np.zeros(ts[k].shape) if g is None else g.numpy()) for k, g in zip(names, gs)}


def random_rotmats(rs, shape):
    """Orthonormal rotations (Gram-Schmidt of Gaussian 3 x 3)."""
    q, r = np.linalg.qr(rs.randn(*shape, 3, 3))
    q = q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[..., None, :]
    det = np.linalg.det(q)
    q[..., :, 0] *= det[..., None]
    return q


WHICH = ('vertices', 'joints', 'orientations')
# the cases of golden_forward_grad.npz (tests/golden/make_golden_forward_grad.py)
CASES = ('pose', 'rel', 'glob', 'norot', 'novert', 'trans13', 'kidscalar', 'kid', 'extrabetas')


def model_dir(tag):
    """Directory of a model kind of the gradient tests under the synthetic model root: util.model_dir, plus smpl_b300
    (its own directory: 300 betas)."""
    import util

    return tag if tag == 'smpl_b300' else util.model_dir(tag)


def cotangents(seed, B, J, V, which=WHICH):
    """The seeded cotangents of golden_forward_grad.npz (not stored in the fixture)."""
    rs = np.random.RandomState(seed)
    c = dict(vertices=rs.randn(B, V, 3), joints=rs.randn(B, J, 3), orientations=rs.randn(B, J, 3, 3))
    return {k: c[k].astype(np.float32) for k in which}
