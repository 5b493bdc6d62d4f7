"""``BodyFitterOpt`` — the closed-form fit followed by gradient refinement (counterpart of the reference's
``smplfitter.pt.BodyFitterOpt``, src/smplfitter/pt/bodyfitter_opt.py; same constructor, ``fit`` signature and result keys).

The closed-form ``BodyFitter.fit`` gives the start.  With ``refine_steps > 0`` the start is refined by Adam over the
global rotations (6D form: the first two columns of each matrix, orthonormalised by Gram-Schmidt), the betas, the
translation and the kid factor, minimising the mean vertex (and joint) distance plus a ridge on the betas from the third
on.  The learning rate rises linearly over the first ``warmup_ratio`` of the steps, then follows a half cosine to zero.
The result is returned as relative rotation vectors, as the closed-form fit returns it.

The optimizer, the 6D map and the beta ridge run in PyTorch, on a few hundred floats per instance.  The vertex- and
joint-sized work of a step is one native call (``smplfit_fit_objective_f32``, or ``smplfit_mesh_objective_f32`` without
target joints, through ``BodyModel._objective_direct``): the loss and its gradient with respect to the global rotation
matrices, betas, translation and kid factor, with neither the mesh nor its cotangent written to memory.
``fused_objective=False`` runs the same loop through ``BodyModel.forward`` and its HIP backward
(``smplfit_forward_backward_f32``) with the loss in PyTorch operators (the yardstick of the tests and of
tools/bench_fitter_opt.py).
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from ._autograd import mat2rotvec, rotvec2mat
from .bodyfitter import BodyFitter


def _gram_schmidt(six: torch.Tensor) -> torch.Tensor:
    """(..., 6) -> (..., 3, 3): columns u, v, u x v from the two 3-vectors of ``six``, orthonormalised."""
    u = six[..., :3]
    u = u / (torch.linalg.norm(u, dim=-1, keepdim=True) + 1e-8)
    v = six[..., 3:]
    v = v - (u * v).sum(-1, keepdim=True) * u
    v = v / (torch.linalg.norm(v, dim=-1, keepdim=True) + 1e-8)
    return torch.stack([u, v, torch.linalg.cross(u, v)], dim=-1)


def _six(rot: torch.Tensor) -> torch.Tensor:
    return torch.cat([rot[..., :, 0], rot[..., :, 1]], dim=-1)


class BodyFitterOpt(nn.Module):
    """Closed-form fit, optionally refined by Adam on the mean vertex (and joint) distance."""

    def __init__(self, body_model, enable_kid: bool = False, fused_objective: bool = True):
        super().__init__()
        self.body_model = body_model
        self.enable_kid = enable_kid
        self.fused_objective = fused_objective
        self.fitter = BodyFitter(body_model, enable_kid=enable_kid)

    def fit(
        self,
        target_vertices: torch.Tensor,
        target_joints: Optional[torch.Tensor] = None,
        vertex_weights: Optional[torch.Tensor] = None,
        joint_weights: Optional[torch.Tensor] = None,
        num_iter: int = 1,
        beta_regularizer: float = 1,
        beta_regularizer2: float = 0,
        share_beta: bool = False,
        final_adjust_rots: bool = True,
        scale_target: bool = False,
        scale_fit: bool = False,
        refine_steps: int = 0,
        refine_lr: float = 0.03,
        warmup_ratio: float = 0.5,
    ) -> dict[str, torch.Tensor]:
        """``pose_rotvecs``, ``shape_betas``, ``trans`` (and ``kid_factor`` with ``enable_kid``).  ``refine_steps=0``
        (and an empty batch) returns the closed-form fit unchanged; otherwise the fit runs without its final rotation
        adjustment and is refined (module docstring).  A refinement while ``torch.compile`` is tracing raises
        ``NotImplementedError``."""
        if refine_steps > 0 and torch.compiler.is_compiling():
            raise NotImplementedError('the refinement (an optimizer loop) cannot be traced; call it outside torch.compile')
        start = self.fitter.fit(
            target_vertices, target_joints=target_joints, vertex_weights=vertex_weights, joint_weights=joint_weights,
            num_iter=num_iter, beta_regularizer=beta_regularizer, beta_regularizer2=beta_regularizer2,
            share_beta=share_beta, final_adjust_rots=final_adjust_rots if refine_steps == 0 else False,
            scale_target=scale_target, scale_fit=scale_fit, requested_keys=['pose_rotvecs', 'shape_betas', 'trans'])
        if refine_steps == 0 or target_vertices.shape[0] == 0:
            return start
        return self._refine(target_vertices, target_joints, vertex_weights, joint_weights, start, beta_regularizer,
                            refine_steps, refine_lr, warmup_ratio)

    def _refine(self, target_vertices, target_joints, vertex_weights, joint_weights, start, beta_regularizer, steps,
                lr, warmup_ratio):
        from .bodyflipper_opt import refine_lr_at  # (that module imports this one's 6D helpers)

        m = self.body_model
        J, V, parents = m.num_joints, m.num_vertices, m.kintree_parents
        B = target_vertices.shape[0]
        with torch.no_grad():
            rel = rotvec2mat(start['pose_rotvecs'].reshape(B, J, 3))
            glob = [rel[:, 0]]
            for j in range(1, J):
                glob.append(glob[int(parents[j])] @ rel[:, j])
            six = _six(torch.stack(glob, 1))
        six = six.clone().requires_grad_(True)
        betas = start['shape_betas'].detach().clone().requires_grad_(True)
        trans = start['trans'].detach().clone().requires_grad_(True)
        params = [six, betas, trans]
        kid = None
        if 'kid_factor' in start:
            kid = start['kid_factor'].detach().clone().requires_grad_(True)
            params.append(kid)
        opt = torch.optim.Adam(params, lr=lr, betas=(0.97, 0.999))

        def mean_dist(pred, target, weights):
            d = torch.linalg.norm(pred - target, dim=-1)
            return torch.mean(d if weights is None else weights * d)

        ridge = beta_regularizer > 0 and betas.shape[1] > 2
        for step in range(steps):
            for group in opt.param_groups:
                group['lr'] = refine_lr_at(step, steps, lr, warmup_ratio)
            opt.zero_grad()
            rot = _gram_schmidt(six)
            if self.fused_objective:
                # the means over all B * V vertex and B * J joint distances
                _, g = m._objective_direct(
                    target_vertices, glob_rotmats=rot.detach(), shape_betas=betas, trans=trans, kid_factor=kid,
                    vertex_weights=vertex_weights, scale=1.0 / (B * V), target_joints=target_joints,
                    joint_weights=joint_weights, joint_scale=1.0 / (B * J))
                rot.backward(g[5])
                betas.grad, trans.grad = g[1], g[2]
                if kid is not None:
                    kid.grad = g[3]
                if ridge:
                    with torch.no_grad():  # d/dbetas of beta_regularizer * mean(betas[:, 2:] ** 2)
                        betas.grad[:, 2:] += (2.0 * beta_regularizer / betas[:, 2:].numel()) * betas[:, 2:]
            else:
                out = m(glob_rotmats=rot, shape_betas=betas, trans=trans, kid_factor=kid)
                loss = mean_dist(out['vertices'], target_vertices, vertex_weights)
                if target_joints is not None:
                    loss = loss + mean_dist(out['joints'], target_joints, joint_weights)
                if ridge:
                    loss = loss + beta_regularizer * torch.mean(betas[:, 2:] ** 2)
                loss.backward()
            opt.step()
        with torch.no_grad():
            glob = _gram_schmidt(six)
            idx = torch.as_tensor([int(p) for p in parents[1:]], device=glob.device)
            parent = torch.cat([torch.eye(3, device=glob.device, dtype=glob.dtype).expand(B, 1, 3, 3),
                                glob[:, idx]], dim=1)
            pose = mat2rotvec(parent.transpose(-1, -2) @ glob).reshape(B, J * 3)
        res = dict(pose_rotvecs=pose, shape_betas=betas.detach(), trans=trans.detach())
        if kid is not None:
            res['kid_factor'] = kid.detach()
        return res
