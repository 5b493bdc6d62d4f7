"""``BodyFlipperOpt`` — the closed-form flip followed by gradient refinement (counterpart of the reference's
``smplfitter.pt.BodyFlipperOpt``, src/smplfitter/pt/bodyflipper_opt.py; same ``flip`` signature, defaults and result keys).

``BodyFlipper.flip`` gives the start.  With ``refine_steps > 0`` the start is refined by Adam against the mirrored mesh
``flip_vertices(forward(inputs))``, minimising the mean vertex distance over the relative rotations (6D form: the first
two columns of each matrix, orthonormalised by Gram-Schmidt), the betas, the translation and the kid factor.  The
learning rate rises linearly over the first ``int(refine_steps * warmup_ratio)`` steps, then follows a half cosine.

The optimizer and the 6D map run in PyTorch, on a few hundred floats per instance.  The vertex-sized work of a step is
one native call (``smplfit_mesh_objective_f32`` through ``BodyModel._objective_direct``): the loss and its gradient
with respect to the rotation matrices, betas, translation and kid factor, with neither the vertices nor their cotangent
written to memory.  ``fused_objective=False`` runs the same loop through ``BodyModel.forward``'s autograd with the loss
in PyTorch operators (the yardstick of the tests and of tools/bench_flip_opt.py).
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from ._autograd import mat2rotvec, rotvec2mat
from .bodyfitter_opt import _gram_schmidt, _six
from .bodyflipper import BodyFlipper


def refine_lr_at(step: int, steps: int, lr: float, warmup_ratio: float) -> float:
    """Learning rate of refinement step ``step`` of ``steps``: linear warm-up over ``int(steps * warmup_ratio)`` steps
    (none when that is 0), then a half cosine from ``lr`` towards 0."""
    warm = int(steps * warmup_ratio)
    if step < warm:
        return lr * (step + 1) / warm
    progress = (step - warm) / max(1, steps - warm)
    return lr * 0.5 * (1.0 + math.cos(math.pi * progress))


class BodyFlipperOpt(nn.Module):
    """Closed-form flip, optionally refined by Adam on the mean vertex distance to the mirrored mesh."""

    def __init__(self, body_model, fused_objective: bool = True):
        super().__init__()
        self.body_model = body_model
        self.fused_objective = fused_objective
        self.flipper = BodyFlipper(body_model)

    def flip(
        self,
        pose_rotvecs: torch.Tensor,
        shape_betas: torch.Tensor,
        trans: torch.Tensor,
        kid_factor: Optional[torch.Tensor] = None,
        num_iter: int = 1,
        refine_steps: int = 0,
        refine_lr: float = 0.03,
        warmup_ratio: float = 0.1,
    ) -> dict[str, torch.Tensor]:
        """The parameters of the x-mirrored body: ``pose_rotvecs``, ``shape_betas``, ``trans`` and ``kid_factor`` (always
        a tensor, as in ``BodyFlipper.flip``).  ``refine_steps=0`` (and an empty batch) returns ``BodyFlipper.flip``'s
        result unchanged.  Inputs that require gradients raise ``NotImplementedError``, and so does a refinement while
        ``torch.compile`` is tracing."""
        if any(isinstance(t, torch.Tensor) and t.requires_grad for t in (pose_rotvecs, shape_betas, trans, kid_factor)):
            raise NotImplementedError('the HIP flip is not differentiable; detach the inputs')
        if refine_steps > 0 and torch.compiler.is_compiling():
            raise NotImplementedError('the refinement (an optimizer loop) cannot be traced; call it outside torch.compile')
        init = self.flipper.flip(pose_rotvecs, shape_betas, trans, kid_factor, num_iter)
        if refine_steps == 0 or pose_rotvecs.shape[0] == 0:
            return init
        with torch.no_grad():
            inp = self.body_model(pose_rotvecs, shape_betas, trans, kid_factor=kid_factor)
            target = self.flipper.flip_vertices(inp['vertices'])
        return self._refine(target, init, refine_steps, refine_lr, warmup_ratio)

    def _refine(self, target, init, steps, lr, warmup_ratio):
        m = self.body_model
        B, J, V = target.shape[0], m.num_joints, m.num_vertices
        with torch.no_grad():
            six = _six(rotvec2mat(init['pose_rotvecs'].detach().reshape(B, J, 3)))
        six = six.clone().requires_grad_(True)
        betas = init['shape_betas'].detach().clone().requires_grad_(True)
        trans = init['trans'].detach().clone().requires_grad_(True)
        kid = init['kid_factor'].detach().clone().requires_grad_(True)
        opt = torch.optim.Adam([six, betas, trans, kid], lr=lr, betas=(0.97, 0.999))
        scale = 1.0 / (B * V)  # the mean over all B * V vertex distances
        for step in range(steps):
            for group in opt.param_groups:
                group['lr'] = refine_lr_at(step, steps, lr, warmup_ratio)
            opt.zero_grad()
            rot = _gram_schmidt(six)
            if self.fused_objective:
                _, g = m._objective_direct(target, shape_betas=betas, trans=trans, kid_factor=kid,
                                           rel_rotmats=rot.detach(), scale=scale)
                rot.backward(g[4])
                betas.grad, trans.grad, kid.grad = g[1], g[2], g[3]
            else:
                out = m(rel_rotmats=rot, shape_betas=betas, trans=trans, kid_factor=kid)
                torch.mean(torch.linalg.norm(out['vertices'] - target, dim=-1)).backward()
            opt.step()
        with torch.no_grad():
            pose = mat2rotvec(_gram_schmidt(six)).reshape(B, J * 3)
        return dict(pose_rotvecs=pose, shape_betas=betas.detach(), trans=trans.detach(), kid_factor=kid.detach())
