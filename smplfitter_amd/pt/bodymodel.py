"""``BodyModel`` — same surface as ``smplfitter.pt.BodyModel`` (reference
src/smplfitter/pt/bodymodel.py:12-453), with ``forward`` dispatched to the HIP LBS kernels through the
C-ABI (``smplfit_forward_f32``) and ``rototranslate`` to its own kernel (``smplfit_rototranslate_f32``).  One
extension of that surface: ``rototranslate`` also takes a batch.  PyTorch tensors are containers only: device memory +
stream.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib, modelio


_NO_CPU_PATH = (
    'smplfitter_amd runs on MI355X through its HIP kernels only: move the model and the '
    "inputs to a 'cuda' (ROCm) device. There is no CPU path."
)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class BodyModel(nn.Module):
    """Statistical body model of the SMPL family (forward = blend shapes + FK + linear blend
    skinning).  Constructor arguments, buffers and attributes follow the reference
    (pt/bodymodel.py:53-119)."""

    def __init__(
        self,
        model_name: str = 'smpl',
        gender: str = 'neutral',
        model_root: Optional[str] = None,
        num_betas: Optional[int] = None,
        vertex_subset_size: Optional[int] = None,
        vertex_subset=None,
        faces=None,
        joint_regressor_post_lbs=None,
        device=None,
    ):
        super().__init__()
        self.gender = gender
        self.model_name = model_name
        if isinstance(vertex_subset, torch.Tensor):
            vertex_subset = vertex_subset.cpu().numpy()
        data = modelio.load_model(
            model_name, gender, model_root, num_betas, vertex_subset_size, vertex_subset, faces,
            joint_regressor_post_lbs,
        )
        f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)  # noqa: E731
        self.v_template = nn.Buffer(f32(data.v_template))
        self.shapedirs = nn.Buffer(f32(data.shapedirs))
        self.posedirs = nn.Buffer(f32(data.posedirs))
        self.J_regressor_post_lbs = nn.Buffer(f32(data.J_regressor_post_lbs))
        self.J_template = nn.Buffer(f32(data.J_template))
        self.J_shapedirs = nn.Buffer(f32(data.J_shapedirs))
        self.kid_shapedir = nn.Buffer(f32(data.kid_shapedir))
        self.kid_J_shapedir = nn.Buffer(f32(data.kid_J_shapedir))
        self.weights = nn.Buffer(f32(data.weights))
        self.kintree_parents_tensor = nn.Buffer(torch.tensor(data.kintree_parents, dtype=torch.int64))
        self.kintree_parents = data.kintree_parents
        self.faces = data.faces
        self.num_joints = data.num_joints
        self.num_vertices = data.num_vertices
        self.num_betas = self.shapedirs.shape[2]
        self.vertex_subset = data.vertex_subset
        self.joint_names = data.joint_names
        if self.vertex_subset is None:
            self.vertex_subset = np.arange(self.num_vertices)
        self._handles = {}  # device index -> _lib.Handle (model constants uploaded to that GPU)
        from . import ops

        ops.register_model(self)  # id for the torch.library operators (read while compiling)
        if device is not None:
            self.to(device)

    # -- native handle ---------------------------------------------------------------------------
    def _native(self, device: torch.device, kid: bool = False) -> _lib.Handle:
        """The C-ABI handle holding this model's constants on ``device`` (created on first use).
        ``kid=True``: the variant whose last shape unknown is the kid blend shape."""
        if device.type != 'cuda':
            raise RuntimeError(_NO_CPU_PATH)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        h = self._handles.get((idx, kid))
        if h is None:
            reg = self.J_regressor_post_lbs
            desc, keep = _lib.make_desc(
                self.v_template.cpu().numpy(), self.shapedirs.cpu().numpy(),
                self.posedirs.cpu().numpy(), self.weights.cpu().numpy(),
                self.J_template.cpu().numpy(), self.J_shapedirs.cpu().numpy(), self.kintree_parents,
                reg.cpu().numpy() if reg.shape[1] == self.num_vertices else None,
                is_smpl_family=self.model_name.startswith('smpl'),
                kid_shapedir=self.kid_shapedir.cpu().numpy() if kid else None,
                kid_J_shapedir=self.kid_J_shapedir.cpu().numpy() if kid else None,
            )
            with torch.cuda.device(idx):
                h = _lib.Handle(desc)
            self._handles[(idx, kid)] = h
        return h

    def kernel_path(self, device: Optional[torch.device] = None, enable_kid: bool = False) -> str:
        """Which kernel family fits and forward passes of this model run on (``smplfit_info.vertex_path``):
        ``'batch-major'`` (<= 8 skinning weights per vertex, <= 16 betas: the rates of the benchmark configurations),
        ``'wave-per-instance'`` (small vertex subsets, non-normalised weights: about 0.4 x the rate) or
        ``'general'`` (any other ``num_betas`` — e.g. the default ``None``: every column of the file — or more than eight
        weights per vertex: run-time loops, a correctness path whose per-call workspace holds an S x S fp64 system per
        instance — about 1.7 MB per instance at 300 betas).  No counterpart in the reference."""
        device = self.v_template.device if device is None else torch.device(device)
        return ('wave-per-instance', 'batch-major', 'general')[int(self._native(device, kid=enable_kid).info.vertex_path)]

    @staticmethod
    def _workspace(h: _lib.Handle, batch: int, device) -> torch.Tensor:
        return torch.empty(h.workspace_bytes(batch), dtype=torch.uint8, device=device)

    # -- forward ---------------------------------------------------------------------------------
    def forward(
        self,
        pose_rotvecs: Optional[torch.Tensor] = None,
        shape_betas: Optional[torch.Tensor] = None,
        trans: Optional[torch.Tensor] = None,
        kid_factor: Optional[torch.Tensor] = None,
        rel_rotmats: Optional[torch.Tensor] = None,
        glob_rotmats: Optional[torch.Tensor] = None,
        return_vertices: bool = True,
    ) -> dict[str, torch.Tensor]:
        """Vertices, joints and global orientations for a batch (pt/bodymodel.py:121-307).

        Differentiable: when gradients are enabled and a tensor input requires grad, the outputs carry a ``grad_fn``
        whose backward is the HIP vector-Jacobian product (``smplfit_forward_backward_f32``) with respect to
        ``pose_rotvecs`` / ``rel_rotmats`` / ``glob_rotmats``, ``shape_betas``, ``trans`` and ``kid_factor``.  The
        model buffers are constants: they get no gradient.  Once differentiable (no double backward).  One
        divergence from the reference: at a rotation vector of exactly zero the gradient is the true derivative of
        the exponential map, not 0."""
        if torch.compiler.is_compiling():  # one opaque operator for torch.compile / export
            kid = kid_factor
            if kid is not None and not isinstance(kid, torch.Tensor):
                kid = torch.as_tensor(kid, dtype=torch.float32, device=self.v_template.device)
            j, o, v = torch.ops.smplfitter_amd.forward(
                self._model_id, pose_rotvecs, shape_betas, trans, kid, rel_rotmats, glob_rotmats,
                return_vertices)
            res = dict(joints=j, orientations=o)
            if return_vertices:
                res['vertices'] = v
            return res
        args = (pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats)
        if torch.is_grad_enabled() and any(isinstance(a, torch.Tensor) and a.requires_grad for a in args):
            j, o, v = _ForwardFn.apply(self, return_vertices, *args)
            res = dict(joints=j, orientations=o)
            if return_vertices:
                res['vertices'] = v
            return res
        return self._forward_direct(pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats,
                                    glob_rotmats, return_vertices)

    def _grad_inputs(self, batch, pose_rotvecs, shape_betas, kid_factor, rel_rotmats, glob_rotmats):
        """The inputs of the gradient calls as detached contiguous fp32 tensors on the model's device: (pose, glob, rel,
        betas cut to the model's ``num_betas``, their count, kid_factor expanded to the batch)."""
        device = self.v_template.device
        J = self.num_joints
        prep = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        rel = prep(rel_rotmats.reshape(batch, J, 3, 3)) if rel_rotmats is not None else None
        pose = prep(pose_rotvecs.reshape(batch, J * 3)) if pose_rotvecs is not None else None
        glob = prep(glob_rotmats)
        betas = prep(shape_betas)
        nb = 0
        if betas is not None:
            nb = min(betas.shape[1], self.num_betas)
            betas = betas[:, :nb].contiguous()
            if nb == 0:
                betas = None
        kid = None
        if isinstance(kid_factor, torch.Tensor):
            kid = kid_factor.detach().to(device=device, dtype=torch.float32).reshape(-1)
            kid = kid.expand(batch).contiguous() if kid.numel() == 1 else kid.contiguous()
        elif kid_factor is not None:
            kid = torch.full((batch,), float(kid_factor), dtype=torch.float32, device=device)
        return pose, glob, rel, betas, nb, kid

    def _backward_direct(self, pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats,
                         grad_joints=None, grad_orientations=None, grad_vertices=None):
        """The C-ABI call behind ``forward``'s backward (``smplfit_forward_backward_f32``): the gradients of the six
        inputs (None for an input not given), each in the caller's shape and dtype — broadcasts of ``trans`` (1, 3) and
        of a one-element ``kid_factor`` summed over the batch, betas beyond the model's ``num_betas`` zero."""
        device = self.v_template.device
        J = self.num_joints
        batch = 0
        for arg in (pose_rotvecs, shape_betas, trans, rel_rotmats, glob_rotmats):
            if arg is not None:
                batch = arg.shape[0]
                break
        ins = (pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats)
        zeros = [None if a is None or not isinstance(a, torch.Tensor) else torch.zeros_like(a) for a in ins]
        if batch == 0:
            return zeros
        prep = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        pose, glob, rel, betas, nb, kid = self._grad_inputs(batch, pose_rotvecs, shape_betas, kid_factor, rel_rotmats,
                                                            glob_rotmats)
        g = lambda t: None if t is None or t.numel() == 0 else prep(t)  # noqa: E731
        gj, go, gv = g(grad_joints), g(grad_orientations), g(grad_vertices)
        new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)  # noqa: E731
        g_pose = new(batch, J * 3) if pose is not None else None
        g_rel = new(batch, J, 3, 3) if rel is not None else None
        g_glob = new(batch, J, 3, 3) if glob is not None else None
        g_betas = new(batch, nb) if betas is not None else None
        g_trans = new(batch, 3) if trans is not None else None
        g_kid = new(batch) if isinstance(kid_factor, torch.Tensor) else None
        h = self._native(device, kid=kid is not None)
        ws = torch.empty(h.forward_backward_workspace_bytes(batch), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            args = _lib.ForwardBackwardArgs(
                pose_rotvecs=p(pose), glob_rotmats=p(glob), rel_rotmats=p(rel), shape_betas=p(betas),
                num_betas_given=nb, trans=None, kid_factor=p(kid), batch=batch, grad_vertices=p(gv),
                grad_joints=p(gj), grad_orientations=p(go), grad_pose_rotvecs=p(g_pose),
                grad_glob_rotmats=p(g_glob), grad_rel_rotmats=p(g_rel), grad_shape_betas=p(g_betas),
                grad_trans=p(g_trans), grad_kid_factor=p(g_kid), workspace=ws.data_ptr(),
                workspace_bytes=ws.numel(), hip_stream=stream)
            _lib.check(_lib.load().smplfit_forward_backward_f32(h.ptr, C.byref(args)))
        return self._grad_outputs(ins, zeros, batch, nb, g_pose, g_betas, g_trans, g_kid, g_rel, g_glob)

    def _grad_outputs(self, ins, zeros, batch, nb, g_pose, g_betas, g_trans, g_kid, g_rel, g_glob):
        """The native gradients in the callers' shapes and dtypes (``_backward_direct``)."""
        pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats = ins
        out = list(zeros)
        if g_pose is not None:
            out[0] = g_pose.reshape(pose_rotvecs.shape).to(pose_rotvecs.dtype)
        if shape_betas is not None:
            gb = torch.zeros(shape_betas.shape, dtype=torch.float32, device=self.v_template.device)
            if g_betas is not None:
                gb[:, :nb] = g_betas
            out[1] = gb.to(shape_betas.dtype)
        if g_trans is not None:
            gt = g_trans if trans.shape[0] == batch else g_trans.sum(0, keepdim=True)
            out[2] = gt.reshape(trans.shape).to(trans.dtype)
        if g_kid is not None:
            gk = g_kid.sum() if kid_factor.numel() == 1 and batch != 1 else g_kid
            out[3] = gk.reshape(kid_factor.shape).to(kid_factor.dtype)
        if g_rel is not None:
            out[4] = g_rel.reshape(rel_rotmats.shape).to(rel_rotmats.dtype)
        if g_glob is not None:
            out[5] = g_glob.reshape(glob_rotmats.shape).to(glob_rotmats.dtype)
        return out

    def _objective_direct(self, target_vertices, pose_rotvecs=None, shape_betas=None, trans=None, kid_factor=None,
                          rel_rotmats=None, glob_rotmats=None, vertex_weights=None, scale: float = 1.0,
                          target_joints=None, joint_weights=None, joint_scale: float = 1.0):
        """Value and gradient of the mesh-distance objective in one C-ABI call (``smplfit_mesh_objective_f32``):
        ``loss`` (B) with ``loss[b] = scale * sum_v w_bv |forward(inputs).vertices_bv - target_bv|``, and the gradients
        of ``loss.sum()`` with respect to the six inputs, prepared and returned as ``_backward_direct`` does (a
        broadcast ``trans`` / ``kid_factor`` is expanded on the way in and its gradient summed on the way out).  The
        vertices and their cotangent are never written to memory.  With ``target_joints`` (B, J, 3) the call is
        ``smplfit_fit_objective_f32`` and the loss gains ``joint_scale * sum_j u_bj |forward(inputs).joints_bj -
        target_joints_bj|``, ``u`` = ``joint_weights`` (B, J) or 1.  Returns ``(loss, grads)``."""
        device = self.v_template.device
        J, V = self.num_joints, self.num_vertices
        batch = target_vertices.shape[0]
        if tuple(target_vertices.shape) != (batch, V, 3):
            raise ValueError(f'target_vertices must have shape (batch, {V}, 3), got {tuple(target_vertices.shape)}')
        ins = (pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats)
        if sum(x is not None for x in (pose_rotvecs, rel_rotmats, glob_rotmats)) > 1:
            raise ValueError('Only one rotation input may be provided (pose_rotvecs, rel_rotmats, or glob_rotmats).')
        zeros = [None if a is None or not isinstance(a, torch.Tensor) else torch.zeros_like(a) for a in ins]
        loss = torch.zeros(batch, dtype=torch.float32, device=device)
        if batch == 0:
            return loss, zeros
        prep = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        pose, glob, rel, betas, nb, kid = self._grad_inputs(batch, pose_rotvecs, shape_betas, kid_factor, rel_rotmats,
                                                            glob_rotmats)
        tr = prep(trans)
        if tr is not None and tr.shape[0] != batch:
            tr = tr.expand(batch, 3).contiguous()
        target = prep(target_vertices)
        vw = prep(vertex_weights)
        if vw is not None and tuple(vw.shape) != (batch, V):
            raise ValueError(f'vertex_weights must have shape (batch, {V}), got {tuple(vw.shape)}')
        tj, jw = prep(target_joints), prep(joint_weights)
        if tj is not None and tuple(tj.shape) != (batch, J, 3):
            raise ValueError(f'target_joints must have shape (batch, {J}, 3), got {tuple(tj.shape)}')
        if jw is not None and tuple(jw.shape) != (batch, J):
            raise ValueError(f'joint_weights must have shape (batch, {J}), got {tuple(jw.shape)}')
        if jw is not None and tj is None:
            raise ValueError('joint_weights without target_joints')
        new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)  # noqa: E731
        g_pose = new(batch, J * 3) if pose is not None else None
        g_rel = new(batch, J, 3, 3) if rel is not None else None
        g_glob = new(batch, J, 3, 3) if glob is not None else None
        g_betas = new(batch, nb) if betas is not None else None
        g_trans = new(batch, 3) if trans is not None else None
        g_kid = new(batch) if isinstance(kid_factor, torch.Tensor) else None
        h = self._native(device, kid=kid is not None)
        nws = h.mesh_objective_workspace_bytes(batch) if tj is None else h.fit_objective_workspace_bytes(batch)
        ws = torch.empty(nws, dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            common = dict(
                pose_rotvecs=p(pose), glob_rotmats=p(glob), rel_rotmats=p(rel), shape_betas=p(betas),
                num_betas_given=nb, trans=p(tr), kid_factor=p(kid), batch=batch, target_vertices=p(target),
                vertex_weights=p(vw), scale=float(scale), loss=p(loss), grad_pose_rotvecs=p(g_pose),
                grad_glob_rotmats=p(g_glob), grad_rel_rotmats=p(g_rel), grad_shape_betas=p(g_betas),
                grad_trans=p(g_trans), grad_kid_factor=p(g_kid), workspace=ws.data_ptr(),
                workspace_bytes=ws.numel(), hip_stream=stream)
            if tj is None:
                args = _lib.MeshObjectiveArgs(**common)
                _lib.check(_lib.load().smplfit_mesh_objective_f32(h.ptr, C.byref(args)))
            else:
                args = _lib.FitObjectiveArgs(target_joints=p(tj), joint_weights=p(jw), joint_scale=float(joint_scale),
                                             **common)
                _lib.check(_lib.load().smplfit_fit_objective_f32(h.ptr, C.byref(args)))
        return loss, self._grad_outputs(ins, zeros, batch, nb, g_pose, g_betas, g_trans, g_kid, g_rel, g_glob)

    def _forward_direct(self, pose_rotvecs=None, shape_betas=None, trans=None, kid_factor=None,
                        rel_rotmats=None, glob_rotmats=None, return_vertices: bool = True):
        """The C-ABI call behind ``forward`` (and behind the ``smplfitter_amd::forward`` operator)."""
        self._check_forward_inputs(pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats)
        device = self.v_template.device
        J, V = self.num_joints, self.num_vertices
        batch = 0
        for arg in (pose_rotvecs, shape_betas, trans, rel_rotmats, glob_rotmats):
            if arg is not None:
                batch = arg.shape[0]
                break
        if batch == 0:
            res = dict(
                joints=torch.empty((0, J, 3), device=device),
                orientations=torch.empty((0, J, 3, 3), device=device),
            )
            if return_vertices:
                res['vertices'] = torch.empty((0, V, 3), device=device)
            return res
        pose, glob, rel, betas, nb, tr, kid = self._prep_forward_inputs(batch, pose_rotvecs, shape_betas, trans, kid_factor,
                                                                        rel_rotmats, glob_rotmats)
        h = self._native(device, kid=kid is not None)
        ws = self._workspace(h, batch, device)
        joints = torch.empty((batch, J, 3), dtype=torch.float32, device=device)
        orient = torch.empty((batch, J, 3, 3), dtype=torch.float32, device=device)
        verts = torch.empty((batch, V, 3), dtype=torch.float32, device=device) if return_vertices else None
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            args = _lib.ForwardArgs(
                pose_rotvecs=p(pose), glob_rotmats=p(glob), rel_rotmats=p(rel), shape_betas=p(betas),
                num_betas_given=nb, trans=p(tr), kid_factor=p(kid), batch=batch, vertices=p(verts),
                joints=p(joints), orientations=p(orient), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                hip_stream=stream)
            _lib.check(_lib.load().smplfit_forward_ex_f32(h.ptr, C.byref(args)))
        res = dict(joints=joints, orientations=orient)
        if return_vertices:
            res['vertices'] = verts
        return res

    @staticmethod
    def _check_forward_inputs(pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats):
        """The input checks of ``forward`` (and of ``mesh_error``): one rotation form, batched torch tensors."""
        n_rot = sum(x is not None for x in (pose_rotvecs, rel_rotmats, glob_rotmats))
        if n_rot > 1:
            raise ValueError(
                'Only one rotation input may be provided '
                '(pose_rotvecs, rel_rotmats, or glob_rotmats).'
            )
        for name, arg, min_ndim in [
            ('pose_rotvecs', pose_rotvecs, 2), ('shape_betas', shape_betas, 2), ('trans', trans, 2),
            ('kid_factor', kid_factor, 1), ('rel_rotmats', rel_rotmats, 4),
            ('glob_rotmats', glob_rotmats, 4),
        ]:
            if arg is not None:
                if isinstance(arg, np.ndarray):
                    raise TypeError(
                        f"Expected torch.Tensor for '{name}', got numpy.ndarray. "
                        f'Convert with torch.from_numpy() or torch.as_tensor().'
                    )
                if arg.ndim < min_ndim:
                    raise ValueError(
                        f"Expected batched input for '{name}' with at least "
                        f'{min_ndim} dimensions, but got shape {tuple(arg.shape)}. '
                        f'For single (unbatched) inputs, use model.single() instead.'
                    )

    def _prep_forward_inputs(self, batch, pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats):
        """The inputs of a forward call as contiguous fp32 tensors on the model's device: (pose, glob, rel, betas cut to
        the model's ``num_betas``, their count, trans and kid_factor expanded to the batch)."""
        device = self.v_template.device
        J = self.num_joints
        prep = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        # rel_rotmats: the kinematic chain of pt/bodymodel.py:230-234 runs inside the joint kernel
        rel = prep(rel_rotmats.reshape(batch, J, 3, 3)) if rel_rotmats is not None else None
        pose = prep(pose_rotvecs.reshape(batch, J * 3)) if pose_rotvecs is not None else None
        glob = prep(glob_rotmats)
        betas = prep(shape_betas)
        nb = 0
        if betas is not None:
            nb = min(betas.shape[1], self.num_betas)
            betas = betas[:, :nb].contiguous()
            if nb == 0:
                betas = None
        tr = prep(trans)
        if tr is not None and tr.shape[0] != batch:
            tr = tr.expand(batch, 3).contiguous()
        kid = None
        if kid_factor is not None:
            kid = torch.as_tensor(kid_factor, dtype=torch.float32, device=device).reshape(-1)
            kid = kid.expand(batch).contiguous() if kid.numel() == 1 else kid.contiguous()
        return pose, glob, rel, betas, nb, tr, kid

    def single(self, pose_rotvecs=None, shape_betas=None, trans=None, kid_factor=None,
               rel_rotmats=None, glob_rotmats=None, return_vertices: bool = True):
        """Unbatched ``forward`` (pt/bodymodel.py:310-380)."""
        u = lambda t: t.unsqueeze(0) if t is not None else None  # noqa: E731
        if all(x is None for x in (pose_rotvecs, shape_betas, trans, rel_rotmats, glob_rotmats)):
            shape_betas = torch.zeros((0,), dtype=torch.float32, device=self.v_template.device)
            pose_rotvecs = torch.zeros((self.num_joints * 3,), dtype=torch.float32,
                                       device=self.v_template.device)
        res = self.forward(u(pose_rotvecs), u(shape_betas), u(trans), kid_factor, u(rel_rotmats),
                           u(glob_rotmats), return_vertices)
        return {k: v.squeeze(0) for k, v in res.items()}

    # -- mesh error ------------------------------------------------------------------------------
    def mesh_error(
        self,
        target_vertices: torch.Tensor,
        target_joints: Optional[torch.Tensor] = None,
        pose_rotvecs: Optional[torch.Tensor] = None,
        shape_betas: Optional[torch.Tensor] = None,
        trans: Optional[torch.Tensor] = None,
        kid_factor: Optional[torch.Tensor] = None,
        rel_rotmats: Optional[torch.Tensor] = None,
        glob_rotmats: Optional[torch.Tensor] = None,
        return_mesh: bool = False,
        align: str = 'none',
        align_on: str = 'each',
        vertex_weights: Optional[torch.Tensor] = None,
        joint_weights: Optional[torch.Tensor] = None,
    ) -> dict[str, torch.Tensor]:
        """How far the model at the given parameters lies from target points (no counterpart in the reference; DESIGN.md
        §22): ``vertex_error`` (B, V), the Euclidean distance of every vertex of ``forward(...)`` to its row of
        ``target_vertices`` (B, V, 3); with ``target_joints`` (B, J, 3) also ``joint_error`` (B, J); with
        ``return_mesh`` also ``vertices`` and ``joints``, the bits ``forward`` gives.  Unweighted.  One C-ABI call
        (``smplfit_mesh_error_f32``): without ``return_mesh`` the mesh is measured where it is formed and never written
        as (B, V, 3) on the batch-major kernels.  The parameters are those of ``forward``; an empty batch returns empty
        tensors.  With gradients enabled and an input that requires grad, and under ``torch.compile``, the same keys
        come from ``forward`` and PyTorch arithmetic, so they are differentiable like ``forward``.

        ``align`` ('none', 'root', 'translation', 'rigid', 'similarity') moves the model onto the targets
        before it is measured — 'root' joint 0 onto joint 0 (MPJPE), 'similarity' with ``align_on='each'`` the
        Procrustes-aligned errors (PA-PVE, PA-MPJPE); ``align_on`` 'vertices' / 'joints' takes one transform from that
        set for both.  ``vertex_weights`` (B, V) / ``joint_weights`` (B, J) steer the alignment and the row means, not
        the per-point distances.  With an alignment or weights the call (``smplfit_mesh_error_aligned_f32``) also returns
        ``mean_vertex_error`` (B,) (and ``mean_joint_error``), ``align_scale`` (B,), ``align_rotation`` (B, 3, 3),
        ``align_translation`` (B, 3) — the vertices' transform, the joints' for ``align_on='joints'`` and 'root' — and
        with ``align_on='each'`` and target joints ``joint_align_scale`` / ``_rotation`` / ``_translation``.  A row
        without a transform (zero total weight, a non-finite point, ...) is NaN, no other row is.  ``vertices`` stay
        ``forward``'s bits, unaligned."""
        keys = ['vertex_error'] + (['joint_error'] if target_joints is not None else [])
        if return_mesh:
            keys += ['vertices', 'joints']
        params = dict(pose_rotvecs=pose_rotvecs, shape_betas=shape_betas, trans=trans, kid_factor=kid_factor,
                      rel_rotmats=rel_rotmats, glob_rotmats=glob_rotmats)
        if align not in _lib.ALIGN_MODES:
            raise ValueError(f'align must be one of {tuple(_lib.ALIGN_MODES)}, got {align!r}')
        if align_on not in _lib.ALIGN_ON:
            raise ValueError(f'align_on must be one of {tuple(_lib.ALIGN_ON)}, got {align_on!r}')
        aligned = align != 'none' or vertex_weights is not None or joint_weights is not None
        ins = (target_vertices, target_joints, vertex_weights, joint_weights, *params.values())
        composed = torch.compiler.is_compiling() or (
            torch.is_grad_enabled() and any(isinstance(a, torch.Tensor) and a.requires_grad for a in ins))
        if aligned:
            fn = self._aligned_composed if composed else self._aligned_direct
            return fn(keys, target_vertices, target_joints, align, align_on, vertex_weights, joint_weights, **params)
        if composed:
            return self._recon_composed(keys, target_vertices, target_joints, **params)
        return self._recon_direct(keys, target_vertices, target_joints, **params)

    def _check_align(self, keys, target_vertices, target_joints, align, align_on, vertex_weights, joint_weights):
        """The checks of an aligned mesh-error call beyond the step's own (no device needed); returns the batch."""
        batch = self._check_recon_targets(keys, target_vertices, target_joints)
        if target_joints is None:
            if align == 'root':
                raise ValueError("align='root' needs target_joints")
            if align_on == 'joints' and align != 'none':
                raise ValueError("align_on='joints' needs target_joints")
            if joint_weights is not None:
                raise ValueError('joint_weights need target_joints')
        for name, arg, n in (('vertex_weights', vertex_weights, self.num_vertices), ('joint_weights', joint_weights, self.num_joints)):
            if arg is None:
                continue
            if not isinstance(arg, torch.Tensor):
                raise TypeError(f"Expected torch.Tensor for '{name}', got {type(arg).__name__}.")
            if tuple(arg.shape) != (batch, n):
                raise ValueError(f'{name} must have shape ({batch}, {n}), got {tuple(arg.shape)}')
        return batch

    @staticmethod
    def _align_keys(align, align_on, joints):
        """(transform keys of the primary set, of the joints' own) an aligned call returns."""
        names = ('scale', 'rotation', 'translation')
        own = joints and align_on == 'each' and align in ('translation', 'rigid', 'similarity')
        return [f'align_{n}' for n in names], [f'joint_align_{n}' for n in names] if own else []

    def _aligned_composed(self, keys, target_vertices, target_joints, align, align_on, vertex_weights, joint_weights, **params):
        """The keys of an aligned mesh-error call from ``forward`` and PyTorch arithmetic in fp64 (pt/align.py): the route
        of calls that carry gradients or are being traced."""
        from . import align as A

        batch = self._check_align(keys, target_vertices, target_joints, align, align_on, vertex_weights, joint_weights)
        fw = self.forward(**params, return_vertices=True)
        dev = fw['vertices'].device
        to = lambda a: None if a is None else a.to(dev)  # noqa: E731
        tv, tj, vw, jw = to(target_vertices), to(target_joints), to(vertex_weights), to(joint_weights)
        sets = dict(v=(fw['vertices'], tv, vw))
        if tj is not None:
            sets['j'] = (fw['joints'], tj, jw)
        one, eye = torch.ones(batch, dtype=torch.float64, device=dev), torch.eye(3, dtype=torch.float64, device=dev).expand(batch, 3, 3)
        if align == 'none':
            xf = {k: (one, eye, torch.zeros(batch, 3, dtype=torch.float64, device=dev)) for k in sets}
        elif align == 'root':
            x0, y0, w = fw['joints'].to(torch.float64), tj.to(torch.float64), A.weighted_row_mean(tj[..., 0] * 0, jw)
            ok = torch.isfinite(w + (x0.sum((1, 2)) + y0.sum((1, 2))) * 0)
            nan = torch.full_like(one, float('nan'))
            t = torch.where(ok[:, None], y0[:, 0] - x0[:, 0], nan[:, None])
            xf = {k: (torch.where(ok, one, nan), torch.where(ok[:, None, None], eye, nan[:, None, None]), t) for k in sets}
        else:
            src = dict(each=None, vertices='v', joints='j')[align_on]
            solved = {k: A.procrustes(*sets[k], align) for k in sets if src in (None, k)}
            xf = {k: solved[src or k] for k in sets}
        f32 = lambda a: a.to(torch.float32)  # noqa: E731
        out = {}
        if 'vertices' in keys:
            out['vertices'], out['joints'] = fw['vertices'], fw['joints']
        for k, name in (('v', 'vertex'), ('j', 'joint')):
            if k in sets:
                x, y, w = sets[k]
                e = A.aligned_errors(x, y, *xf[k])
                out[f'{name}_error'], out[f'mean_{name}_error'] = f32(e), f32(A.weighted_row_mean(e, w))
        first, own = self._align_keys(align, align_on, tj is not None)
        primary = xf['j'] if (align == 'root' or (align_on == 'joints' and align != 'none')) else xf['v']
        out.update({k: f32(v) for k, v in zip(first, primary)})
        out.update({k: f32(v) for k, v in zip(own, xf.get('j', ()))})
        return out

    def _aligned_direct(self, keys, target_vertices, target_joints, align, align_on, vertex_weights, joint_weights,
                        pose_rotvecs=None, shape_betas=None, trans=None, kid_factor=None, rel_rotmats=None, glob_rotmats=None):
        """The C-ABI call of the aligned mesh-error step (``smplfit_mesh_error_aligned_f32``)."""
        self._check_forward_inputs(pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats)
        batch = self._check_align(keys, target_vertices, target_joints, align, align_on, vertex_weights, joint_weights)
        for name, arg in (('pose_rotvecs', pose_rotvecs), ('shape_betas', shape_betas), ('rel_rotmats', rel_rotmats),
                          ('glob_rotmats', glob_rotmats)):
            if arg is not None and arg.shape[0] != batch:
                raise ValueError(f'{name} has {arg.shape[0]} rows, target_vertices {batch}')
        if trans is not None and trans.shape[0] not in (1, batch):
            raise ValueError(f'trans has {trans.shape[0]} rows, target_vertices {batch}')
        device = self.v_template.device
        J, V = self.num_joints, self.num_vertices
        joints = target_joints is not None
        first, own = self._align_keys(align, align_on, joints)
        shapes = dict(vertices=(batch, V, 3), joints=(batch, J, 3), vertex_error=(batch, V), joint_error=(batch, J))
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=device)  # noqa: E731
        out = {k: new(*shapes[k]) for k in _lib.RECON_KEYS if k in keys}
        out['mean_vertex_error'] = new(batch)
        if joints:
            out['mean_joint_error'] = new(batch)
        for names in (first, own):
            if names:
                out.update({names[0]: new(batch), names[1]: new(batch, 3, 3), names[2]: new(batch, 3)})
        if align == 'none':  # (no transform to solve for: the identity)
            out[first[0]].fill_(1.0)
            out[first[1]].copy_(torch.eye(3, device=device))
            out[first[2]].zero_()
        if batch == 0:
            return out
        prep = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        pose, glob, rel, betas, nb, tr, kid = self._prep_forward_inputs(batch, pose_rotvecs, shape_betas, trans, kid_factor,
                                                                        rel_rotmats, glob_rotmats)
        tv, tj, vw, jw = prep(target_vertices), prep(target_joints), prep(vertex_weights), prep(joint_weights)
        h = self._native(device, kid=kid is not None)
        ws = torch.empty(h.mesh_error_aligned_workspace_bytes(batch), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            args = _lib.MeshErrorArgs(
                pose_rotvecs=p(pose), glob_rotmats=p(glob), rel_rotmats=p(rel), shape_betas=p(betas),
                num_betas_given=nb, trans=p(tr), kid_factor=p(kid), batch=batch, target_vertices=p(tv),
                target_joints=p(tj), **{k: p(out.get(k)) for k in _lib.RECON_KEYS}, workspace=ws.data_ptr(),
                workspace_bytes=ws.numel(), hip_stream=stream)
            xf = {} if align == 'none' else dict(zip(('scale', 'rotation', 'translation'), (p(out[k]) for k in first)))
            xf.update(zip(('joint_scale', 'joint_rotation', 'joint_translation'), (p(out[k]) for k in own)))
            al = _lib.MeshAlignArgs(
                align=_lib.ALIGN_MODES[align], align_on=_lib.ALIGN_ON[align_on], vertex_weights=p(vw), joint_weights=p(jw),
                mean_vertex_error=p(out['mean_vertex_error']), mean_joint_error=p(out.get('mean_joint_error')), **xf)
            _lib.check(_lib.load().smplfit_mesh_error_aligned_f32(h.ptr, C.byref(args), C.byref(al)))
        return out

    def _check_recon_targets(self, keys, target_vertices, target_joints):
        """The target checks of the mesh-error step (no device needed); returns the batch."""
        for name, arg in (('target_vertices', target_vertices), ('target_joints', target_joints)):
            if isinstance(arg, np.ndarray):
                raise TypeError(f"Expected torch.Tensor for '{name}', got numpy.ndarray.")
        J, V = self.num_joints, self.num_vertices
        if target_vertices.ndim != 3 or tuple(target_vertices.shape[1:]) != (V, 3):
            raise ValueError(f'target_vertices must have shape (batch, {V}, 3), got {tuple(target_vertices.shape)}')
        batch = target_vertices.shape[0]
        if target_joints is not None and tuple(target_joints.shape) != (batch, J, 3):
            raise ValueError(f'target_joints must have shape ({batch}, {J}, 3), got {tuple(target_joints.shape)}')
        if 'joint_error' in keys and target_joints is None:
            raise ValueError("'joint_error' needs target_joints")
        return batch

    def _recon_composed(self, keys, target_vertices, target_joints, **params):
        """The keys of the mesh-error step from ``forward`` and PyTorch arithmetic: the route of calls that carry
        gradients or are being traced (gradients flow through ``forward``'s backward)."""
        self._check_recon_targets(keys, target_vertices, target_joints)
        fw = self.forward(**params, return_vertices='vertices' in keys or 'vertex_error' in keys)
        out = {}
        if 'vertices' in keys:
            out['vertices'] = fw['vertices']
        if 'joints' in keys:
            out['joints'] = fw['joints']
        if 'vertex_error' in keys:
            out['vertex_error'] = torch.linalg.vector_norm(fw['vertices'] - target_vertices.to(fw['vertices'].device), dim=-1)
        if 'joint_error' in keys:
            out['joint_error'] = torch.linalg.vector_norm(fw['joints'] - target_joints.to(fw['joints'].device), dim=-1)
        return out

    def _recon_direct(self, keys, target_vertices, target_joints, pose_rotvecs=None, shape_betas=None, trans=None,
                      kid_factor=None, rel_rotmats=None, glob_rotmats=None):
        """The C-ABI call of the mesh-error step on its own (``smplfit_mesh_error_f32``): the keys of ``keys`` (of
        ``_lib.RECON_KEYS``) at the given forward inputs."""
        self._check_forward_inputs(pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats)
        batch = self._check_recon_targets(keys, target_vertices, target_joints)
        for name, arg in (('pose_rotvecs', pose_rotvecs), ('shape_betas', shape_betas), ('rel_rotmats', rel_rotmats),
                          ('glob_rotmats', glob_rotmats)):
            if arg is not None and arg.shape[0] != batch:
                raise ValueError(f'{name} has {arg.shape[0]} rows, target_vertices {batch}')
        if trans is not None and trans.shape[0] not in (1, batch):
            raise ValueError(f'trans has {trans.shape[0]} rows, target_vertices {batch}')
        device = self.v_template.device
        J, V = self.num_joints, self.num_vertices
        shapes = dict(vertices=(batch, V, 3), joints=(batch, J, 3), vertex_error=(batch, V), joint_error=(batch, J))
        out = {k: torch.empty(shapes[k], dtype=torch.float32, device=device) for k in _lib.RECON_KEYS if k in keys}
        if batch == 0 or not out:
            return out
        prep = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        pose, glob, rel, betas, nb, tr, kid = self._prep_forward_inputs(batch, pose_rotvecs, shape_betas, trans, kid_factor,
                                                                        rel_rotmats, glob_rotmats)
        tv, tj = prep(target_vertices), prep(target_joints)
        h = self._native(device, kid=kid is not None)
        ws = torch.empty(h.mesh_error_workspace_bytes(batch), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            args = _lib.MeshErrorArgs(
                pose_rotvecs=p(pose), glob_rotmats=p(glob), rel_rotmats=p(rel), shape_betas=p(betas),
                num_betas_given=nb, trans=p(tr), kid_factor=p(kid), batch=batch, target_vertices=p(tv),
                target_joints=p(tj), **{k: p(out.get(k)) for k in _lib.RECON_KEYS}, workspace=ws.data_ptr(),
                workspace_bytes=ws.numel(), hip_stream=stream)
            _lib.check(_lib.load().smplfit_mesh_error_f32(h.ptr, C.byref(args)))
        return out

    # -- rototranslate ---------------------------------------------------------------------------
    def rototranslate(
        self,
        R: torch.Tensor,
        t: Optional[torch.Tensor] = None,
        pose_rotvecs: Optional[torch.Tensor] = None,
        shape_betas: Optional[torch.Tensor] = None,
        trans: Optional[torch.Tensor] = None,
        kid_factor: Optional[torch.Tensor] = None,
        post_translate: bool = True,
    ) -> tuple[torch.Tensor, torch.Tensor]:
        """Rotates and translates the body in parametric form (pt/bodymodel.py:383-453): the parameters
        ``(new_pose_rotvecs, new_trans)`` with ``forward(new_pose_rotvecs, shape_betas, new_trans) = R @ forward(
        pose_rotvecs, shape_betas, trans) + t`` (``post_translate``) or ``R @ (forward(...) - t)`` (otherwise).  The root
        rotation acts about the pelvis of the shaped T-pose, so the translation carries ``(R - I) @ pelvis``.  One HIP
        launch (``smplfit_rototranslate_f32``).

        Unbatched, as the reference: ``R`` (3, 3), ``t`` (3,) or None, ``pose_rotvecs`` (3J,), ``shape_betas`` (n,) with
        ``n <= num_betas``, ``trans`` (3,), ``kid_factor`` (1,) or None; returns (3J,) and (3,).

        Batched (no counterpart in the reference): ``pose_rotvecs`` (B, 3J) and ``trans`` (B, 3) with ``R`` (3, 3) or
        (B, 3, 3), ``t`` None, (3,) or (B, 3), ``shape_betas`` (n,) or (B, n), ``kid_factor`` None, a scalar, (1,) or
        (B,); returns (B, 3J) and (B, 3).  ``B = 0`` returns empty tensors.

        Differentiable like ``forward``: with gradients enabled and a tensor input that requires grad, the backward is
        the HIP vector-Jacobian product (``smplfit_rototranslate_backward_f32``) with respect to all six inputs, once
        differentiable; an input shared across the batch gets the sum over the rows.  At a root rotation vector of
        exactly zero the gradient is the true derivative of the exponential map, not 0."""
        if pose_rotvecs is None or shape_betas is None or trans is None:
            raise ValueError('pose_rotvecs, shape_betas, and trans are required.')
        if torch.compiler.is_compiling():  # one opaque operator for torch.compile / export
            kid = kid_factor
            if kid is not None and not isinstance(kid, torch.Tensor):
                kid = torch.as_tensor(kid, dtype=torch.float32, device=self.v_template.device)
            p, tr = torch.ops.smplfitter_amd.rototranslate(
                self._model_id, R, t, pose_rotvecs, shape_betas, trans, kid, post_translate)
            return p, tr
        ins = (R, t, pose_rotvecs, shape_betas, trans, kid_factor)
        if torch.is_grad_enabled() and any(isinstance(a, torch.Tensor) and a.requires_grad for a in ins):
            return _RototranslateFn.apply(self, post_translate, *ins)
        return self._rototranslate_direct(*ins, post_translate)

    def _rigid_inputs(self, R, t, pose_rotvecs, shape_betas, trans, kid_factor):
        """The inputs of ``rototranslate`` checked and as detached contiguous fp32 tensors in the C-ABI's shapes:
        ``pose`` (B, 3J), ``trans`` (B, 3), ``R`` (B, 3, 3) or (3, 3), ``t`` (B, 3), (3,) or None, ``betas`` (B, n) and
        ``kid`` (B) or None (both expanded here when shared; ``R`` and ``t`` are shared inside the kernel)."""
        device = self.v_template.device
        J3 = 3 * self.num_joints
        named = dict(R=R, t=t, pose_rotvecs=pose_rotvecs, shape_betas=shape_betas, trans=trans, kid_factor=kid_factor)
        for name, a in named.items():
            if isinstance(a, np.ndarray):
                raise TypeError(f"Expected torch.Tensor for '{name}', got numpy.ndarray. "
                                f'Convert with torch.from_numpy() or torch.as_tensor().')
            if isinstance(a, torch.Tensor) and a.device.type != 'cuda':
                raise RuntimeError(_NO_CPU_PATH)
        if device.type != 'cuda':
            raise RuntimeError(_NO_CPU_PATH)
        prep = lambda a: a.detach().to(device=device, dtype=torch.float32)  # noqa: E731
        single = pose_rotvecs.ndim == 1
        bad = lambda name, a, want: ValueError(  # noqa: E731
            f"rototranslate: '{name}' must have shape {want}, got {tuple(a.shape)}")
        pose = prep(pose_rotvecs)
        if single:
            pose = pose[None]
        if pose.ndim != 2 or pose.shape[1] != J3:
            raise bad('pose_rotvecs', pose_rotvecs, f'({J3},) or (batch, {J3})')
        B = pose.shape[0]
        tr = prep(trans)
        if tuple(tr.shape) != ((3,) if single else (B, 3)):
            raise bad('trans', trans, '(3,)' if single else f'({B}, 3)')
        tr = tr.reshape(B, 3)
        Rm = prep(R)
        if tuple(Rm.shape) != (3, 3) and (single or tuple(Rm.shape) != (B, 3, 3)):
            raise bad('R', R, '(3, 3)' if single else f'(3, 3) or ({B}, 3, 3)')
        tt = None
        if t is not None:
            tt = prep(t)
            if tuple(tt.shape) != (3,) and (single or tuple(tt.shape) != (B, 3)):
                raise bad('t', t, '(3,)' if single else f'(3,) or ({B}, 3)')
        betas = prep(shape_betas)
        if betas.ndim == 2 and not single and betas.shape[0] == B:
            betas_shared = False
        elif betas.ndim == 1:
            betas_shared = True
            betas = betas[None].expand(B, betas.shape[0])
        else:
            raise bad('shape_betas', shape_betas, '(n,)' if single else f'(n,) or ({B}, n)')
        nb = betas.shape[1]
        if nb > self.num_betas:
            raise ValueError(f'rototranslate: {nb} shape_betas given to a model of {self.num_betas}')
        kid, kid_shared = None, False
        if kid_factor is not None:
            kid = torch.as_tensor(kid_factor, dtype=torch.float32, device=device).detach().reshape(-1)
            kid_shared = kid.numel() == 1
            if not kid_shared and (single or kid.numel() != B or kid_factor.ndim != 1):
                raise bad('kid_factor', kid_factor, '(1,)' if single else f'a scalar, (1,) or ({B},)')
            kid = kid.expand(B).contiguous()
        c = lambda a: None if a is None else a.contiguous()  # noqa: E731
        return dict(single=single, B=B, R=c(Rm), R_per=Rm.ndim == 3, t=c(tt), t_per=tt is not None and tt.ndim == 2,
                    pose=c(pose), betas=c(betas) if nb else None, nb=nb, betas_shared=betas_shared, trans=c(tr),
                    kid=kid, kid_shared=kid_shared)

    @staticmethod
    def _rigid_fields(x, stream):
        p = lambda a: None if a is None else a.data_ptr()  # noqa: E731
        return dict(R=p(x['R']), R_per_instance=int(x['R_per']), t=p(x['t']), t_per_instance=int(x['t_per']),
                    pose_rotvecs=p(x['pose']), shape_betas=p(x['betas']), num_betas_given=x['nb'], trans=p(x['trans']),
                    kid_factor=p(x['kid']), batch=x['B'], hip_stream=stream)

    def _rototranslate_direct(self, R, t, pose_rotvecs, shape_betas, trans, kid_factor, post_translate=True):
        """The C-ABI call behind ``rototranslate`` (and behind the ``smplfitter_amd::rototranslate`` operator)."""
        x = self._rigid_inputs(R, t, pose_rotvecs, shape_betas, trans, kid_factor)
        device = self.v_template.device
        B = x['B']
        new_pose = torch.empty((B, 3 * self.num_joints), dtype=torch.float32, device=device)
        new_trans = torch.empty((B, 3), dtype=torch.float32, device=device)
        if B:
            h = self._native(device, kid=x['kid'] is not None)
            with torch.cuda.device(device):
                stream = torch.cuda.current_stream(device).cuda_stream
                args = _lib.RototranslateArgs(
                    post_translate=int(bool(post_translate)), new_pose_rotvecs=new_pose.data_ptr(),
                    new_trans=new_trans.data_ptr(), **self._rigid_fields(x, stream))
                _lib.check(_lib.load().smplfit_rototranslate_f32(h.ptr, C.byref(args)))
        return (new_pose[0], new_trans[0]) if x['single'] else (new_pose, new_trans)

    def _rototranslate_backward_direct(self, R, t, pose_rotvecs, shape_betas, trans, kid_factor, post_translate,
                                       grad_pose=None, grad_trans=None):
        """The C-ABI call behind ``rototranslate``'s backward (``smplfit_rototranslate_backward_f32``): the gradients of
        the six inputs (None for one that is no tensor), each in the caller's shape and dtype; what was shared across
        the batch gets the sum of the per-row gradients (one ``sum(0)``: deterministic)."""
        ins = (R, t, pose_rotvecs, shape_betas, trans, kid_factor)
        x = self._rigid_inputs(*ins)
        device = self.v_template.device
        B, nb = x['B'], x['nb']
        out = [torch.zeros_like(a) if isinstance(a, torch.Tensor) else None for a in ins]
        if B == 0:
            return out
        g = lambda a, w: None if a is None else a.detach().to(device=device, dtype=torch.float32).reshape(B, w).contiguous()  # noqa: E731
        gp, gt_in = g(grad_pose, 3 * self.num_joints), g(grad_trans, 3)
        new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)  # noqa: E731
        g_R, g_pose, g_tr = new(B, 3, 3), new(B, 3 * self.num_joints), new(B, 3)
        g_t = new(B, 3) if isinstance(t, torch.Tensor) else None
        g_betas = new(B, nb) if nb else None
        g_kid = new(B) if isinstance(kid_factor, torch.Tensor) else None
        h = self._native(device, kid=x['kid'] is not None)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            p = lambda a: None if a is None else a.data_ptr()  # noqa: E731
            args = _lib.RototranslateBackwardArgs(
                post_translate=int(bool(post_translate)), grad_new_pose_rotvecs=p(gp), grad_new_trans=p(gt_in),
                grad_R=p(g_R), grad_t=p(g_t), grad_pose_rotvecs=p(g_pose), grad_shape_betas=p(g_betas),
                grad_trans=p(g_tr), grad_kid_factor=p(g_kid), **self._rigid_fields(x, stream))
            _lib.check(_lib.load().smplfit_rototranslate_backward_f32(h.ptr, C.byref(args)))
        give = lambda gr, a, shared: (gr.sum(0) if shared else gr).reshape(a.shape).to(a.dtype)  # noqa: E731
        out[0] = give(g_R, R, not x['R_per'])
        if g_t is not None:
            out[1] = give(g_t, t, not x['t_per'])
        out[2] = give(g_pose, pose_rotvecs, False)
        if g_betas is not None:
            out[3] = give(g_betas, shape_betas, x['betas_shared'])
        out[4] = give(g_tr, trans, False)
        if g_kid is not None:
            out[5] = give(g_kid, kid_factor, x['kid_shared'])
        return out


class _RototranslateFn(torch.autograd.Function):
    """``BodyModel.rototranslate`` under autograd: the forward is ``_rototranslate_direct`` (bit for bit the no-grad
    result), the backward ``_rototranslate_backward_direct`` on the current stream.  Only the inputs are saved."""

    @staticmethod
    def forward(ctx, model, post_translate, R, t, pose_rotvecs, shape_betas, trans, kid_factor):
        ins = (R, t, pose_rotvecs, shape_betas, trans, kid_factor)
        ctx.model, ctx.post_translate = model, post_translate
        ctx.set_materialize_grads(False)
        ctx.tensor_mask = [isinstance(a, torch.Tensor) for a in ins]
        ctx.others = [None if m else a for m, a in zip(ctx.tensor_mask, ins)]
        ctx.save_for_backward(*[a for a in ins if isinstance(a, torch.Tensor)])
        return model._rototranslate_direct(*ins, post_translate)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pose, g_trans):
        saved = iter(ctx.saved_tensors)
        ins = [next(saved) if m else o for m, o in zip(ctx.tensor_mask, ctx.others)]
        grads = ctx.model._rototranslate_backward_direct(*ins, ctx.post_translate, g_pose, g_trans)
        grads = [gr if isinstance(a, torch.Tensor) and a.requires_grad else None for gr, a in zip(grads, ins)]
        return (None, None, *grads)


class _ForwardFn(torch.autograd.Function):
    """``BodyModel.forward`` under autograd: the forward is ``_forward_direct`` (bit for bit the no-grad result), the
    backward ``_backward_direct`` on the current stream.  Only the inputs are saved."""

    @staticmethod
    def forward(ctx, model, return_vertices, pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats):
        ins = (pose_rotvecs, shape_betas, trans, kid_factor, rel_rotmats, glob_rotmats)
        ctx.model = model
        ctx.set_materialize_grads(False)  # an output the loss does not use: None, no zero-filled cotangent
        ctx.tensor_mask = [isinstance(a, torch.Tensor) for a in ins]
        ctx.others = [None if m else a for m, a in zip(ctx.tensor_mask, ins)]
        ctx.save_for_backward(*[a for a in ins if isinstance(a, torch.Tensor)])
        r = model._forward_direct(*ins, return_vertices)
        v = r['vertices'] if return_vertices else r['joints'].new_empty((0,))
        return r['joints'], r['orientations'], v

    @staticmethod
    @once_differentiable
    def backward(ctx, g_joints, g_orient, g_verts):
        saved = iter(ctx.saved_tensors)
        ins = [next(saved) if m else o for m, o in zip(ctx.tensor_mask, ctx.others)]
        grads = ctx.model._backward_direct(*ins, g_joints, g_orient, g_verts)
        grads = [gr if isinstance(a, torch.Tensor) and a.requires_grad else None for gr, a in zip(grads, ins)]
        return (None, None, *grads)
