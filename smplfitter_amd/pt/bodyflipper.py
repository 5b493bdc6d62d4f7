"""``BodyFlipper`` — same surface as ``smplfitter.pt.BodyFlipper`` (reference src/smplfitter/pt/bodyflipper.py):
mirrors body parameters along the x axis (left/right flip augmentation) by evaluating the model, mirroring the mesh
with a sparse (V x V) matrix followed by x -> -x, and fitting the model again — with the kid blend shape enabled,
warm-started from the naively flipped pose and the input betas.

Everything runs in the HIP kernels.  The default ``flip`` branch is ONE C-ABI call (``smplfit_flip_f32``): the
forward of the input parameters (with ``kid_factor``), the mirror transfer, the naive flip of the pose and the
warm-started fit hand their data to each other in the kernels' instance-innermost streams, so no ``(B, V, 3)`` mesh
is written.  ``flip_vertices`` on its own is ``smplfit_transfer_f32`` on the negating transfer.
"""

from __future__ import annotations

import ctypes as C
import os
import os.path as osp
from typing import Optional

import numpy as np
import scipy.optimize
import scipy.sparse as sp
import scipy.spatial.distance
import torch
import torch.nn as nn

from .. import _lib
from .bodyconverter import load_vertex_converter_csr
from .bodyfitter import BodyFitter
from .bodymodel import BodyModel

_SMPL_V, _SMPLX_V = 6890, 10475


def load_mirror_csr(path):
    """The SMPL-X mirror matrix of ``smplx_flip_correspondences.npz``: row v holds the barycentric weights ``bc[v]`` of
    the three vertices ``closest_faces[v]`` around the mirror image of vertex v."""
    m = np.load(path)
    cols, w = np.asarray(m['closest_faces']), np.asarray(m['bc'])
    n = w.shape[0]
    rows = np.repeat(np.arange(cols.shape[0]), cols.shape[1])
    return sp.coo_matrix((w.reshape(-1), (rows, cols.reshape(-1))), shape=(cols.shape[0], n)).tocsr().astype(np.float32)


def mirror_csr_for(num_vertices: int):
    """The (V x V) mirror matrix of a model with ``num_vertices`` vertices, in sorted CSR form, read from
    ``$DATA_ROOT/body_models``: SMPL-X from its correspondence file, SMPL as smplx2smpl @ mirror_smplx @ smpl2smplx."""
    if num_vertices not in (_SMPL_V, _SMPLX_V):
        raise ValueError(f'Unsupported number of vertices: {num_vertices}')
    root = osp.join(os.getenv('DATA_ROOT', '.'), 'body_models')
    m = load_mirror_csr(osp.join(root, 'smplx', 'smplx_flip_correspondences.npz'))
    if num_vertices == _SMPL_V:
        s2x = load_vertex_converter_csr(osp.join(root, 'smpl2smplx_deftrafo_setup.pkl'))
        x2s = load_vertex_converter_csr(osp.join(root, 'smplx2smpl_deftrafo_setup.pkl'))
        m = (x2s @ m @ s2x).tocsr()
    m.sort_indices()
    return m


def mirror_mapping(points) -> np.ndarray:
    """For every point the index of the point nearest to its x-mirrored image, as a one-to-one assignment
    (minimum total distance)."""
    p = np.asarray(points, np.float64)
    rows, cols = scipy.optimize.linear_sum_assignment(scipy.spatial.distance.cdist(p, p * [-1.0, 1.0, 1.0]))
    return cols[np.argsort(rows)]


class BodyFlipper(nn.Module):
    """Mirrors body model parameters along the x axis (reference pt/bodyflipper.py).

    Deviation from the reference: ``mirror_inds`` (the vertex mirror map, which ``flip`` never uses) is computed on
    first access instead of in the constructor — its assignment over all vertices takes seconds and a V x V distance
    matrix (about 0.9 GB for SMPL-X).  Its values are the reference's."""

    def __init__(self, body_model: BodyModel):
        super().__init__()
        self.body_model = body_model
        self.fitter = BodyFitter(body_model, enable_kid=True)
        device = body_model.v_template.device
        # the reference keeps a torch sparse-CSR buffer; here the matrix lives in the native library (one device copy
        # per GPU, made on first use) and ``mirror_csr`` is its host (scipy) form
        self.mirror_csr = mirror_csr_for(body_model.num_vertices)
        self.mirror_inds_joints = nn.Buffer(torch.tensor(
            mirror_mapping(body_model.J_template.cpu().numpy()), dtype=torch.int, device=device))
        self._mirror_inds = None
        self._transfers = {}  # device index -> _lib.Transfer (the negating mirror)
        self._plans = {}      # device index -> _lib.FlipPlan, or None where the fused call does not apply

    @property
    def mirror_inds(self) -> torch.Tensor:
        """Vertex mirror map (computed on first access, see the class docstring)."""
        if self._mirror_inds is None:
            # the rest mesh = the forward at zero parameters: the pose feature is the flattened relative rotations
            # (identities), every skinning transform the identity, so each posed template vertex is scaled by the sum
            # of its weights (one for the official models)
            bm = self.body_model
            feat = np.tile(np.eye(3).reshape(-1), bm.num_joints - 1)
            v_posed = bm.v_template.cpu().double().numpy() + bm.posedirs.cpu().double().numpy() @ feat
            rest = v_posed * bm.weights.cpu().double().numpy().sum(1, keepdims=True)
            self._mirror_inds = torch.tensor(mirror_mapping(rest), dtype=torch.int)
        return self._mirror_inds.to(self.body_model.v_template.device)

    # the native objects (ctypes handles) are per-process caches: a copy / pickle of the module starts without them
    def __getstate__(self):
        state = dict(self.__dict__)
        state['_transfers'], state['_plans'] = {}, {}
        return state

    def __deepcopy__(self, memo):
        import copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k in ('_transfers', '_plans') else copy.deepcopy(v, memo)
        return new

    # -- native objects ----------------------------------------------------------------------------
    def _transfer(self, device: torch.device) -> _lib.Transfer:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        t = self._transfers.get(idx)
        if t is None:
            m = self.mirror_csr
            with torch.cuda.device(idx):
                t = _lib.Transfer(m.shape[1], m.shape[0], m.indptr, m.indices, m.data, negate_x=True)
            self._transfers[idx] = t
        return t

    def _plan(self, device: torch.device) -> Optional[_lib.FlipPlan]:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in self._plans:
            try:
                with torch.cuda.device(idx):
                    self._plans[idx] = _lib.FlipPlan(self.body_model._native(device, kid=True), self._transfer(device),
                                                     self.mirror_inds_joints.cpu().numpy())
            except NotImplementedError:  # a model outside the batch-major kernels: forward + flip_vertices + fit
                self._plans[idx] = None
        return self._plans[idx]

    # -- API -----------------------------------------------------------------------------------------
    def flip(
        self,
        pose_rotvecs: torch.Tensor,
        shape_betas: torch.Tensor,
        trans: torch.Tensor,
        kid_factor: Optional[torch.Tensor] = None,
        num_iter: int = 1,
    ) -> dict[str, torch.Tensor]:
        """Same arguments / results as the reference's ``flip``: the parameters of the x-mirrored body —
        ``pose_rotvecs``, ``shape_betas``, ``trans`` and ``kid_factor`` (always a tensor: the fit has the kid
        unknown; near 0 when no ``kid_factor`` is given).  Inputs that require gradients raise
        ``NotImplementedError``."""
        if any(isinstance(t, torch.Tensor) and t.requires_grad for t in (pose_rotvecs, shape_betas, trans, kid_factor)):
            raise NotImplementedError('the HIP flip is not differentiable; detach the inputs')
        kid_reg = 1e9 if kid_factor is None else 0.0
        fit = self._flip_fused(pose_rotvecs, shape_betas, trans, kid_factor, num_iter, kid_reg)
        if fit is None:
            fit = self._flip_unfused(pose_rotvecs, shape_betas, trans, kid_factor, num_iter)
        return dict(pose_rotvecs=fit['pose_rotvecs'], shape_betas=fit['shape_betas'], trans=fit['trans'],
                    kid_factor=fit['kid_factor'])

    def _flip_unfused(self, pose_rotvecs, shape_betas, trans, kid_factor, num_iter):
        """The reference's sequence of calls: forward (with kid_factor), flip_vertices, warm-started fit."""
        inp = self.body_model(pose_rotvecs, shape_betas, trans, kid_factor=kid_factor)
        return self.fitter.fit(
            target_vertices=self.flip_vertices(inp['vertices']), num_iter=num_iter, beta_regularizer=1e-2,
            beta_regularizer2=1e-2, final_adjust_rots=True, kid_regularizer=1e9 if kid_factor is None else 0.0,
            initial_pose_rotvecs=self.naive_flip_rotvecs(pose_rotvecs), initial_shape_betas=shape_betas,
            requested_keys=['pose_rotvecs', 'shape_betas'])

    def _flip_fused(self, pose_rotvecs, shape_betas, trans, kid_factor, num_iter, kid_reg):
        """``smplfit_flip_f32``: forward + mirror + naive flip + warm-started fit in one call; None when the fused
        path does not apply (models outside the batch-major kernels, SMPLFIT_BM=0, tracing, empty batch)."""
        bm = self.body_model
        device = bm.v_template.device
        if torch.compiler.is_compiling() or device.type != 'cuda' or pose_rotvecs.shape[0] == 0:
            return None
        plan = self._plan(device)
        if plan is None:
            return None
        B, J, S = pose_rotvecs.shape[0], bm.num_joints, self.fitter.n_betas
        prep = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        pose = prep(pose_rotvecs.reshape(B, J * 3))
        betas = prep(shape_betas)
        nb = 0
        if betas is not None:
            nb = min(betas.shape[1], bm.num_betas)
            betas = betas[:, :nb].contiguous() if nb > 0 else None
        tr = prep(trans)
        if tr is not None and tr.shape[0] != B:
            tr = tr.expand(B, 3).contiguous()
        kid = None
        if kid_factor is not None:
            kid = torch.as_tensor(kid_factor, dtype=torch.float32, device=device).reshape(-1)
            kid = kid.expand(B).contiguous() if kid.numel() == 1 else kid.contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)  # noqa: E731
        out = dict(pose_rotvecs=new(B, 3 * J), shape_betas=new(B, S), trans=new(B, 3), kid_factor=new(B))
        ws = torch.empty(plan.workspace_bytes(B), dtype=torch.uint8, device=device)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(device):
            args = _lib.FlipArgs(
                pose_rotvecs=p(pose), shape_betas=p(betas), num_betas_given=nb, trans=p(tr), kid_factor=p(kid),
                batch=B, num_iter=int(num_iter), beta_regularizer=1e-2, beta_regularizer2=1e-2,
                kid_regularizer=float(kid_reg), final_adjust_rots=1, out_pose_rotvecs=p(out['pose_rotvecs']),
                out_shape_betas=p(out['shape_betas']), out_trans=p(out['trans']),
                out_kid_factor=p(out['kid_factor']), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                hip_stream=torch.cuda.current_stream(device).cuda_stream)
            try:
                _lib.check(_lib.load().smplfit_flip_f32(plan.ptr, C.byref(args)))
            except NotImplementedError:
                # the plan was made while the batch-major kernels applied; the tuning options have been reloaded since
                # (SMPLFIT_BM=0): THIS call takes the forward + flip_vertices + fit calls.  The plan is kept
                return None
        return out

    def flip_vertices(self, inp_vertices: torch.Tensor) -> torch.Tensor:
        """Mirrored vertices (reference ``flip_vertices``): ``(mirror_csr @ v) * [-1, 1, 1]``, (B, V, 3) -> (B, V, 3),
        ``smplfit_transfer_f32`` on the negating transfer."""
        V = self.body_model.num_vertices
        if inp_vertices.ndim != 3 or tuple(inp_vertices.shape[1:]) != (V, 3):
            raise ValueError(f'inp_vertices must have shape (batch, {V}, 3), got {tuple(inp_vertices.shape)}')
        if inp_vertices.requires_grad:
            raise NotImplementedError('the HIP transfer kernel is not differentiable; detach the input')
        device = self.body_model.v_template.device
        v = inp_vertices.to(device=device, dtype=torch.float32).contiguous()
        out = torch.empty_like(v)
        if v.shape[0] > 0:
            t = self._transfer(device)
            with torch.cuda.device(device):
                _lib.check(_lib.load().smplfit_transfer_f32(
                    t.ptr, C.c_void_p(v.data_ptr()), v.shape[0], C.c_void_p(out.data_ptr()),
                    C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
        return out

    def naive_flip_rotvecs(self, pose_rotvecs: torch.Tensor) -> torch.Tensor:
        """The joints' rotation vectors reordered by ``mirror_inds_joints`` and multiplied by (1, -1, -1), without
        regard to the model's slight asymmetry (reference ``naive_flip_rotvecs``)."""
        J = self.body_model.num_joints
        sign = torch.tensor([1.0, -1.0, -1.0], dtype=pose_rotvecs.dtype, device=pose_rotvecs.device)
        r = pose_rotvecs.reshape(-1, J, 3)[:, self.mirror_inds_joints.to(pose_rotvecs.device).long()] * sign
        return r.reshape(-1, J * 3)
