"""``HandReplacer`` — same surface as ``smplfitter.pt.HandReplacer`` (reference src/smplfitter/pt/handreplacer.py):
replaces the hand vertices of SMPL-topology meshes with the hand pose of an SMPL-H pose vector — a vertex-weighted fit
of the SMPL-H model (hands down-weighted), the fitted pose's hand joints overwritten, the model evaluated again, and a
per-vertex blend ``out = in + (new - in) * hand_mix_weight[v]`` that leaves everything away from the hands as it was.

``replace_hand`` is ONE C-ABI call (``smplfit_replace_hands_f32``): the fit reads its weights as the (V) vector they
are, the hand joints are overwritten in the relative rotation matrices the forward's joint stage consumes, and the new
mesh is blended with the input where it is written — no (B, V) weight tensor and no (B, V, 3) intermediate.  Where the
fused call does not apply (``torch.compile``, a model or a switch that keeps the forward off the batch-major kernels) the
class composes the public ``BodyFitter.fit``, ``BodyModel.forward`` and the PyTorch blend, as the reference does.

The reference's quirk is kept: BOTH hands come from the source's RIGHT-hand block (``copy_hand_params``: left = right
mirrored, right unchanged).
"""

from __future__ import annotations

import ctypes as C
import os
import os.path as osp
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, modelio
from .bodyconverter import load_vertex_converter_csr
from .bodyfitter import BodyFitter
from .bodymodel import BodyModel

_HAND_START, _HAND_JOINTS = 22, 15  # SMPL-H: joints 22..36 left hand, 37..51 right hand


_N_HAND = _HAND_JOINTS * 3                      # values of one hand's block of a pose
_LEFT0 = _HAND_START * 3                        # first value of the left-hand block; the right-hand block follows it
_FIT_OPTIONS = dict(num_iter=3, beta_regularizer=0.0, final_adjust_rots=False)  # the fit of replace_hand


def _quintic_ramp(x: torch.Tensor, lo, hi) -> torch.Tensor:
    """0 below ``lo``, 1 above ``hi``, the quintic 6 t^5 - 15 t^4 + 10 t^3 of t = (x - lo) / (hi - lo) between (zero
    first and second derivative at both ends): the blend weight of a vertex as a function of its |x|."""
    t = ((x - lo) / (hi - lo)).clamp(0.0, 1.0)
    return t * t * t * (10.0 + t * (6.0 * t - 15.0))


def _dominated_rows(csr, columns) -> np.ndarray:
    """The rows of a sparse matrix that hold an entry above one half in one of ``columns``, ascending."""
    wanted = np.zeros(csr.shape[1], bool)
    wanted[np.asarray(columns, np.int64)] = True
    coo = csr.tocoo()
    return np.unique(coo.row[wanted[coo.col] & (coo.data > 0.5)]).astype(np.int64)


def load_pickle(path):
    """A pickle of plain containers and numpy arrays (``MANO_SMPLX_vertex_ids.pkl``) through the restricted unpickler."""
    with open(path, 'rb') as f:
        return modelio.restricted_load(f, encoding='latin1')


class HandReplacer(nn.Module):
    """Replaces the hand vertices of SMPL with the hand pose of SMPL-H (reference pt/handreplacer.py).

    ``hand_pose_source``: a flat SMPL-H pose of 52 * 3 values (the reference's only argument).  Keyword arguments, not in
    the reference: ``model_root`` — the directory of the ``smplh16`` model (default: the loader's search order);
    ``data_root`` — where ``body_models/smplx/MANO_SMPLX_vertex_ids.pkl`` and
    ``body_models/smplx2smpl_deftrafo_setup.pkl`` live (default ``$DATA_ROOT``, else ``.``); ``device``; ``num_betas``
    (default: every shape direction of the file — 16 for ``smplh16``).

    Deviation from the reference: the rest mesh behind ``hand_mix_weight`` is not taken from a forward pass at zero
    parameters (the reference's ``single()``) — the constructor needs no device —, but from the identity that pass
    reduces to, in fp32 on the host.  The two agree to a few ulps of a coordinate, ``hand_mix_weight`` to 1e-5; where it
    is exactly 0 or 1 it is so in both."""

    def __init__(self, hand_pose_source: torch.Tensor, *, model_root: Optional[str] = None,
                 data_root: Optional[str] = None, device=None, num_betas: Optional[int] = None):
        super().__init__()
        hand_pose_source = torch.as_tensor(hand_pose_source)
        n_pose = (_HAND_START + 2 * _HAND_JOINTS) * 3
        if hand_pose_source.ndim != 1 or hand_pose_source.shape[0] != n_pose:
            raise ValueError(f'hand_pose_source must be a flat SMPL-H pose of {n_pose} values, '
                             f'got shape {tuple(hand_pose_source.shape)}')
        root = osp.join(data_root if data_root is not None else os.getenv('DATA_ROOT', '.'), 'body_models')
        ids = load_pickle(osp.join(root, 'smplx', 'MANO_SMPLX_vertex_ids.pkl'))
        smplx2smpl = load_vertex_converter_csr(osp.join(root, 'smplx2smpl_deftrafo_setup.pkl'))
        # SMPL(-H) vertices that one SMPL-X hand vertex determines by more than half
        hand_rows = _dominated_rows(smplx2smpl, np.concatenate([np.asarray(ids[k]).reshape(-1) for k in ('left_hand', 'right_hand')]))

        self.smplh_bm = BodyModel('smplh16', 'neutral', model_root=model_root, num_betas=num_betas, device=device)
        self.smplh_fitter = BodyFitter(self.smplh_bm)
        bm = self.smplh_bm
        V = bm.num_vertices
        if smplx2smpl.shape[0] != V:
            raise ValueError(f'smplx2smpl_deftrafo_setup.pkl has {smplx2smpl.shape[0]} rows, the SMPL-H model {V} vertices')
        # |x| of the rest mesh in fp32 on the host (see the class docstring): with identity rotations every skinning
        # transform is the identity, so a posed template vertex is scaled by the sum of its skinning weights
        rest_feature = torch.eye(3).reshape(-1).repeat(bm.num_joints - 1)
        rest = (bm.v_template.cpu() + bm.posedirs.cpu() @ rest_feature) * bm.weights.cpu().sum(1, keepdim=True)
        abs_x = rest[:, 0].abs()
        self.hand_indices_all = torch.from_numpy(hand_rows)
        # the blend ramps up over the 10 cm in front of the innermost hand vertex
        inner = abs_x[self.hand_indices_all].min()
        self.hand_mix_weight = _quintic_ramp(abs_x, inner - 0.1, inner)
        self.hand_pose_source = hand_pose_source
        self.vertex_weights = torch.ones(1, V)
        self.vertex_weights[0, self.hand_indices_all] = 0.1
        self._plans = {}  # device index -> _lib.ReplaceHandsPlan, or None where the fused call does not apply

    # the native objects (ctypes handles) are per-process caches: a copy / pickle of the module starts without them
    def __getstate__(self):
        state = dict(self.__dict__)
        state['_plans'] = {}
        return state

    def __deepcopy__(self, memo):
        import copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == '_plans' else copy.deepcopy(v, memo)
        return new

    # -- the reference's helpers -------------------------------------------------------------------
    def mirror_rotvecs(self, hand_pose: torch.Tensor) -> torch.Tensor:
        """Flat rotation vectors mirrored across the x = 0 plane: the y and z components change sign."""
        out = hand_pose.reshape(-1, 3).clone()
        out[:, 1:] = -out[:, 1:]
        return out.reshape(-1)

    def copy_hand_params(self, smplh_pose: torch.Tensor) -> None:
        """Overwrite the hand joints of the SMPL-H poses ``smplh_pose`` (B, 156) in place, as the reference does: the
        left hand gets the source's RIGHT hand mirrored, the right hand the source's right hand."""
        right = self.hand_pose_source[_LEFT0 + _N_HAND:_LEFT0 + 2 * _N_HAND].to(device=smplh_pose.device, dtype=smplh_pose.dtype)
        smplh_pose[:, _LEFT0:_LEFT0 + 2 * _N_HAND] = torch.cat([self.mirror_rotvecs(right), right])

    def replacement_rotvecs(self) -> torch.Tensor:
        """The 30 * 3 values written over the joints 22..51 of every fitted pose."""
        pose = torch.zeros(1, _LEFT0 + 2 * _N_HAND, dtype=torch.float32)
        self.copy_hand_params(pose)
        return pose[0, _LEFT0:]

    # -- native plan -------------------------------------------------------------------------------
    def _plan(self, device: torch.device) -> Optional[_lib.ReplaceHandsPlan]:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in self._plans:
            try:
                with torch.cuda.device(idx):
                    self._plans[idx] = _lib.ReplaceHandsPlan(
                        self.smplh_bm._native(device), self.vertex_weights[0].numpy(), self.hand_mix_weight.numpy(),
                        _HAND_START, 2 * _HAND_JOINTS, self.replacement_rotvecs().numpy())
            except NotImplementedError:  # a model whose forward is outside the batch-major kernels
                self._plans[idx] = None
        return self._plans[idx]

    # -- API ---------------------------------------------------------------------------------------
    def replace_hand(self, smpl_verts: torch.Tensor) -> torch.Tensor:
        """(B, 6890, 3) -> (B, 6890, 3): the reference's ``replace_hand``.  Inputs that require gradients raise
        ``NotImplementedError``; an empty batch returns an empty result."""
        return self.replace_hand_with_params(smpl_verts)['vertices']

    def replace_hand_with_params(self, smpl_verts: torch.Tensor) -> dict[str, torch.Tensor]:
        """``replace_hand`` together with the parameters of the mesh that was blended in (not in the reference):
        ``vertices`` (B, V, 3), and ``pose_rotvecs`` (B, 156), ``shape_betas`` (B, S), ``trans`` (B, 3) — the fitted
        SMPL-H parameters with the hand joints overwritten, so that
        ``in + (smplh_bm(pose_rotvecs, shape_betas, trans)['vertices'] - in) * hand_mix_weight[:, None]`` is
        ``vertices``."""
        bm = self.smplh_bm
        V = bm.num_vertices
        if smpl_verts.ndim != 3 or tuple(smpl_verts.shape[1:]) != (V, 3):
            raise ValueError(f'smpl_verts must have shape (batch, {V}, 3), got {tuple(smpl_verts.shape)}')
        if smpl_verts.requires_grad:
            raise NotImplementedError('the HIP hand replacement is not differentiable; detach the input')
        device = bm.v_template.device
        if smpl_verts.shape[0] == 0:
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)  # noqa: E731
            return dict(vertices=new(0, V, 3), pose_rotvecs=new(0, bm.num_joints * 3),
                        shape_betas=new(0, self.smplh_fitter.n_betas), trans=new(0, 3))
        res = self._replace_fused(smpl_verts)
        if res is None:
            res = self._replace_unfused(smpl_verts)
        return res

    def _replace_unfused(self, smpl_verts):
        """The reference's sequence of calls: weighted fit, hand joints overwritten, forward, blend."""
        device = self.smplh_bm.v_template.device
        v = smpl_verts.to(device=device, dtype=torch.float32)
        weights = self.vertex_weights.to(device).expand(v.shape[0], -1).contiguous()
        fit = self.smplh_fitter.fit(v, vertex_weights=weights, requested_keys=['pose_rotvecs', 'shape_betas'], **_FIT_OPTIONS)
        pose = fit['pose_rotvecs'].clone()
        self.copy_hand_params(pose)
        posed = self.smplh_bm(pose, fit['shape_betas'], fit['trans'])['vertices']
        out = v + (posed - v) * self.hand_mix_weight.to(device).unsqueeze(1)
        return dict(vertices=out, pose_rotvecs=pose, shape_betas=fit['shape_betas'], trans=fit['trans'])

    def _replace_fused(self, smpl_verts):
        """``smplfit_replace_hands_f32``; None when the fused path does not apply (tracing, a model or a tuning switch
        that keeps the forward off the batch-major kernels)."""
        bm = self.smplh_bm
        device = bm.v_template.device
        if torch.compiler.is_compiling() or device.type != 'cuda':
            return None
        plan = self._plan(device)
        if plan is None:
            return None
        B, J, V, S = smpl_verts.shape[0], bm.num_joints, bm.num_vertices, self.smplh_fitter.n_betas
        v = smpl_verts.to(device=device, dtype=torch.float32).contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)  # noqa: E731
        out = dict(vertices=new(B, V, 3), pose_rotvecs=new(B, 3 * J), shape_betas=new(B, S), trans=new(B, 3))
        ws = torch.empty(plan.workspace_bytes(B), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            args = _lib.ReplaceHandsArgs(
                vertices=v.data_ptr(), batch=B, num_iter=_FIT_OPTIONS['num_iter'],
                beta_regularizer=_FIT_OPTIONS['beta_regularizer'], beta_regularizer2=0.0,
                final_adjust_rots=int(_FIT_OPTIONS['final_adjust_rots']), out_vertices=out['vertices'].data_ptr(),
                out_pose_rotvecs=out['pose_rotvecs'].data_ptr(), out_shape_betas=out['shape_betas'].data_ptr(),
                out_trans=out['trans'].data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                hip_stream=torch.cuda.current_stream(device).cuda_stream)
            try:
                _lib.check(_lib.load().smplfit_replace_hands_f32(plan.ptr, C.byref(args)))
            except NotImplementedError:
                # the plan was made while the batch-major kernels applied; the tuning options have been reloaded since
                # (SMPLFIT_BM=0): THIS call takes fit + forward + blend.  The plan is kept
                return None
        return out
