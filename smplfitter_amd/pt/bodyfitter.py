"""``BodyFitter`` — same surface as ``smplfitter.pt.BodyFitter`` (reference
src/smplfitter/pt/bodyfitter.py:15-549); ``fit`` in its default configuration runs entirely in the HIP
kernels behind ``smplfit_fit_f32``, and its gradients with respect to the targets and weights in those behind
``smplfit_fit_backward_f32``.  Options the kernels do not implement raise
``NotImplementedError`` — they never silently compute something else.
"""

from __future__ import annotations

import collections
import ctypes as C
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .bodymodel import BodyModel, _ptr


def _share_callback(ws: torch.Tensor, group):
    """``smplfit_share_allreduce_fn`` for a ``share_beta`` batch sharded over ``group`` (a null callback
    without one) and the list an exception raised inside it is parked in.  ``sums`` lies inside the
    workspace tensor ``ws``; the collective is ordered after the kernels already enqueued on the current
    stream (nccl = RCCL) or synchronous (gloo)."""
    failure: list = []
    if group is None:
        return _lib.ShareAllreduceFn(), failure

    def allreduce_sums(_user, sums_ptr, count, _stream):
        try:
            import torch.distributed as dist
            off = sums_ptr - ws.data_ptr()
            sums = ws.view(torch.uint8).reshape(-1)[off:off + 8 * count].view(torch.float64)
            if dist.get_backend(group) == 'gloo':  # host collective: stage explicitly
                staged = sums.cpu()
                dist.all_reduce(staged, op=dist.ReduceOp.SUM, group=group)
                sums.copy_(staged)
            else:
                dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
            return 0
        except BaseException as e:  # never unwind through the C frames
            failure.append(e)
            return 1

    return _lib.ShareAllreduceFn(allreduce_sums), failure


def _segment_sizes(segments, batch: int) -> tuple:
    """``share_beta_segments`` as a tuple of ints, checked on the host: positive sizes that sum to the batch."""
    if isinstance(segments, torch.Tensor):
        if segments.device.type != 'cpu' or segments.is_floating_point() or segments.is_complex() or segments.dtype == torch.bool:
            raise ValueError('share_beta_segments must be a sequence of ints or a CPU integer tensor')
        segments = segments.reshape(-1).tolist()
    sizes = tuple(int(n) for n in segments)
    if any(n < 1 for n in sizes):
        raise ValueError(f'share_beta_segments: every segment needs at least one row, got {list(sizes)}')
    if sum(sizes) != batch:
        raise ValueError(f'share_beta_segments sum to {sum(sizes)}, the batch has {batch} rows')
    return sizes


def _recon_keys(requested_keys, target_joints, **scale_options) -> tuple:
    """The keys of the mesh-error step among ``requested_keys`` (``vertices, joints, vertex_error, joint_error``:
    DESIGN.md §22), checked on the host: ``joint_error`` needs target joints, and no key is served with a scale option
    (which target the errors of a scaled fit refer to is undecided)."""
    recon = tuple(k for k in _lib.RECON_KEYS if k in requested_keys)
    if recon:
        if 'joint_error' in recon and target_joints is None:
            raise ValueError("requested_keys: 'joint_error' needs target_joints")
        bad = [k for k, v in scale_options.items() if v]
        if bad:
            raise NotImplementedError(f'requested_keys {list(recon)} are not served together with {", ".join(bad)}')
    return recon


class BodyFitter(nn.Module):
    """Fits SMPL-family parameters (pose, shape, translation) to target vertices (and joints).

    Parameters:
        body_model: the :class:`BodyModel` to fit.
        enable_kid: adds the kid blend shape (AGORA) as one more shape unknown
            (reference pt/bodyfitter.py:52-58); results then carry ``kid_factor``.
        native_backward: the gradients of :meth:`fit` come from the HIP adjoint (``smplfit_fit_backward_f32``);
            ``False`` keeps the PyTorch restatement (pt/_autograd.py), which also serves more than 17 shape unknowns.
    """

    def __init__(self, body_model: BodyModel, enable_kid: bool = False, native_backward: bool = True):
        super().__init__()
        self.native_backward = native_backward
        self.body_model = body_model
        self.n_betas = body_model.shapedirs.shape[2]
        self.enable_kid = enable_kid
        self._torchfit = None  # tables of the differentiable restatement (pt/_autograd.py), built on first use
        self._torchfit64 = None  # the same in fp64 (fit_with_known_shape's PyTorch route)
        self.is_smpl_family = body_model.model_name.startswith('smpl')
        # (device index, segment sizes) -> _lib.ShareSegments, least recently used first; bounded: the track layout of
        # a caller changes from call to call
        self._segment_plans = collections.OrderedDict()

    MAX_SEGMENT_PLANS = 16

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_segment_plans'] = collections.OrderedDict()
        return state

    def __deepcopy__(self, memo):
        import copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = collections.OrderedDict() if k == '_segment_plans' else copy.deepcopy(v, memo)
        return new

    def _segment_plan(self, device: torch.device, sizes: tuple) -> _lib.ShareSegments:
        """The native tables of a layout of segments on ``device`` (``smplfit_share_segments_create``), cached."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, sizes)
        plan = self._segment_plans.pop(key, None)
        if plan is None:
            with torch.cuda.device(device):
                plan = _lib.ShareSegments(sizes)
            while len(self._segment_plans) >= self.MAX_SEGMENT_PLANS:
                # (its device tables go with the last reference: hipFree waits for the work that reads them)
                self._segment_plans.popitem(last=False)
        self._segment_plans[key] = plan
        return plan

    def fit(
        self,
        target_vertices: torch.Tensor,
        target_joints: Optional[torch.Tensor] = None,
        vertex_weights: Optional[torch.Tensor] = None,
        joint_weights: Optional[torch.Tensor] = None,
        num_iter: int = 1,
        beta_regularizer: float = 1,
        beta_regularizer2: float = 0,
        scale_regularizer: float = 0,
        kid_regularizer: Optional[float] = None,
        share_beta: bool = False,
        final_adjust_rots: bool = True,
        scale_target: bool = False,
        scale_fit: bool = False,
        initial_pose_rotvecs: Optional[torch.Tensor] = None,
        initial_shape_betas: Optional[torch.Tensor] = None,
        initial_kid_factor: Optional[torch.Tensor] = None,
        requested_keys: Optional[list[str]] = None,
        _workspace: Optional[torch.Tensor] = None,
        share_beta_group=None,
        share_beta_segments=None,
    ) -> dict[str, torch.Tensor]:
        """Same arguments and returned keys as the reference's ``fit`` (pt/bodyfitter.py:283-549):
        ``shape_betas, trans, orientations, relative_orientations`` and ``pose_rotvecs`` when
        requested (default).  ``initial_pose_rotvecs / initial_shape_betas / initial_kid_factor``
        warm-start the fit (``smplfit_fit_warm_f32``; reference :363-382).

        ``share_beta_group`` (not in the reference): a ``torch.distributed`` process group over which
        a ``share_beta`` batch is sharded, one block of instances per rank — the summed normal
        equations of every shape solve are all-reduced over it, so all ranks get the shape of the
        WHOLE batch (``smplfitter_amd.dist.fit_sharded`` passes it).

        ``share_beta_segments`` (not in the reference): the sizes of consecutive runs of rows — a sequence of ints or
        a CPU integer tensor, positive, summing to the batch — for many tracks in one call: every run gets one shape
        (and one kid factor), and its rows are bit for bit those of ``fit(rows of the run, share_beta=True)`` with the
        same options (to the bit while the batch and the run take the same cell tables — both up to 768
        rows or both above —, to rounding otherwise).  Implies ``share_beta``; not with ``share_beta_group``, gradients or
        ``torch.compile``.

        ``requested_keys`` also understands ``'vertices'``, ``'joints'``, ``'vertex_error'`` and ``'joint_error'`` (not
        in the reference): the model posed at the fitted parameters — the bits of ``BodyModel.forward(
        glob_rotmats=orientations, shape_betas, trans, kid_factor)`` — and the unweighted Euclidean distance of every
        vertex / joint to its target, from the same call (``smplfit_fit_recon_f32``): the fit's results keep their bits.
        ``'joint_error'`` needs ``target_joints`` (``ValueError``); none of them is served with ``scale_target`` /
        ``scale_fit`` (``NotImplementedError``).  A caller ``_workspace`` then has the size of
        ``Handle.fit_recon_workspace_bytes``.  With gradients or under ``torch.compile`` the keys come from
        ``BodyModel.forward`` and PyTorch arithmetic on the results."""
        if requested_keys is None:
            requested_keys = ['pose_rotvecs']
        segments = None
        if share_beta_segments is not None:
            if share_beta_group is not None:
                raise ValueError('share_beta_segments cannot be combined with share_beta_group')
            segments = _segment_sizes(share_beta_segments, target_vertices.shape[0])
            if torch.compiler.is_compiling():
                raise NotImplementedError('share_beta_segments cannot be traced (the smplfitter_amd::fit operator has no '
                                          'argument for them); call the fit outside the compiled region')
            share_beta = True
        if scale_target and scale_fit:  # same check, same message as pt/bodyfitter.py:858-859
            raise ValueError('Only one of estim_scale_target and estim_scale_fit can be True')
        scale_mode = 1 if scale_target else 2 if scale_fit else 0
        recon = _recon_keys(requested_keys, target_joints, scale_target=scale_target, scale_fit=scale_fit)
        if share_beta_group is not None:
            if not share_beta:
                raise ValueError('share_beta_group needs share_beta=True')
            if torch.compiler.is_compiling():
                raise NotImplementedError('a sharded share_beta fit cannot be traced (collective inside the fit)')
        if initial_kid_factor is not None and not self.enable_kid:
            raise NotImplementedError(
                'initial_kid_factor needs BodyFitter(enable_kid=True) on the HIP path')
        # the reference defaults the kid ridge weight to beta_regularizer (pt/bodyfitter.py:1235-1237)
        kid_reg = float(beta_regularizer if kid_regularizer is None else kid_regularizer)
        if torch.is_grad_enabled() and not torch.compiler.is_compiling() and any(
                t is not None and t.requires_grad for t in (target_vertices, target_joints, vertex_weights, joint_weights)):
            # gradients with respect to the targets / weights (reference: tests/pt/test_fitter_grad.py): the forward is
            # the HIP fit under an autograd Function whose backward is one native call (smplfit_fit_backward_f32,
            # DESIGN.md §17); more than 17 shape unknowns, or native_backward=False, run the algorithm written with
            # PyTorch operators (pt/_autograd.py) on the model's cuda device instead
            unsupported = dict(share_beta=share_beta, scale_target=scale_target, scale_fit=scale_fit,
                               initial_pose_rotvecs=initial_pose_rotvecs, initial_shape_betas=initial_shape_betas,
                               initial_kid_factor=initial_kid_factor)
            if self.native_backward and self.n_betas + int(self.enable_kid) <= 17:
                bad = [k for k, v in unsupported.items() if v is not None and v is not False]
                if bad:
                    raise NotImplementedError(f'the differentiable fit does not implement {", ".join(bad)}; detach the inputs to use the HIP path')
                opts = (int(num_iter), float(beta_regularizer), float(beta_regularizer2), kid_reg, bool(final_adjust_rots))
                res = _FitFn.apply(self, opts, _workspace, target_vertices, target_joints, vertex_weights, joint_weights)
                result = dict(pose_rotvecs=res[0], shape_betas=res[1], trans=res[2], orientations=res[3],
                              relative_orientations=res[4])
                if self.enable_kid:
                    result['kid_factor'] = res[5]
            else:
                result = self._fit_differentiable(
                    target_vertices, target_joints, vertex_weights, joint_weights, num_iter, beta_regularizer,
                    beta_regularizer2, kid_regularizer, final_adjust_rots, unsupported=unsupported)
            result.update(self._recon_after(recon, True, target_vertices, target_joints, result))
        elif torch.compiler.is_compiling():  # one opaque operator for torch.compile / export
            pose, betas, trans, kid, orient, rel, scale = torch.ops.smplfitter_amd.fit(
                self.body_model._model_id, self.enable_kid, target_vertices, target_joints,
                vertex_weights, joint_weights, int(num_iter), float(beta_regularizer),
                float(beta_regularizer2), kid_reg, bool(final_adjust_rots), initial_pose_rotvecs,
                initial_shape_betas, initial_kid_factor, bool(share_beta), scale_mode,
                float(scale_regularizer))
            result = dict(pose_rotvecs=pose, shape_betas=betas, trans=trans, orientations=orient,
                          relative_orientations=rel)
            if self.enable_kid:
                result['kid_factor'] = kid
            if scale_mode:
                result['scale_corr'] = scale
            result.update(self._recon_after(recon, True, target_vertices, target_joints, result))
        else:
            result = self._fit_direct(target_vertices, target_joints, vertex_weights, joint_weights,
                                      num_iter, beta_regularizer, beta_regularizer2, kid_reg,
                                      final_adjust_rots, initial_pose_rotvecs, initial_shape_betas,
                                      initial_kid_factor, _workspace, share_beta, scale_mode,
                                      scale_regularizer, share_beta_group, segments, recon)
        # relative_orientations = parent^T @ global of the FINAL rotations (pt/bodyfitter.py:523-533);
        # returned always (the reference returns the pre-refinement ones when neither
        # 'relative_orientations' nor 'pose_rotvecs' is requested)
        if 'pose_rotvecs' not in requested_keys:
            result.pop('pose_rotvecs', None)
        return result

    def _fit_differentiable(self, target_vertices, target_joints, vertex_weights, joint_weights, num_iter,
                            beta_regularizer, beta_regularizer2, kid_regularizer, final_adjust_rots, unsupported):
        bm = self.body_model
        device = bm.v_template.device
        if device.type != 'cuda':
            raise RuntimeError("smplfitter_amd runs on MI355X only: move the model and the inputs to a 'cuda' (ROCm) device")
        bad = [k for k, v in unsupported.items() if v is not None and v is not False]
        if bad:
            raise NotImplementedError(f'the differentiable fit does not implement {", ".join(bad)}; detach the inputs to use the HIP path')
        self._torchfit_route(stacklevel=4)
        mv = lambda t: None if t is None else t.to(device)  # noqa: E731
        return self._torchfit.fit(mv(target_vertices), mv(target_joints), mv(vertex_weights), mv(joint_weights),
                                  num_iter=int(num_iter), beta_regularizer=float(beta_regularizer),
                                  beta_regularizer2=float(beta_regularizer2), kid_regularizer=kid_regularizer,
                                  final_adjust_rots=bool(final_adjust_rots))

    def _fit_direct(self, target_vertices, target_joints, vertex_weights, joint_weights, num_iter,
                    beta_regularizer, beta_regularizer2, kid_reg, final_adjust_rots,
                    initial_pose_rotvecs, initial_shape_betas, initial_kid_factor, _workspace,
                    share_beta=False, scale_mode=0, scale_regularizer=0.0, share_beta_group=None, segments=None, recon=()):
        """The C-ABI call behind ``fit`` (and behind the ``smplfitter_amd::fit`` operator): every result
        tensor, ``pose_rotvecs`` included.  ``segments``: the checked sizes of ``share_beta_segments``.  ``recon``: the
        keys of the mesh-error step to return as well (``_recon_keys``): the call is then ``smplfit_fit_recon_f32``."""
        bm = self.body_model
        device = bm.v_template.device
        for t in (target_vertices, target_joints, vertex_weights, joint_weights):
            if t is not None and t.requires_grad and torch.is_grad_enabled():  # (fit() wraps this call in _FitFn instead)
                raise NotImplementedError('the HIP fit kernels are not differentiable; detach the inputs')
        J, V, S = bm.num_joints, bm.num_vertices, self.n_betas
        if target_vertices.ndim != 3 or tuple(target_vertices.shape[1:]) != (V, 3):
            raise ValueError(f'target_vertices must have shape (batch, {V}, 3), got {tuple(target_vertices.shape)}')
        B = target_vertices.shape[0]
        prep = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        tv, tj, vw, jw = prep(target_vertices), prep(target_joints), prep(vertex_weights), prep(joint_weights)
        if tj is not None and tuple(tj.shape) != (B, J, 3):
            raise ValueError(f'target_joints must have shape ({B}, {J}, 3), got {tuple(tj.shape)}')
        if vw is not None and tuple(vw.shape) != (B, V):
            raise ValueError(f'vertex_weights must have shape ({B}, {V})')
        if jw is not None and tuple(jw.shape) != (B, J):
            raise ValueError(f'joint_weights must have shape ({B}, {J})')
        init_pose = None if initial_pose_rotvecs is None else prep(initial_pose_rotvecs.reshape(B, J * 3))
        init_betas = None if initial_shape_betas is None else prep(initial_shape_betas)[:, :S].contiguous()
        init_kid = None
        if initial_kid_factor is not None:
            init_kid = torch.as_tensor(initial_kid_factor, dtype=torch.float32, device=device).reshape(-1)
            init_kid = init_kid.expand(B).contiguous() if init_kid.numel() == 1 else init_kid.contiguous()
        pose = torch.empty((B, 3 * J), dtype=torch.float32, device=device)
        betas = torch.empty((B, S), dtype=torch.float32, device=device)
        trans = torch.empty((B, 3), dtype=torch.float32, device=device)
        orient = torch.empty((B, J, 3, 3), dtype=torch.float32, device=device)
        rel = torch.empty((B, J, 3, 3), dtype=torch.float32, device=device)
        kid = torch.empty((B,), dtype=torch.float32, device=device) if self.enable_kid else None
        scale = torch.empty((B,), dtype=torch.float32, device=device) if scale_mode else None
        shapes = dict(vertices=(B, V, 3), joints=(B, J, 3), vertex_error=(B, V), joint_error=(B, J))
        extra = {k: torch.empty(shapes[k], dtype=torch.float32, device=device) for k in recon}
        if B == 0 and share_beta_group is not None:
            raise ValueError('every rank of a sharded share_beta fit needs at least one instance')
        if B > 0:
            h = bm._native(device, kid=self.enable_kid)
            plan = self._segment_plan(device, segments) if segments is not None else None
            if _workspace is not None:
                ws = _workspace
            elif recon:
                ws = torch.empty(h.fit_recon_workspace_bytes(B, plan), dtype=torch.uint8, device=device)
            else:
                ws = self._segments_workspace(h, B, device, plan)
            callback, failure = _share_callback(ws, share_beta_group)
            with torch.cuda.device(device):
                stream = torch.cuda.current_stream(device).cuda_stream
                args = _lib.FitArgs(
                    target_vertices=tv.data_ptr(), target_joints=tj.data_ptr() if tj is not None else None,
                    vertex_weights=vw.data_ptr() if vw is not None else None,
                    joint_weights=jw.data_ptr() if jw is not None else None, batch=B, num_iter=int(num_iter),
                    beta_regularizer=float(beta_regularizer), beta_regularizer2=float(beta_regularizer2),
                    kid_regularizer=kid_reg, final_adjust_rots=int(bool(final_adjust_rots)),
                    initial_pose_rotvecs=init_pose.data_ptr() if init_pose is not None else None,
                    initial_shape_betas=init_betas.data_ptr() if init_betas is not None else None,
                    num_initial_betas=0 if init_betas is None else init_betas.shape[1],
                    initial_kid_factor=init_kid.data_ptr() if init_kid is not None else None,
                    share_beta=int(bool(share_beta)), scale_mode=int(scale_mode),
                    scale_regularizer=float(scale_regularizer), pose_rotvecs=pose.data_ptr(),
                    shape_betas=betas.data_ptr(), trans=trans.data_ptr(),
                    kid_factor=kid.data_ptr() if kid is not None else None, orientations=orient.data_ptr(),
                    relative_orientations=rel.data_ptr(),
                    scale_corr=scale.data_ptr() if scale is not None else None, workspace=ws.data_ptr(),
                    workspace_bytes=ws.numel(), hip_stream=stream, share_allreduce=callback)
                if recon:
                    rargs = _lib.FitReconArgs(**{k: t.data_ptr() for k, t in extra.items()})
                    rc = _lib.load().smplfit_fit_recon_f32(h.ptr, C.byref(args), plan.ptr if plan is not None else None,
                                                           C.byref(rargs))
                else:
                    rc = _lib.load().smplfit_fit_segments_f32(h.ptr, C.byref(args), plan.ptr if plan is not None else None)
                if failure:
                    raise failure[0]
                _lib.check(rc)
        result = dict(pose_rotvecs=pose, shape_betas=betas, trans=trans, orientations=orient,
                      relative_orientations=rel)
        if self.enable_kid:
            result['kid_factor'] = kid
        if scale_mode:
            result['scale_corr'] = scale
        result.update(extra)
        return result

    @staticmethod
    def _robust_options(loss, tuning, scale, scale_floor, batch):
        """``loss, tuning, scale, scale_floor`` of :meth:`fit_robust` / :meth:`_robust_weights`, checked on the host:
        ``(loss id, tuning, fixed scale or 0, (B,) scale tensor or None, scale_floor)``."""
        if loss not in _lib.ROBUST_LOSSES:
            raise ValueError(f'loss must be one of {list(_lib.ROBUST_LOSSES)}, got {loss!r}')
        tuning = float(_lib.ROBUST_TUNING[loss] if tuning is None else tuning)
        if not (tuning > 0 and np.isfinite(tuning)):
            raise ValueError(f'tuning must be positive and finite, got {tuning}')
        scale_floor = float(scale_floor)
        fixed, rows = 0.0, None
        if isinstance(scale, torch.Tensor) and scale.ndim > 0:
            if tuple(scale.shape) != (batch,) or not scale.is_floating_point():
                raise ValueError(f'scale must be None, a positive number or a floating-point tensor of shape ({batch},), '
                                 f'got shape {tuple(scale.shape)}')
            rows = scale
        elif scale is not None:
            fixed = float(scale)
            if not (fixed > 0 and np.isfinite(fixed)):
                raise ValueError(f'scale must be positive and finite, got {fixed}')
        elif not (scale_floor > 0 and np.isfinite(scale_floor)):
            raise ValueError(f'scale_floor must be positive and finite, got {scale_floor}')
        return _lib.ROBUST_LOSSES[loss], tuning, fixed, rows, scale_floor

    def _robust_weights(self, vertex_error, joint_error=None, vertex_weights=None, joint_weights=None, *,
                        loss='geman_mcclure', tuning=None, scale=None, scale_floor=1e-3, _out=None):
        """The reweighting step alone (``smplfit_robust_weights_f32``): from errors ``(B, N_v)`` and
        optionally ``(B, N_j)`` — any counts, not the model's — and optional prior weights of the same shapes,
        ``robust_scale`` (B,), ``robust_vertex_weights`` and, with joint errors, ``robust_joint_weights``; the options
        are those of :meth:`fit_robust`.  ``_out``: a dict of preallocated contiguous fp32 result tensors by those
        keys."""
        if vertex_error.ndim != 2 or vertex_error.shape[1] < 1:
            raise ValueError(f'vertex_error must have shape (batch, N >= 1), got {tuple(vertex_error.shape)}')
        B, Nv = vertex_error.shape
        if joint_error is not None and (joint_error.ndim != 2 or joint_error.shape[0] != B or joint_error.shape[1] < 1):
            raise ValueError(f'joint_error must have shape ({B}, N >= 1), got {tuple(joint_error.shape)}')
        Nj = 0 if joint_error is None else joint_error.shape[1]
        if vertex_weights is not None and tuple(vertex_weights.shape) != (B, Nv):
            raise ValueError(f'vertex_weights must have shape ({B}, {Nv})')
        if joint_weights is not None and (joint_error is None or tuple(joint_weights.shape) != (B, Nj)):
            raise ValueError(f'joint_weights need joint_error and the shape ({B}, {Nj})')
        loss_id, tuning, fixed, rows, scale_floor = self._robust_options(loss, tuning, scale, scale_floor, B)
        device = vertex_error.device if vertex_error.device.type == 'cuda' else self.body_model.v_template.device
        if device.type != 'cuda':
            raise RuntimeError("smplfitter_amd runs on MI355X only: move the model or the errors to a 'cuda' (ROCm) device")
        prep = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        ev, ej, w0v, w0j, rows = prep(vertex_error), prep(joint_error), prep(vertex_weights), prep(joint_weights), prep(rows)
        out = dict(_out or {})
        shapes = dict(robust_vertex_weights=(B, Nv), robust_scale=(B,))
        if ej is not None:
            shapes['robust_joint_weights'] = (B, Nj)
        for k, sh in shapes.items():
            t = out.get(k)
            if t is None:
                out[k] = torch.empty(sh, dtype=torch.float32, device=device)
            elif tuple(t.shape) != sh or t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
                raise ValueError(f'_out[{k!r}] must be a contiguous float32 tensor of shape {sh} on {device}')
        out = {k: out[k] for k in shapes}
        if B > 0:
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            with torch.cuda.device(device):
                args = _lib.RobustWeightsArgs(
                    batch=B, num_vertex_errors=Nv, num_joint_errors=Nj, vertex_error=p(ev), joint_error=p(ej),
                    vertex_weights=p(w0v), joint_weights=p(w0j), loss=loss_id, tuning=tuning, scale=fixed,
                    scale_rows=p(rows), scale_floor=scale_floor, out_vertex_weights=p(out['robust_vertex_weights']),
                    out_joint_weights=p(out.get('robust_joint_weights')), out_scale=p(out['robust_scale']),
                    hip_stream=torch.cuda.current_stream(device).cuda_stream)
                _lib.check(_lib.load().smplfit_robust_weights_f32(C.byref(args)))
        return out

    def fit_robust(
        self,
        target_vertices: torch.Tensor,
        target_joints: Optional[torch.Tensor] = None,
        vertex_weights: Optional[torch.Tensor] = None,
        joint_weights: Optional[torch.Tensor] = None,
        *,
        loss: str = 'geman_mcclure',
        tuning: Optional[float] = None,
        scale=None,
        scale_floor: float = 1e-3,
        num_rounds: int = 2,
        num_iter: int = 1,
        round_num_iter: Optional[int] = None,
        beta_regularizer: float = 1,
        beta_regularizer2: float = 0,
        kid_regularizer: Optional[float] = None,
        share_beta: bool = False,
        final_adjust_rots: bool = True,
        scale_target: bool = False,
        scale_fit: bool = False,
        requested_keys: Optional[list[str]] = None,
        _workspace: Optional[torch.Tensor] = None,
        share_beta_group=None,
        share_beta_segments=None,
    ) -> dict[str, torch.Tensor]:
        """:meth:`fit` for targets with gross outliers (not in the reference): the fit, then
        ``num_rounds`` times the per-point errors at its results, weights from them, and the fit again with those
        weights from the previous pose — one native call (``smplfit_fit_robust_f32``), nothing between the fits but one
        mesh-error pass and one reweighting launch.

        Per row ``b`` the weights are ``w0 * psi(e / (tuning * sigma_b))`` with the prior weights ``w0`` given here
        (``vertex_weights, joint_weights``; none: 1) and ``psi`` of ``loss``: ``'huber'`` min(1, 1/u), ``'cauchy'``
        1/(1+u²), ``'geman_mcclure'`` 1/(1+u²)², ``'tukey'`` (1-u²)² below 1 and exactly 0 from 1 on.  ``tuning=None``
        picks 1.345 / 2.385 / 3.0 / 4.685 (API defaults).  ``scale``: ``None`` — ``sigma_b = max(1.4826 * lower median of
        the row's vertex errors with a positive prior weight, scale_floor)``, found on the device —, a positive number
        for all rows, or a ``(B,)`` tensor.  The joints are weighted with the same ``sigma_b``.  ``round_num_iter``:
        ``num_iter`` of the later rounds (``None``: ``num_iter``).  A row with a non-finite error, or with an entry of a
        ``(B,)`` ``scale`` that is not positive and finite (the tensor is read on the device alone), gets NaN scale and
        weights throughout, and with them a non-finite fit; other rows are not affected.

        Returns ``fit``'s keys (``requested_keys`` as there, the four reconstruction keys included: measured at the last
        round's results) plus ``robust_vertex_weights`` (B, V), ``robust_joint_weights`` (B, J) with target joints and
        ``robust_scale`` (B,): the weights and scales that produced the last round.  ``num_rounds=0`` returns the bits
        of ``fit``, the prior weights (or ones) and NaN scales.  The rounds have the bits of the same loop written with
        ``fit(requested_keys=[errors])``, :meth:`_robust_weights` and a warm ``fit``.

        ``ValueError``: wrong shapes, an unknown loss, bad numbers.  ``NotImplementedError``: ``scale_target`` /
        ``scale_fit``, ``share_beta_group``, inputs that require grad, ``torch.compile``.  A caller ``_workspace`` has
        the size of ``Handle.fit_robust_workspace_bytes``."""
        if requested_keys is None:
            requested_keys = ['pose_rotvecs']
        bm = self.body_model
        J, V, S = bm.num_joints, bm.num_vertices, self.n_betas
        if target_vertices.ndim != 3 or tuple(target_vertices.shape[1:]) != (V, 3):
            raise ValueError(f'target_vertices must have shape (batch, {V}, 3), got {tuple(target_vertices.shape)}')
        B = target_vertices.shape[0]
        if target_joints is not None and tuple(target_joints.shape) != (B, J, 3):
            raise ValueError(f'target_joints must have shape ({B}, {J}, 3), got {tuple(target_joints.shape)}')
        if vertex_weights is not None and tuple(vertex_weights.shape) != (B, V):
            raise ValueError(f'vertex_weights must have shape ({B}, {V})')
        if joint_weights is not None and tuple(joint_weights.shape) != (B, J):
            raise ValueError(f'joint_weights must have shape ({B}, {J})')
        loss_id, tuning, fixed, rows, scale_floor = self._robust_options(loss, tuning, scale, scale_floor, B)
        num_rounds, num_iter = int(num_rounds), int(num_iter)
        round_num_iter = num_iter if round_num_iter is None else int(round_num_iter)
        if num_rounds < 0:
            raise ValueError(f'num_rounds must be >= 0, got {num_rounds}')
        if num_iter < 1 or round_num_iter < 1:
            raise ValueError(f'num_iter and round_num_iter must be >= 1, got {num_iter} and {round_num_iter}')
        segments = None
        if share_beta_segments is not None:
            if share_beta_group is not None:
                raise ValueError('share_beta_segments cannot be combined with share_beta_group')
            segments = _segment_sizes(share_beta_segments, B)
            share_beta = True
        if scale_target or scale_fit:
            raise NotImplementedError('fit_robust does not serve scale_target / scale_fit (which target the errors of a '
                                      'scaled fit refer to is undecided)')
        if share_beta_group is not None:
            raise NotImplementedError('fit_robust does not serve share_beta_group (a sharded share_beta fit)')
        if torch.compiler.is_compiling():
            raise NotImplementedError('fit_robust cannot be traced; call it outside the compiled region')
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in
                                          (target_vertices, target_joints, vertex_weights, joint_weights, rows)):
            raise NotImplementedError('fit_robust is not differentiable; detach the inputs')
        recon = _recon_keys(requested_keys, target_joints)
        kid_reg = float(beta_regularizer if kid_regularizer is None else kid_regularizer)

        device = bm.v_template.device
        prep = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        tv, tj, vw, jw, rows = prep(target_vertices), prep(target_joints), prep(vertex_weights), prep(joint_weights), prep(rows)
        new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)  # noqa: E731
        result = dict(pose_rotvecs=new(B, 3 * J), shape_betas=new(B, S), trans=new(B, 3), orientations=new(B, J, 3, 3),
                      relative_orientations=new(B, J, 3, 3))
        if self.enable_kid:
            result['kid_factor'] = new(B)
        shapes = dict(vertices=(B, V, 3), joints=(B, J, 3), vertex_error=(B, V), joint_error=(B, J))
        extra = {k: new(*shapes[k]) for k in recon}
        robust = dict(robust_vertex_weights=new(B, V), robust_scale=new(B))
        if tj is not None:
            robust['robust_joint_weights'] = new(B, J)
        if B > 0:
            h = bm._native(device, kid=self.enable_kid)
            plan = self._segment_plan(device, segments) if segments is not None else None
            ws = _workspace if _workspace is not None else torch.empty(h.fit_robust_workspace_bytes(B, plan), dtype=torch.uint8,
                                                                       device=device)
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            with torch.cuda.device(device):
                args = _lib.FitArgs(
                    target_vertices=p(tv), target_joints=p(tj), vertex_weights=p(vw), joint_weights=p(jw), batch=B,
                    num_iter=num_iter, beta_regularizer=float(beta_regularizer), beta_regularizer2=float(beta_regularizer2),
                    kid_regularizer=kid_reg, final_adjust_rots=int(bool(final_adjust_rots)), share_beta=int(bool(share_beta)),
                    pose_rotvecs=p(result['pose_rotvecs']), shape_betas=p(result['shape_betas']), trans=p(result['trans']),
                    kid_factor=p(result.get('kid_factor')), orientations=p(result['orientations']),
                    relative_orientations=p(result['relative_orientations']), workspace=ws.data_ptr(),
                    workspace_bytes=ws.numel(), hip_stream=torch.cuda.current_stream(device).cuda_stream)
                rargs = _lib.FitReconArgs(**{k: t.data_ptr() for k, t in extra.items()}) if recon else None
                bargs = _lib.FitRobustArgs(
                    loss=loss_id, tuning=tuning, scale=fixed, scale_rows=p(rows), scale_floor=scale_floor,
                    num_rounds=num_rounds, round_num_iter=round_num_iter, vertex_weights=p(robust['robust_vertex_weights']),
                    joint_weights=p(robust.get('robust_joint_weights')), scale_out=p(robust['robust_scale']))
                _lib.check(_lib.load().smplfit_fit_robust_f32(h.ptr, C.byref(args), plan.ptr if plan is not None else None,
                                                              C.byref(rargs) if rargs is not None else None, C.byref(bargs)))
        result.update(extra)
        result.update(robust)
        if 'pose_rotvecs' not in requested_keys:
            result.pop('pose_rotvecs', None)
        return result

    def _recon_after(self, recon, composed, target_vertices, target_joints, result, shape_betas=None, kid_factor=None):
        """The keys ``recon`` of the mesh-error step at the parameters of ``result`` (``orientations, trans`` and, unless
        given, ``shape_betas, kid_factor``), for the calls whose own native call does not return them: ``composed`` —
        gradients, tracing — from ``BodyModel.forward`` and PyTorch arithmetic, else ``smplfit_mesh_error_f32``."""
        if not recon:
            return {}
        bm = self.body_model
        params = dict(glob_rotmats=result['orientations'], trans=result['trans'],
                      shape_betas=result['shape_betas'] if shape_betas is None else shape_betas,
                      kid_factor=result.get('kid_factor') if kid_factor is None else kid_factor)
        call = bm._recon_composed if composed else bm._recon_direct
        return call(recon, target_vertices, target_joints, **params)

    @staticmethod
    def _segments_workspace(h, batch, device, plan):
        """The workspace of a fit or a shape solve: with a plan of segments, its own query's size."""
        nbytes = h.workspace_bytes(batch) if plan is None else plan.workspace_bytes(h)
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    FIT_GRAD_NAMES = ('target_vertices', 'target_joints', 'vertex_weights', 'joint_weights')

    def _fit_backward(self, target_vertices, target_joints, vertex_weights, joint_weights, num_iter, beta_regularizer,
                      beta_regularizer2, kid_regularizer, final_adjust_rots, grad_pose_rotvecs=None, grad_shape_betas=None,
                      grad_trans=None, grad_kid_factor=None, grad_orientations=None, grad_relative_orientations=None,
                      want=FIT_GRAD_NAMES):
        """The C-ABI call behind ``fit``'s backward (``smplfit_fit_backward_f32``): the gradients named in ``want`` (of
        ``FIT_GRAD_NAMES``; an input that was not given is skipped) as fp32 tensors on the model's device, from the
        cotangents of the results (each may be None: zero)."""
        bm = self.body_model
        device = bm.v_template.device
        prep = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        tv, tj, vw, jw = prep(target_vertices), prep(target_joints), prep(vertex_weights), prep(joint_weights)
        B, J, V, S = tv.shape[0], bm.num_joints, bm.num_vertices, self.n_betas
        cot = dict(grad_pose_rotvecs=(grad_pose_rotvecs, (B, 3 * J)), grad_shape_betas=(grad_shape_betas, (B, S)),
                   grad_trans=(grad_trans, (B, 3)), grad_kid_factor=(grad_kid_factor if self.enable_kid else None, (B,)),
                   grad_orientations=(grad_orientations, (B, J, 3, 3)),
                   grad_relative_orientations=(grad_relative_orientations, (B, J, 3, 3)))
        cot = {k: None if t is None else prep(t).reshape(sh) for k, (t, sh) in cot.items()}
        new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)  # noqa: E731
        given = dict(target_vertices=(tv, (B, V, 3)), target_joints=(tj, (B, J, 3)), vertex_weights=(vw, (B, V)),
                     joint_weights=(jw, (B, J)))
        out = {k: new(*given[k][1]) for k in want if given[k][0] is not None}
        if B == 0:
            return out
        h = bm._native(device, kid=self.enable_kid)
        ws = torch.empty(h.fit_backward_workspace_bytes(B, int(num_iter)), dtype=torch.uint8, device=device)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            args = _lib.FitBackwardArgs(
                target_vertices=p(tv), target_joints=p(tj), vertex_weights=p(vw), joint_weights=p(jw), batch=B,
                num_iter=int(num_iter), beta_regularizer=float(beta_regularizer), beta_regularizer2=float(beta_regularizer2),
                kid_regularizer=float(kid_regularizer), final_adjust_rots=int(bool(final_adjust_rots)),
                **{k: p(t) for k, t in cot.items()}, **{f'grad_{k}': p(out.get(k)) for k in self.FIT_GRAD_NAMES},
                workspace=ws.data_ptr(), workspace_bytes=ws.numel(), hip_stream=stream)
            _lib.check(_lib.load().smplfit_fit_backward_f32(h.ptr, C.byref(args)))
        return out

    def fit_with_known_pose(
        self,
        pose_rotvecs: torch.Tensor,
        target_vertices: torch.Tensor,
        target_joints: Optional[torch.Tensor] = None,
        vertex_weights: Optional[torch.Tensor] = None,
        joint_weights: Optional[torch.Tensor] = None,
        beta_regularizer: float = 1,
        beta_regularizer2: float = 0,
        scale_regularizer: float = 0,
        kid_regularizer: Optional[float] = None,
        share_beta: bool = False,
        scale_target: bool = False,
        scale_fit: bool = False,
        beta_regularizer_reference: Optional[torch.Tensor] = None,
        kid_regularizer_reference: Optional[torch.Tensor] = None,
        requested_keys: Optional[list[str]] = None,
        share_beta_group=None,
        share_beta_segments=None,
    ) -> dict[str, torch.Tensor]:
        """Shape and translation (and possibly scale) for a known pose (reference
        pt/bodyfitter.py:552-653): global rotations by forward kinematics of ``pose_rotvecs`` (the HIP
        forward kernel), then one shape solve (``smplfit_shape_solve_ex_f32``) with the target mean added
        back.  Differentiable: when gradients are enabled and a tensor input (the pose, a target, a weight, a ridge
        reference) requires grad, the results carry a ``grad_fn`` whose backward is the closed-form adjoint of the
        solve in HIP (``smplfit_shape_solve_backward_f32``); once differentiable; up to 17 shape
        unknowns; ``share_beta`` and the scale options with gradients raise ``NotImplementedError``.
        ``share_beta`` ignores the ridge references, as the reference's all-shared solve does
        (pt/lstsq.py:45-47).  ``share_beta_group``, ``share_beta_segments``: as in :meth:`fit`; so are the
        keys ``'vertices'``, ``'joints'``, ``'vertex_error'``, ``'joint_error'`` of ``requested_keys``, served by
        ``smplfit_mesh_error_f32`` behind the solve (not with the scale options)."""
        if scale_target and scale_fit:  # same check, same message as pt/bodyfitter.py:858-859
            raise ValueError('Only one of estim_scale_target and estim_scale_fit can be True')
        segments = None
        if share_beta_segments is not None:
            if share_beta_group is not None:
                raise ValueError('share_beta_segments cannot be combined with share_beta_group')
            segments = _segment_sizes(share_beta_segments, target_vertices.shape[0])
            if torch.compiler.is_compiling():
                raise NotImplementedError('share_beta_segments cannot be traced; call the fit outside the compiled region')
            share_beta = True
        if share_beta_group is not None and not share_beta:
            raise ValueError('share_beta_group needs share_beta=True')
        recon = _recon_keys(requested_keys or (), target_joints, scale_target=scale_target, scale_fit=scale_fit)
        if kid_regularizer_reference is not None and not self.enable_kid:
            kid_regularizer_reference = None  # the reference only reads it with enable_kid (:1235-1246)
        bm = self.body_model
        B = target_vertices.shape[0]
        pose = pose_rotvecs.reshape(B, bm.num_joints * 3)
        kid_reg = float(beta_regularizer if kid_regularizer is None else kid_regularizer)
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in
                                          (pose_rotvecs, target_vertices, target_joints, vertex_weights, joint_weights,
                                           beta_regularizer_reference, kid_regularizer_reference)):
            # differentiable: the shape solve under an autograd Function whose backward is one native call
            # (smplfit_shape_solve_backward_f32); the pose gets its gradient through G and BodyModel.forward's backward
            bad = [k for k, v in dict(share_beta=share_beta, scale_target=scale_target, scale_fit=scale_fit).items() if v]
            if bad:
                raise NotImplementedError(f'the differentiable fit_with_known_pose does not implement {", ".join(bad)}; '
                                          'detach the inputs to use the HIP path')
            if self.n_betas + int(self.enable_kid) > 17:
                raise NotImplementedError('the differentiable fit_with_known_pose serves at most 17 shape unknowns '
                                          '(betas + kid); detach the inputs to use the HIP path')
            G = bm(pose_rotvecs=pose, return_vertices=False)['orientations']
            opts = (float(beta_regularizer), float(beta_regularizer2), kid_reg)
            res = _KnownPoseFn.apply(self, opts, G, target_vertices, target_joints, vertex_weights, joint_weights,
                                     beta_regularizer_reference, kid_regularizer_reference)
            r = dict(shape_betas=res[0], trans=res[1])
            if self.enable_kid:
                r['kid_factor'] = res[2]
            composed = True
        else:
            composed = torch.compiler.is_compiling()
            G = bm(pose_rotvecs=pose, return_vertices=False)['orientations']
            r = self._shape_solve(G, target_vertices, target_joints, vertex_weights, joint_weights,
                                  beta_regularizer, beta_regularizer2, kid_regularizer=kid_reg,
                                  add_mean=True, want_mesh=False, share_beta=share_beta,
                                  scale_mode=1 if scale_target else 2 if scale_fit else 0,
                                  scale_regularizer=scale_regularizer, beta_ref=beta_regularizer_reference,
                                  kid_ref=kid_regularizer_reference, share_beta_group=share_beta_group,
                                  segments=segments)
        parents = bm.kintree_parents_tensor[1:].to(G.device)
        parent_glob = torch.cat(
            [torch.eye(3, device=G.device).expand(B, 1, 3, 3), G.index_select(1, parents)], dim=1)
        out = dict(shape_betas=r['shape_betas'], trans=r['trans'], orientations=G,
                   relative_orientations=parent_glob.transpose(-1, -2) @ G)
        if self.enable_kid:
            out['kid_factor'] = r['kid_factor']
        if 'scale_corr' in r:
            out['scale_corr'] = r['scale_corr']
        out.update(self._recon_after(recon, composed, target_vertices, target_joints, out))
        return out

    def fit_with_known_shape(
        self,
        shape_betas: torch.Tensor,
        target_vertices: torch.Tensor,
        target_joints: Optional[torch.Tensor] = None,
        vertex_weights: Optional[torch.Tensor] = None,
        joint_weights: Optional[torch.Tensor] = None,
        kid_factor: Optional[torch.Tensor] = None,
        num_iter: int = 1,
        final_adjust_rots: bool = True,
        initial_pose_rotvecs: Optional[torch.Tensor] = None,
        scale_fit: bool = False,
        requested_keys: Optional[list[str]] = None,
    ) -> dict[str, torch.Tensor]:
        """Pose and translation (and, with ``scale_fit``, a per-instance scale) for known shape
        parameters (reference pt/bodyfitter.py:655-838), one C-ABI call
        (``smplfit_fit_known_shape_f32``).  Result keys as the reference: ``trans``, ``orientations``,
        ``scale_corr`` with ``scale_fit``, ``relative_orientations`` / ``pose_rotvecs`` when requested.

        The reference's ``scale_fit`` branch only runs for a batch of one (a ``(B,)`` scale is multiplied
        into ``(B,3)`` means, :1675-1676); here every instance gets the scale a batch-of-one call gives.

        Differentiable: when gradients are enabled and ``shape_betas``, a target, a weight or a tensor ``kid_factor``
        requires grad, the results carry a ``grad_fn`` whose backward is one native call
        (``smplfit_fit_known_shape_backward_f32``); once differentiable; up to 17 shape unknowns
        natively (more, and ``native_backward=False``: the PyTorch restatement); ``scale_fit`` and
        ``initial_pose_rotvecs`` with gradients raise ``NotImplementedError``.

        ``requested_keys`` understands ``'vertices'``, ``'joints'``, ``'vertex_error'``, ``'joint_error'`` as in
        :meth:`fit`, served by ``smplfit_mesh_error_f32`` behind the fit (not with ``scale_fit``)."""
        if requested_keys is None:
            requested_keys = ['pose_rotvecs']
        bm = self.body_model
        for name, arg in (('target_vertices', target_vertices), ('shape_betas', shape_betas)):
            if isinstance(arg, np.ndarray):
                raise TypeError(f"Expected torch.Tensor for '{name}', got numpy.ndarray.")
        if target_vertices.ndim != 3:
            raise ValueError(f'Expected batched target_vertices (B, V, 3), got {tuple(target_vertices.shape)}')
        recon = _recon_keys(requested_keys, target_joints, scale_fit=scale_fit)
        composed = torch.compiler.is_compiling()
        if torch.is_grad_enabled() and not torch.compiler.is_compiling() and any(
                isinstance(t, torch.Tensor) and t.requires_grad for t in
                (shape_betas, target_vertices, target_joints, vertex_weights, joint_weights, kid_factor, initial_pose_rotvecs)):
            bad = [k for k, v in dict(scale_fit=scale_fit, initial_pose_rotvecs=initial_pose_rotvecs).items()
                   if v is not None and v is not False]
            if bad:
                raise NotImplementedError(f'the differentiable fit does not implement {", ".join(bad)}; detach the inputs to use the HIP path')
            n_unknowns = bm.num_betas + int(kid_factor is not None)
            composed = True
            if self.native_backward and n_unknowns <= 17 and target_vertices.shape[0] > 0:
                opts = (int(num_iter), bool(final_adjust_rots))
                pose, trans, orient, rel = _KnownShapeFn.apply(self, opts, shape_betas, kid_factor, target_vertices,
                                                               target_joints, vertex_weights, joint_weights)
                out = dict(trans=trans, orientations=orient, relative_orientations=rel, pose_rotvecs=pose)
            else:
                # the PyTorch restatement, in fp64: in fp32 it leaves the joint-weight gradient of a known-shape fit (of
                # order 1e-7 .. 1e-4: the joints of a part agree on its rotation whatever their weights) at rounding noise
                device = bm.v_template.device
                mv = lambda t: t.to(device) if isinstance(t, torch.Tensor) else t  # noqa: E731
                out = self._torchfit_route(dtype=torch.float64).fit_with_known_shape(
                    mv(shape_betas), mv(target_vertices), mv(target_joints), mv(vertex_weights), mv(joint_weights),
                    mv(kid_factor), num_iter=int(num_iter), final_adjust_rots=bool(final_adjust_rots))
                out = {k: v.to(target_vertices.dtype) for k, v in out.items()}
        else:
            out = self._fit_known_shape_direct(shape_betas, target_vertices, target_joints, vertex_weights, joint_weights,
                                               kid_factor, num_iter, final_adjust_rots, initial_pose_rotvecs, scale_fit)
        out.update(self._recon_after(recon, composed, target_vertices, target_joints, out, shape_betas=shape_betas,
                                     kid_factor=kid_factor))
        if 'relative_orientations' not in requested_keys and 'pose_rotvecs' not in requested_keys:
            out.pop('relative_orientations')
        if 'pose_rotvecs' not in requested_keys:
            out.pop('pose_rotvecs')
        return out

    def _torchfit_route(self, stacklevel=3, dtype=torch.float32):
        """The PyTorch restatement of this fitter (pt/_autograd.py) in ``dtype``, built on first use; the first one
        comes with the warning."""
        from ._autograd import TorchFit

        if self.body_model.v_template.device.type != 'cuda':
            raise RuntimeError("smplfitter_amd runs on MI355X only: move the model and the inputs to a 'cuda' (ROCm) device")
        attr = '_torchfit' if dtype == torch.float32 else '_torchfit64'
        if getattr(self, attr) is None:
            first = self._torchfit is None and self._torchfit64 is None
            setattr(self, attr, TorchFit(self.body_model, enable_kid=self.enable_kid, dtype=dtype))
            if first:
                # said once per fitter: a caller that feeds network outputs in training mode without detach() lands here
                import warnings

                warnings.warn('smplfitter_amd: inputs of BodyFitter.fit require gradients — this call runs the PyTorch '
                              'restatement (pt/_autograd.py), hundreds of times slower than the HIP kernels; detach() the '
                              'inputs or call under torch.no_grad() unless the gradients are wanted', RuntimeWarning,
                              stacklevel=stacklevel)
        return getattr(self, attr)

    def _fit_known_shape_direct(self, shape_betas, target_vertices, target_joints, vertex_weights, joint_weights,
                                kid_factor, num_iter, final_adjust_rots, initial_pose_rotvecs, scale_fit):
        """The C-ABI call of ``fit_with_known_shape`` (``smplfit_fit_known_shape_f32``); every result key."""
        bm = self.body_model
        device = bm.v_template.device
        prep = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        tv, tj, vw, jw = prep(target_vertices), prep(target_joints), prep(vertex_weights), prep(joint_weights)
        B, J = tv.shape[0], bm.num_joints
        betas = prep(shape_betas)[:, :bm.num_betas].contiguous()
        kid = None
        if kid_factor is not None:
            kid = torch.as_tensor(kid_factor, dtype=torch.float32, device=device).detach().reshape(-1)
            kid = kid.expand(B).contiguous() if kid.numel() == 1 else kid.contiguous()
        init = None if initial_pose_rotvecs is None else prep(initial_pose_rotvecs.reshape(B, J * 3))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)  # noqa: E731
        pose, trans = new(B, J * 3), new(B, 3)
        orient, rel = new(B, J, 3, 3), new(B, J, 3, 3)
        scale = new(B) if scale_fit else None
        if B > 0:
            h = bm._native(device, kid=kid is not None)
            ws = bm._workspace(h, B, device)
            with torch.cuda.device(device):
                stream = torch.cuda.current_stream(device).cuda_stream
                _lib.check(_lib.load().smplfit_fit_known_shape_f32(
                    h.ptr, _ptr(betas), betas.shape[1], _ptr(kid), _ptr(init), _ptr(tv), _ptr(tj), _ptr(vw),
                    _ptr(jw), B, int(num_iter), int(bool(final_adjust_rots)), int(bool(scale_fit)),
                    _ptr(pose), _ptr(trans), _ptr(scale), _ptr(orient), _ptr(rel), _ptr(ws), ws.numel(),
                    C.c_void_p(stream)))
        out = dict(trans=trans, orientations=orient)
        if scale_fit:
            out['scale_corr'] = scale
        out['relative_orientations'] = rel
        out['pose_rotvecs'] = pose
        return out

    KNOWN_SHAPE_GRAD_NAMES = ('shape_betas', 'kid_factor', 'target_vertices', 'target_joints', 'vertex_weights',
                              'joint_weights')

    def _fit_known_shape_backward(self, shape_betas, kid_factor, target_vertices, target_joints, vertex_weights,
                                  joint_weights, num_iter, final_adjust_rots, grad_pose_rotvecs=None, grad_trans=None,
                                  grad_orientations=None, grad_relative_orientations=None, want=KNOWN_SHAPE_GRAD_NAMES):
        """The C-ABI call behind ``fit_with_known_shape``'s backward (``smplfit_fit_known_shape_backward_f32``): the
        gradients named in ``want`` (of ``KNOWN_SHAPE_GRAD_NAMES``; an input that was not given is skipped) as fp32
        tensors on the model's device, from the cotangents of the results (each may be None: zero).  ``shape_betas``
        gets the width of the caller's tensor, zero beyond the model's betas; ``kid_factor`` is (B)."""
        bm = self.body_model
        device = bm.v_template.device
        prep = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        tv, tj, vw, jw = prep(target_vertices), prep(target_joints), prep(vertex_weights), prep(joint_weights)
        B, J, V = tv.shape[0], bm.num_joints, bm.num_vertices
        given = prep(shape_betas)
        betas = given[:, :bm.num_betas].contiguous()
        kid = None
        if kid_factor is not None:
            kid = torch.as_tensor(kid_factor, dtype=torch.float32, device=device).detach().reshape(-1)
            kid = kid.expand(B).contiguous() if kid.numel() == 1 else kid.contiguous()
        cot = dict(grad_pose_rotvecs=(grad_pose_rotvecs, (B, 3 * J)), grad_trans=(grad_trans, (B, 3)),
                   grad_orientations=(grad_orientations, (B, J, 3, 3)),
                   grad_relative_orientations=(grad_relative_orientations, (B, J, 3, 3)))
        cot = {k: None if t is None else prep(t).reshape(sh) for k, (t, sh) in cot.items()}
        new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)  # noqa: E731
        ins = dict(shape_betas=(betas, (B, betas.shape[1])), kid_factor=(kid, (B,)), target_vertices=(tv, (B, V, 3)),
                   target_joints=(tj, (B, J, 3)), vertex_weights=(vw, (B, V)), joint_weights=(jw, (B, J)))
        out = {k: new(*ins[k][1]) for k in want if ins[k][0] is not None}
        if B > 0:
            h = bm._native(device, kid=kid is not None)
            ws = torch.empty(h.fit_known_shape_backward_workspace_bytes(B, int(num_iter)), dtype=torch.uint8, device=device)
            p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
            with torch.cuda.device(device):
                stream = torch.cuda.current_stream(device).cuda_stream
                args = _lib.FitKnownShapeBackwardArgs(
                    shape_betas=betas.data_ptr(), num_betas_given=betas.shape[1], kid_factor=p(kid), target_vertices=p(tv),
                    target_joints=p(tj), vertex_weights=p(vw), joint_weights=p(jw), batch=B, num_iter=int(num_iter),
                    final_adjust_rots=int(bool(final_adjust_rots)), **{k: p(t) for k, t in cot.items()},
                    **{f'grad_{k}': p(out.get(k)) for k in self.KNOWN_SHAPE_GRAD_NAMES},
                    workspace=ws.data_ptr(), workspace_bytes=ws.numel(), hip_stream=stream)
                _lib.check(_lib.load().smplfit_fit_known_shape_backward_f32(h.ptr, C.byref(args)))
        if 'shape_betas' in out and given.shape[1] > betas.shape[1]:  # columns beyond the model's betas
            out['shape_betas'] = torch.cat([out['shape_betas'], given.new_zeros(B, given.shape[1] - betas.shape[1])], 1)
        return out

    # -- stage entry points, used by the parity tests ---------------------------------------------
    def _part_rotations(self, target_vertices, target_joints=None, vertex_weights=None, joint_weights=None):
        """Global part rotations of the first rotation pass (centring included)."""
        bm = self.body_model
        device = bm.v_template.device
        prep = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        tv, tj, vw, jw = prep(target_vertices), prep(target_joints), prep(vertex_weights), prep(joint_weights)
        B = tv.shape[0]
        G = torch.empty((B, bm.num_joints, 3, 3), dtype=torch.float32, device=device)
        h = bm._native(device, kid=self.enable_kid)
        ws = bm._workspace(h, B, device)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _lib.check(_lib.load().smplfit_part_rotations_f32(
                h.ptr, _ptr(tv), _ptr(tj), _ptr(vw), _ptr(jw), B, _ptr(G), _ptr(ws), ws.numel(),
                C.c_void_p(stream)))
        return G

    def _shape_solve(self, glob_rotmats, target_vertices, target_joints=None, vertex_weights=None,
                     joint_weights=None, beta_regularizer=1.0, beta_regularizer2=0.0,
                     kid_regularizer=None, add_mean=False, want_mesh=True, share_beta=False, scale_mode=0,
                     scale_regularizer=0.0, beta_ref=None, kid_ref=None, share_beta_group=None, segments=None):
        """One shape solve for given global rotations; targets are centred internally and the returned
        trans / vertices / joints live in the centred frame; ``add_mean`` adds the target mean back to
        trans alone (vertices / joints stay centred)."""
        bm = self.body_model
        device = bm.v_template.device
        prep = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        G, tv, tj = prep(glob_rotmats), prep(target_vertices), prep(target_joints)
        vw, jw = prep(vertex_weights), prep(joint_weights)
        B, J, V, S = tv.shape[0], bm.num_joints, bm.num_vertices, self.n_betas
        bref = None if beta_ref is None else prep(beta_ref)[:, :S].contiguous()
        kref = None
        if kid_ref is not None:
            kref = torch.as_tensor(kid_ref, dtype=torch.float32, device=device).reshape(-1)
            kref = kref.expand(B).contiguous() if kref.numel() == 1 else kref.contiguous()
        betas = torch.empty((B, S), dtype=torch.float32, device=device)
        trans = torch.empty((B, 3), dtype=torch.float32, device=device)
        verts = torch.empty((B, V, 3), dtype=torch.float32, device=device) if want_mesh else None
        joints = torch.empty((B, J, 3), dtype=torch.float32, device=device) if want_mesh else None
        kid = torch.empty((B,), dtype=torch.float32, device=device) if self.enable_kid else None
        scale = torch.empty((B,), dtype=torch.float32, device=device) if scale_mode else None
        kid_reg = float(beta_regularizer if kid_regularizer is None else kid_regularizer)
        h = bm._native(device, kid=self.enable_kid)
        plan = self._segment_plan(device, segments) if segments is not None else None
        ws = self._segments_workspace(h, B, device, plan)
        callback, failure = _share_callback(ws, share_beta_group)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            args = _lib.ShapeSolveArgs(
                glob_rotmats=p(G), target_vertices=p(tv), target_joints=p(tj), vertex_weights=p(vw),
                joint_weights=p(jw), batch=B, beta_regularizer=float(beta_regularizer),
                beta_regularizer2=float(beta_regularizer2), kid_regularizer=kid_reg,
                add_mean=int(bool(add_mean)), beta_regularizer_reference=p(bref),
                num_reference_betas=0 if bref is None else bref.shape[1], kid_regularizer_reference=p(kref),
                share_beta=int(bool(share_beta)), scale_mode=int(scale_mode),
                scale_regularizer=float(scale_regularizer), shape_betas=p(betas), trans=p(trans),
                kid_factor=p(kid), scale_corr=p(scale), vertices_out=p(verts), joints_out=p(joints),
                workspace=ws.data_ptr(), workspace_bytes=ws.numel(), hip_stream=stream,
                share_allreduce=callback)
            rc = _lib.load().smplfit_shape_solve_segments_f32(h.ptr, C.byref(args), plan.ptr if plan is not None else None)
            if failure:
                raise failure[0]
            _lib.check(rc)
        out = dict(shape_betas=betas, trans=trans)
        if want_mesh:
            out.update(vertices=verts, joints=joints)
        if self.enable_kid:
            out['kid_factor'] = kid
        if scale_mode:
            out['scale_corr'] = scale
        return out

    GRAD_NAMES = ('glob_rotmats', 'target_vertices', 'target_joints', 'vertex_weights', 'joint_weights',
                  'beta_regularizer_reference', 'kid_regularizer_reference')

    def _shape_solve_backward(self, glob_rotmats, target_vertices, target_joints, vertex_weights, joint_weights,
                              beta_regularizer, beta_regularizer2, kid_regularizer, beta_ref, kid_ref, shape_betas, trans,
                              kid_factor, grad_shape_betas=None, grad_trans=None, grad_kid_factor=None,
                              want=GRAD_NAMES):
        """The C-ABI call behind ``fit_with_known_pose``'s backward (``smplfit_shape_solve_backward_f32``): the
        gradients named in ``want`` (of ``GRAD_NAMES``; an input that was not given is skipped) as fp32 tensors on the
        model's device, in the shapes the native call writes.  ``shape_betas, trans, kid_factor``: the forward's
        results with the target mean added back."""
        bm = self.body_model
        device = bm.v_template.device
        prep = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        G, tv, tj = prep(glob_rotmats), prep(target_vertices), prep(target_joints)
        vw, jw = prep(vertex_weights), prep(joint_weights)
        B, J, V, S = tv.shape[0], bm.num_joints, bm.num_vertices, self.n_betas
        bref = None if beta_ref is None else prep(beta_ref)[:, :S].contiguous()
        kref = None
        if kid_ref is not None and self.enable_kid:
            kref = torch.as_tensor(kid_ref, dtype=torch.float32, device=device).detach().reshape(-1)
            kref = kref.expand(B).contiguous() if kref.numel() == 1 else kref.contiguous()
        betas, tr, kid = prep(shape_betas), prep(trans), prep(kid_factor) if self.enable_kid else None
        gb, gt = prep(grad_shape_betas), prep(grad_trans)
        gk = prep(grad_kid_factor) if self.enable_kid else None
        new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)  # noqa: E731
        given = dict(glob_rotmats=(G, (B, J, 3, 3)), target_vertices=(tv, (B, V, 3)), target_joints=(tj, (B, J, 3)),
                     vertex_weights=(vw, (B, V)), joint_weights=(jw, (B, J)),
                     beta_regularizer_reference=(bref, (B, 0 if bref is None else bref.shape[1])),
                     kid_regularizer_reference=(kref, (B,)))
        out = {k: new(*given[k][1]) for k in want if given[k][0] is not None}
        if tj is None:  # (no joint rows in the solve: their weights do not enter it)
            if 'joint_weights' in out:
                out['joint_weights'].zero_()
        h = bm._native(device, kid=self.enable_kid)
        ws = torch.empty(h.shape_solve_backward_workspace_bytes(B), dtype=torch.uint8, device=device)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        o = lambda k: p(out.get(k))  # noqa: E731
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            args = _lib.ShapeSolveBackwardArgs(
                glob_rotmats=p(G), target_vertices=p(tv), target_joints=p(tj), vertex_weights=p(vw),
                joint_weights=p(jw) if tj is not None else None, beta_regularizer=float(beta_regularizer),
                beta_regularizer2=float(beta_regularizer2), kid_regularizer=float(kid_regularizer),
                beta_regularizer_reference=p(bref), num_reference_betas=0 if bref is None else bref.shape[1],
                kid_regularizer_reference=p(kref), batch=B, shape_betas=p(betas), trans=p(tr), kid_factor=p(kid),
                grad_shape_betas=p(gb), grad_trans=p(gt), grad_kid_factor=p(gk),
                grad_target_vertices=o('target_vertices'), grad_target_joints=o('target_joints'),
                grad_vertex_weights=o('vertex_weights'),
                grad_joint_weights=o('joint_weights') if tj is not None else None,
                grad_beta_regularizer_reference=o('beta_regularizer_reference'),
                grad_kid_regularizer_reference=o('kid_regularizer_reference'),
                grad_glob_rotmats=o('glob_rotmats'), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                hip_stream=stream)
            _lib.check(_lib.load().smplfit_shape_solve_backward_f32(h.ptr, C.byref(args)))
        return out


class _FitFn(torch.autograd.Function):
    """``fit`` under autograd: the forward is ``BodyFitter._fit_direct`` (the same call, the same bits as without
    gradients), the backward one ``smplfit_fit_backward_f32``, which keeps nothing from the forward but its inputs."""

    @staticmethod
    def forward(ctx, fitter, opts, workspace, tv, tj, vw, jw):
        num_iter, reg, reg2, kid_reg, final_adjust = opts
        det = lambda t: None if t is None else t.detach()  # noqa: E731
        r = fitter._fit_direct(det(tv), det(tj), det(vw), det(jw), num_iter, reg, reg2, kid_reg, final_adjust, None, None,
                               None, workspace)
        ctx.fitter, ctx.opts = fitter, opts
        ctx.save_for_backward(tv, tj, vw, jw)
        ctx.set_materialize_grads(False)
        res = (r['pose_rotvecs'], r['shape_betas'], r['trans'], r['orientations'], r['relative_orientations'])
        return res + ((r['kid_factor'],) if fitter.enable_kid else ())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pose, g_betas, g_trans, g_orient, g_rel, g_kid=None):
        ins = ctx.saved_tensors
        names = BodyFitter.FIT_GRAD_NAMES
        want = tuple(n for n, t, need in zip(names, ins, ctx.needs_input_grad[3:]) if need and t is not None)
        g = ctx.fitter._fit_backward(*ins, *ctx.opts, grad_pose_rotvecs=g_pose, grad_shape_betas=g_betas, grad_trans=g_trans,
                                     grad_kid_factor=g_kid, grad_orientations=g_orient, grad_relative_orientations=g_rel,
                                     want=want)
        grads = [None if g.get(n) is None else g[n].reshape(t.shape).to(device=t.device, dtype=t.dtype)
                 for n, t in zip(names, ins)]
        return (None, None, None, *grads)


class _KnownShapeFn(torch.autograd.Function):
    """``fit_with_known_shape`` under autograd: the forward is ``BodyFitter._fit_known_shape_direct`` (the same call, the
    same bits as without gradients), the backward one ``smplfit_fit_known_shape_backward_f32``, which keeps nothing
    from the forward but its inputs."""

    @staticmethod
    def forward(ctx, fitter, opts, betas, kid, tv, tj, vw, jw):
        num_iter, final_adjust = opts
        r = fitter._fit_known_shape_direct(betas, tv, tj, vw, jw, kid, num_iter, final_adjust, None, False)
        ctx.fitter, ctx.opts = fitter, opts
        ctx.kid_scalar = kid if kid is not None and not isinstance(kid, torch.Tensor) else None
        ctx.save_for_backward(betas, kid if isinstance(kid, torch.Tensor) else None, tv, tj, vw, jw)
        ctx.set_materialize_grads(False)
        return r['pose_rotvecs'], r['trans'], r['orientations'], r['relative_orientations']

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pose, g_trans, g_orient, g_rel):
        ins = list(ctx.saved_tensors)
        names = BodyFitter.KNOWN_SHAPE_GRAD_NAMES
        want = tuple(n for n, t, need in zip(names, ins, ctx.needs_input_grad[2:]) if need and t is not None)
        call = list(ins)
        if call[1] is None:
            call[1] = ctx.kid_scalar
        g = ctx.fitter._fit_known_shape_backward(*call, *ctx.opts, grad_pose_rotvecs=g_pose, grad_trans=g_trans,
                                                 grad_orientations=g_orient, grad_relative_orientations=g_rel, want=want)
        grads = []
        for n, t in zip(names, ins):
            v = g.get(n) if n in want else None
            if v is None:
                grads.append(None)
                continue
            if n == 'kid_factor' and t.numel() == 1 and v.numel() != 1:  # a broadcast kid factor
                v = v.sum()
            grads.append(v.reshape(t.shape).to(device=t.device, dtype=t.dtype))
        return (None, None, *grads)


class _KnownPoseFn(torch.autograd.Function):
    """The shape solve of ``fit_with_known_pose`` under autograd: the forward is ``BodyFitter._shape_solve`` (the same
    call, the same bits as without gradients), the backward one ``smplfit_shape_solve_backward_f32``."""

    @staticmethod
    def forward(ctx, fitter, opts, G, tv, tj, vw, jw, bref, kref):
        reg, reg2, kid_reg = opts
        r = fitter._shape_solve(G, tv, tj, vw, jw, reg, reg2, kid_regularizer=kid_reg, add_mean=True, want_mesh=False,
                                beta_ref=bref, kid_ref=kref)
        ctx.fitter, ctx.opts = fitter, opts
        ctx.kref_scalar = kref if kref is not None and not isinstance(kref, torch.Tensor) else None
        saved = [G, tv, tj, vw, jw, bref, kref if isinstance(kref, torch.Tensor) else None, r['shape_betas'], r['trans'],
                 r.get('kid_factor')]
        ctx.save_for_backward(*saved)
        if fitter.enable_kid:
            return r['shape_betas'], r['trans'], r['kid_factor']
        return r['shape_betas'], r['trans']

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_betas, g_trans, g_kid=None):
        G, tv, tj, vw, jw, bref, kref, betas, trans, kid = ctx.saved_tensors
        if kref is None:
            kref = ctx.kref_scalar
        ins = (G, tv, tj, vw, jw, bref, kref)
        names = BodyFitter.GRAD_NAMES
        want = tuple(n for n, t, need in zip(names, ins, ctx.needs_input_grad[2:]) if need and t is not None)
        reg, reg2, kid_reg = ctx.opts
        g = ctx.fitter._shape_solve_backward(G, tv, tj, vw, jw, reg, reg2, kid_reg, bref, kref, betas, trans, kid,
                                             g_betas, g_trans, g_kid, want=want)
        grads = []
        for n, t in zip(names, ins):
            v = g.get(n)
            if v is None:
                grads.append(None)
                continue
            if n == 'beta_regularizer_reference' and v.shape[1] != t.shape[1]:  # columns beyond the model's betas
                v = torch.cat([v, v.new_zeros(v.shape[0], t.shape[1] - v.shape[1])], 1)
            if n == 'kid_regularizer_reference' and t.numel() == 1 and v.numel() != 1:  # a broadcast reference
                v = v.sum()
            grads.append(v.reshape(t.shape).to(device=t.device, dtype=t.dtype))
        return (None, None, *grads)
