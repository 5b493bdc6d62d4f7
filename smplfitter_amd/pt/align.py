"""Procrustes alignment of point sets and the aligned errors (no counterpart in the reference).

``align_points`` is the step on two arbitrary (B, N, 3) tensors (``smplfit_align_points_f32``); ``BodyModel.mesh_error``
uses the same definitions for the posed model.  ``procrustes`` / ``aligned_errors`` are the PyTorch composition both fall
back to where gradients, tracing or CPU tensors rule the native call out: centred in fp64, ``torch.linalg.svd`` with the
determinant fix, differentiable as far as PyTorch's SVD is."""

from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib

POINT_MODES = ('translation', 'rigid', 'similarity')


def _clean_weights(w):
    """Weights as fp64, NaN where negative or not finite (their row is then NaN throughout)."""
    w = w.to(torch.float64)
    return torch.where((w >= 0) & torch.isfinite(w), w, torch.full_like(w, float('nan')))


def procrustes(x, y, w, mode):
    """(s (B,), R (B, 3, 3), t (B, 3)) in fp64 with ``y ~ s R x + t`` for x, y (B, N, 3) and weights w (B, N) or None:
    the table of DESIGN.md §24 for 'translation', 'rigid' and 'similarity'.  Rows without a transform are NaN."""
    x, y = x.to(torch.float64), y.to(torch.float64)
    B, N = x.shape[:2]
    w = torch.ones((B, N), dtype=torch.float64, device=x.device) if w is None else _clean_weights(w)
    W = w.sum(1)
    xm = (w[..., None] * x).sum(1) / W[:, None]
    ym = (w[..., None] * y).sum(1) / W[:, None]
    xc, yc = x - xm[:, None], y - ym[:, None]
    eye = torch.eye(3, dtype=torch.float64, device=x.device).expand(B, 3, 3)
    R, s = eye, torch.ones_like(W)
    if mode in ('rigid', 'similarity'):
        K = torch.einsum('bn,bnr,bnc->brc', w, yc, xc)
        good = torch.isfinite(K).all(-1).all(-1)
        U, _, Vh = torch.linalg.svd(torch.where(good[:, None, None], K, eye))
        d = torch.sign(torch.linalg.det(U @ Vh))
        d = torch.where(d == 0, torch.ones_like(d), d)
        R = U @ torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1)) @ Vh
        if mode == 'similarity':
            s = (R * K).sum((-1, -2)) / (w * (xc * xc).sum(-1)).sum(1)
    t = ym - s[:, None] * torch.einsum('brc,bc->br', R, xm)
    ok = (W > 0) & torch.isfinite(s) & torch.isfinite(t).all(-1) & torch.isfinite(R).all(-1).all(-1)
    nan = torch.full_like(s, float('nan'))
    return (torch.where(ok, s, nan), torch.where(ok[:, None, None], R, nan[:, None, None]),
            torch.where(ok[:, None], t, nan[:, None]))


def aligned_errors(x, y, s, R, t):
    """|s R x + t - y| per point, in fp64 throughout (a row far from the origin loses nothing)."""
    x, y = x.to(torch.float64), y.to(torch.float64)
    return torch.linalg.vector_norm(s[:, None, None] * torch.einsum('brc,bnc->bnr', R, x) + t[:, None] - y, dim=-1)


def weighted_row_mean(e, w):
    """sum w e / sum w per row in fp64 (w None: the plain mean)."""
    e = e.to(torch.float64)
    if w is None:
        return e.mean(1)
    w = _clean_weights(w)
    return (w * e).sum(1) / w.sum(1)


def _check_points(source, target, weights, align):
    for name, arg in (('source', source), ('target', target), ('weights', weights)):
        if arg is not None and not isinstance(arg, torch.Tensor):
            raise TypeError(f"Expected torch.Tensor for '{name}', got {type(arg).__name__}.")
    if align not in POINT_MODES:
        raise ValueError(f'align must be one of {POINT_MODES}, got {align!r}')
    if source.ndim != 3 or source.shape[-1] != 3 or source.shape[1] < 1:
        raise ValueError(f'source must have shape (batch, N, 3) with N >= 1, got {tuple(source.shape)}')
    if tuple(target.shape) != tuple(source.shape):
        raise ValueError(f'target must have the shape of source {tuple(source.shape)}, got {tuple(target.shape)}')
    if weights is not None and tuple(weights.shape) != tuple(source.shape[:2]):
        raise ValueError(f'weights must have shape {tuple(source.shape[:2])}, got {tuple(weights.shape)}')
    if source.device != target.device or (weights is not None and weights.device != source.device):
        raise ValueError('source, target and weights must be on one device')


def align_points(source: torch.Tensor, target: torch.Tensor, weights: Optional[torch.Tensor] = None,
                 align: str = 'similarity') -> dict[str, torch.Tensor]:
    """Moves ``source`` (B, N, 3) onto ``target`` (B, N, 3) by the weighted Procrustes transform of ``align``
    ('translation', 'rigid', 'similarity') and measures it: ``error`` (B, N) = |s R x + t - y|,
    unweighted; ``mean_error`` (B,) = sum w e / sum w; ``scale`` (B,), ``rotation`` (B, 3, 3), ``translation`` (B, 3).
    ``weights`` (B, N) steer the alignment and the mean.  A row without a transform — zero total weight, no spread
    under 'similarity', a negative or non-finite weight, a non-finite point — is NaN throughout, no other row is.
    On the GPU one C-ABI call (``smplfit_align_points_f32``: fp64 sums in a fixed order, so two runs give the same
    bits); with gradients enabled and an input that requires grad, under ``torch.compile`` and for CPU tensors the
    same keys come from PyTorch arithmetic in fp64."""
    _check_points(source, target, weights, align)
    ins = (source, target, weights)
    B, N = source.shape[:2]
    composed = torch.compiler.is_compiling() or source.device.type != 'cuda' or (
        torch.is_grad_enabled() and any(a is not None and a.requires_grad for a in ins))
    if composed:
        s, R, t = procrustes(source, target, weights, align)
        e = aligned_errors(source, target, s, R, t)
        f = lambda a: a.to(torch.float32)  # noqa: E731
        return dict(error=f(e), mean_error=f(weighted_row_mean(e, weights)), scale=f(s), rotation=f(R), translation=f(t))
    device = source.device
    shapes = dict(error=(B, N), mean_error=(B,), scale=(B,), rotation=(B, 3, 3), translation=(B, 3))
    out = {k: torch.empty(v, dtype=torch.float32, device=device) for k, v in shapes.items()}
    if B == 0:
        return out
    prep = lambda a: None if a is None else a.to(dtype=torch.float32).contiguous()  # noqa: E731
    x, y, w = prep(source), prep(target), prep(weights)
    lib = _lib.load()
    ws = torch.empty(int(lib.smplfit_align_points_workspace_bytes(B, N)), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        args = _lib.AlignPointsArgs(
            batch=B, num_points=N, source=x.data_ptr(), target=y.data_ptr(), weights=None if w is None else w.data_ptr(),
            align=_lib.ALIGN_MODES[align], **{k: v.data_ptr() for k, v in out.items()}, workspace=ws.data_ptr(),
            workspace_bytes=ws.numel(), hip_stream=torch.cuda.current_stream(device).cuda_stream)
        _lib.check(lib.smplfit_align_points_f32(C.byref(args)))
    return out
