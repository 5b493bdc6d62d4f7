"""The fp64 arbiter of the aligned errors in numpy: the weighted Procrustes transform by SVD with the
determinant fix, the errors under a transform, and the condition of a row's alignment.  Shared by tests/test_align_host.py
and tests/test_gpu_mesh_align.py."""

import numpy as np

MODES = ('none', 'root', 'translation', 'rigid', 'similarity')


def procrustes64(x, y, w=None, mode='similarity'):
    """x, y (B, N, 3), w (B, N) or None -> dict(s (B,), R (B, 3, 3), t (B, 3), cond (B,)) in fp64 with y ~ s R x + t:
    'translation', 'rigid' (R = U diag(1, 1, d) V^T, d = sign det(U V^T)) or 'similarity'.  cond = (sigma_2 + d sigma_3)
    / sigma_1 of K: the gap that decides how far a perturbation of K turns R.  Rows with W = 0, a bad weight, a non-finite
    point or (similarity) no spread are NaN."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    B, N = x.shape[:2]
    w = np.ones((B, N)) if w is None else np.asarray(w, np.float64)
    with np.errstate(all='ignore'):
        w = np.where((w >= 0) & np.isfinite(w), w, np.nan)
        W = w.sum(1)
        xm, ym = (w[..., None] * x).sum(1) / W[:, None], (w[..., None] * y).sum(1) / W[:, None]
        xc, yc = x - xm[:, None], y - ym[:, None]
        K = np.einsum('bn,bnr,bnc->brc', w, yc, xc)
        good = np.isfinite(K).all((1, 2)) & (W > 0)
        U, S, Vh = np.linalg.svd(np.where(good[:, None, None], K, np.eye(3)))
        d = np.sign(np.linalg.det(U @ Vh))
        d[d == 0] = 1.0
        D = np.stack([np.ones(B), np.ones(B), d], -1)
        R = np.broadcast_to(np.eye(3), (B, 3, 3)).copy()
        s = np.ones(B)
        if mode in ('rigid', 'similarity'):
            R = (U * D[:, None, :]) @ Vh
        if mode == 'similarity':
            s = (S * D).sum(-1) / (w * (xc * xc).sum(-1)).sum(1)
        t = ym - s[:, None] * np.einsum('brc,bc->br', R, xm)
        cond = (S[:, 1] + d * S[:, 2]) / S[:, 0]
        ok = good & np.isfinite(s) & np.isfinite(t).all(-1)
    nan = np.nan
    return dict(s=np.where(ok, s, nan), R=np.where(ok[:, None, None], R, nan), t=np.where(ok[:, None], t, nan),
                cond=np.where(ok, cond, nan))


def root64(xj, yj, jw=None):
    """The 'root' transform from joints (B, J, 3): t = y_0 - x_0; NaN where the joint set is invalid."""
    xj, yj = np.asarray(xj, np.float64), np.asarray(yj, np.float64)
    B = xj.shape[0]
    p = procrustes64(xj, yj, jw, 'translation')
    ok = np.isfinite(p['s'])
    t = np.where(ok[:, None], yj[:, 0] - xj[:, 0], np.nan)
    return dict(s=np.where(ok, 1.0, np.nan), R=np.where(ok[:, None, None], np.eye(3), np.nan), t=t, cond=np.ones(B))


def identity64(B):
    return dict(s=np.ones(B), R=np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), t=np.zeros((B, 3)), cond=np.ones(B))


def move64(x, tf):
    """s R x + t in fp64 for x (B, N, 3)."""
    x = np.asarray(x, np.float64)
    return np.asarray(tf['s'], np.float64)[:, None, None] * np.einsum('brc,bnc->bnr', np.asarray(tf['R'], np.float64), x) \
        + np.asarray(tf['t'], np.float64)[:, None]


def errors64(x, y, tf):
    return np.linalg.norm(move64(x, tf) - np.asarray(y, np.float64), axis=-1)


def row_mean64(e, w=None):
    e = np.asarray(e, np.float64)
    if w is None:
        return e.mean(1)
    w = np.asarray(w, np.float64)
    with np.errstate(all='ignore'):
        w = np.where((w >= 0) & np.isfinite(w), w, np.nan)
        return (w * e).sum(1) / w.sum(1)
