"""The arbiter of ``BodyFitter.fit_robust``: the reweighting in numpy, and the rounds written on top of
``oracle.smplfit_oracle`` as it stands — ``OracleFitter.fit`` with weights and ``initial_pose_rotvecs``,
``OracleModel.forward(glob_rotmats=...)`` — in the dtype of the oracle model it is given (fp64: the arbiter; fp32: the
floor).  Shared by tests/test_robust_host.py and tests/test_gpu_robust.py."""

import numpy as np

import util

LOSSES = ('huber', 'cauchy', 'geman_mcclure', 'tukey')
TUNING = dict(huber=1.345, cauchy=2.385, geman_mcclure=3.0, tukey=4.685)
MAD = 1.4826


def psi(loss, u):
    """The weight functions of u >= 0, in u's dtype."""
    u = np.asarray(u)
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        if loss == 'huber':
            return np.minimum(1.0, 1.0 / u).astype(u.dtype)
        if loss == 'cauchy':
            return 1.0 / (1.0 + u * u)
        if loss == 'geman_mcclure':
            return 1.0 / (1.0 + u * u) ** 2
        if loss == 'tukey':
            return np.where(u < 1.0, (1.0 - u * u) ** 2, 0.0).astype(u.dtype)
    raise KeyError(loss)


def lower_median(e, w0=None):
    """Per row: element (n - 1) // 2 of the sorted eligible entries (``w0 > 0``; all without ``w0``), and n."""
    med, cnt = np.zeros(e.shape[0], e.dtype), np.zeros(e.shape[0], np.int64)
    for b in range(e.shape[0]):
        x = e[b] if w0 is None else e[b][w0[b] > 0]
        cnt[b] = x.size
        if x.size:
            med[b] = np.sort(x)[(x.size - 1) // 2]
    return med, cnt


def scale_of(ev, w0v=None, scale=None, scale_floor=1e-3):
    """sigma per row in ev's dtype: a fixed number, a (B,) array, or max(1.4826 * lower median, floor) — in fp32 the
    one product the kernel forms, so the comparison is to the bit."""
    dt = ev.dtype.type
    B = ev.shape[0]
    if scale is not None:
        return np.broadcast_to(np.asarray(scale, ev.dtype), (B,)).copy()
    med, cnt = lower_median(ev, w0v)
    return np.where(cnt > 0, np.maximum(dt(MAD) * med, dt(scale_floor)), dt(scale_floor)).astype(ev.dtype)


def weights_of(e, w0, loss, tuning, sigma):
    """w0 * psi(e / (tuning * sigma)) in fp64 from inputs of any dtype; a prior weight of 0 gives 0."""
    e64, s64 = np.asarray(e, np.float64), np.asarray(sigma, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = psi(loss, e64 / (float(tuning) * s64[:, None]))
    if w0 is None:
        return w
    w0 = np.asarray(w0, np.float64)
    return np.where(w0 == 0, 0.0, w0 * w)


def errors_of(om, fit, tv, tj):
    """Unweighted distances of the model at ``fit`` (orientations, shape_betas, trans) to the targets, in om's dtype."""
    fw = om.forward(glob_rotmats=fit['orientations'], shape_betas=fit['shape_betas'], trans=fit['trans'])
    ev = np.linalg.norm(fw['vertices'] - np.asarray(tv, om.dtype), axis=-1)
    ej = None if tj is None else np.linalg.norm(fw['joints'] - np.asarray(tj, om.dtype), axis=-1)
    return ev, ej


def fit_robust(om, tv, tj=None, w0v=None, w0j=None, loss='geman_mcclure', tuning=None, scale=None, scale_floor=1e-3,
               num_rounds=2, num_iter=1, round_num_iter=None, **fit_kw):
    """The rounds in om's dtype: ``fit``; then per round the errors at the previous results, sigma and the weights, and
    ``fit`` with them from the previous pose.  Returns the last fit plus robust_vertex_weights / robust_joint_weights /
    robust_scale."""
    fitter = util.O.OracleFitter(om)
    dt = om.dtype
    tuning = TUNING[loss] if tuning is None else tuning
    r = fitter.fit(tv, tj, w0v, w0j, num_iter=num_iter, **fit_kw)
    wv, wj, sigma = w0v, w0j, None
    for _ in range(num_rounds):
        ev, ej = errors_of(om, r, tv, tj)
        sigma = scale_of(ev, w0v, scale, scale_floor)
        wv = weights_of(ev, w0v, loss, tuning, sigma).astype(dt)
        wj = None if tj is None else weights_of(ej, w0j, loss, tuning, sigma).astype(dt)
        r = fitter.fit(tv, tj, wv, wj, num_iter=num_iter if round_num_iter is None else round_num_iter,
                       initial_pose_rotvecs=r['pose_rotvecs'], **fit_kw)
    r = dict(r)
    r.update(robust_vertex_weights=wv, robust_joint_weights=wj, robust_scale=sigma)
    return r


def outlier_inputs(om64, B=4, frac=0.15, sigma=0.3):
    """The targets of the fp64 and the purpose tests: parameters from ``default_rng(5)`` (pose N(0, 0.25), betas N(0, 1),
    trans N(0, 0.5)), the fp64 mesh; outliers from ``default_rng(7)`` (mask ``random < frac``, displaced by N(0, sigma)
    per coordinate); targets rounded to fp32.  Returns clean vertices (fp64), target vertices and joints (fp32)."""
    rng = np.random.default_rng(5)
    pose = rng.normal(0, 0.25, (B, om64.J * 3))
    betas = rng.normal(0, 1.0, (B, om64.S))
    trans = rng.normal(0, 0.5, (B, 3))
    fw = om64.forward(pose, betas, trans)
    rng = np.random.default_rng(7)
    mask = rng.random((B, om64.V)) < frac
    noise = rng.normal(0, sigma, (B, om64.V, 3))
    tv = (fw['vertices'] + mask[..., None] * noise).astype(np.float32)
    return fw['vertices'], tv, fw['joints'].astype(np.float32)


def mean_distance(om64, fit, clean):
    """Largest per-row mean distance of the mesh at ``fit`` (pose_rotvecs, shape_betas, trans) to ``clean``, in fp64."""
    v = om64.forward(fit['pose_rotvecs'], fit['shape_betas'], fit['trans'])['vertices']
    return float(np.linalg.norm(v - clean, axis=-1).mean(1).max())
