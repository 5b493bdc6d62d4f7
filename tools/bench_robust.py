"""Reweighted fits: ``BodyFitter.fit_robust`` (smplfit_fit_robust_f32) against the same loop written with
the calls that existed before it — ``fit(requested_keys=[..., 'vertex_error', 'joint_error'])``, the lower median of the
vertex errors by ``torch.kthvalue``, the weights in PyTorch, a warm ``fit``, and round again (the last fit without the
error keys: both legs run one mesh-error pass per round) — on the synthetic SMPL- and
SMPL-X-shaped models with target joints, a tenth of the target vertices displaced by N(0, 0.3 m).  The composition runs
none of the new code.  The two legs run alternately, call by call, ``--passes`` times over in one run; medians of
``--reps`` warmed calls, each ending in a device synchronise.

    python tools/bench_robust.py [--models smpl smplx] [--batches 64 4096] [--rounds 1 2] [--reps 10] [--passes 3]
                                 [--out profiles/robust_mi355x.json]
"""

import argparse
import json
import os
import os.path as osp
import sys
import time

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

from smplfitter_amd import _lib, synth  # noqa: E402
from smplfitter_amd.pt import BodyFitter, BodyModel  # noqa: E402

TUNING, FLOOR = 3.0, 1e-3  # Geman-McClure, fit_robust's defaults


def alternate(fa, fb, reps):
    """Median milliseconds of two callables run in turn, after three warm-up rounds."""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    return float(np.median(ta) * 1e3), float(np.median(tb) * 1e3)


def composition(f, tv, tj, num_rounds, kw):
    """The loop a caller wrote before fit_robust: the error keys only on the fits that a further round follows."""
    keys = ['pose_rotvecs', 'vertex_error', 'joint_error']
    r = f.fit(tv, tj, requested_keys=keys if num_rounds else keys[:1], **kw)
    V = tv.shape[1]
    for k in range(num_rounds):
        med = torch.kthvalue(r['vertex_error'], (V - 1) // 2 + 1, dim=1).values
        den = TUNING * torch.clamp(1.4826 * med, min=FLOOR)[:, None]
        wv = 1 / (1 + (r['vertex_error'] / den) ** 2) ** 2
        wj = 1 / (1 + (r['joint_error'] / den) ** 2) ** 2
        r = f.fit(tv, tj, wv, wj, initial_pose_rotvecs=r['pose_rotvecs'],
                  requested_keys=keys if k + 1 < num_rounds else keys[:1], **kw)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', nargs='+', default=['smpl', 'smplx'])
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 4096])
    ap.add_argument('--rounds', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--num-iter', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=tuple(a.models))
    res = dict(num_iter=a.num_iter, loss='geman_mcclure', device=torch.cuda.get_device_name(0),
               library=_lib.load().smplfit_version().decode(), reps=a.reps, passes=a.passes, rows=[])
    rs = np.random.RandomState(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)  # noqa: E731
    kw = dict(num_iter=a.num_iter, beta_regularizer=1.0)
    for name in a.models:
        m = BodyModel(name, 'neutral', model_root=f'{root}/{name}', num_betas=10, device=dev)
        f = BodyFitter(m)
        V, J, S = m.num_vertices, m.num_joints, m.num_betas
        for B in a.batches:
            fw = m(t(rs.randn(B, 3 * J) * 0.1), t(rs.randn(B, S) * 0.5), t(rs.randn(B, 3)))
            g = torch.Generator(device=dev).manual_seed(B)
            rnd = lambda *sh: torch.randn(*sh, device=dev, generator=g)  # noqa: E731
            hit = (torch.rand(B, V, 1, device=dev, generator=g) < 0.1).float()
            tv = fw['vertices'] + rnd(B, V, 3) * 0.002 + hit * rnd(B, V, 3) * 0.3
            tj = fw['joints'] + rnd(B, J, 3) * 0.002
            plain = lambda: f.fit(tv, tj, **kw)  # noqa: E731
            errors = lambda: f.fit(tv, tj, requested_keys=['pose_rotvecs', 'vertex_error', 'joint_error'], **kw)  # noqa: E731
            fit_ms, fit_err_ms = alternate(plain, errors, a.reps)
            r0 = errors()
            step = lambda: f._robust_weights(r0['vertex_error'], r0['joint_error'])  # noqa: E731
            kth = lambda: torch.kthvalue(r0['vertex_error'], (V - 1) // 2 + 1, dim=1)  # noqa: E731
            step_ms, kth_ms = alternate(step, kth, a.reps)
            for nr in a.rounds:
                fused = lambda: f.fit_robust(tv, tj, num_rounds=nr, **kw)  # noqa: E731
                comp = lambda: composition(f, tv, tj, nr, kw)  # noqa: E731
                x, y = fused(), comp()
                # (the composition's weights come from PyTorch arithmetic: equal to rounding, not to the bit)
                dmax = float((x['shape_betas'] - y['shape_betas']).abs().max())
                runs = [alternate(fused, comp, a.reps) for _ in range(a.passes)]
                row = dict(model=name, kernel_path=m.kernel_path(), vertices=V, batch=B, num_rounds=nr,
                           fit_robust_ms=[v[0] for v in runs], composition_ms=[v[1] for v in runs],
                           fit_robust_median_ms=float(np.median([v[0] for v in runs])),
                           composition_median_ms=float(np.median([v[1] for v in runs])), fit_ms=fit_ms,
                           fit_with_errors_ms=fit_err_ms, robust_weights_ms=step_ms, kthvalue_ms=kth_ms,
                           betas_vs_composition_max_abs=dmax)
                row['ratio'] = row['composition_median_ms'] / row['fit_robust_median_ms']
                res['rows'].append(row)
                print(json.dumps(row), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(osp.dirname(osp.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
