"""Fit with reconstruction: ``BodyFitter.fit(requested_keys=['vertices', 'joints', 'vertex_error',
'joint_error'])`` (smplfit_fit_recon_f32) against the composition a caller wrote before it — ``fit``, then
``BodyModel.forward(glob_rotmats=orientations, ...)``, then ``torch.linalg.vector_norm`` of the two differences — and
``BodyModel.mesh_error`` against ``forward`` plus the norms, on the synthetic SMPL-shaped model with target joints.
The two sides of a pair run alternately, call by call; medians of ``--reps`` warmed calls, each ending in a device
synchronise.

    python tools/bench_fit_recon.py [--batches 64 4096] [--reps 10] [--out profiles/fit_recon_mi355x.json]
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

KEYS = ['vertices', 'joints', 'vertex_error', 'joint_error']


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 4096])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--num-iter', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=('smpl',))
    m = BodyModel('smpl', 'neutral', model_root=f'{root}/smpl', num_betas=10, device=dev)
    f = BodyFitter(m)
    V, J, S = m.num_vertices, m.num_joints, m.num_betas
    res = dict(model='smpl', vertices=V, joints=J, betas=S, num_iter=a.num_iter, device=torch.cuda.get_device_name(0),
               library=_lib.load().smplfit_version().decode(), kernel_path=m.kernel_path(), reps=a.reps, batches={})
    # (B, V, 3) traffic per instance behind the fit, in bytes.  Fused: the mesh written, the targets read, the (B, V)
    # errors written.  Composition: the forward's mesh written; the difference reads mesh and targets and writes a
    # (B, V, 3); the norm reads it and writes (B, V).
    res['mesh_bytes_per_instance'] = dict(fused=2 * V * 12 + V * 4, composition=5 * V * 12 + V * 4,
                                          fused_errors_only=V * 12 + V * 4)
    rs = np.random.RandomState(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)  # noqa: E731
    kw = dict(num_iter=a.num_iter, beta_regularizer=1.0)
    for B in a.batches:
        fw = m(t(rs.randn(B, 3 * J) * 0.1), t(rs.randn(B, S) * 0.5), t(rs.randn(B, 3)))
        tv = fw['vertices'] + t(rs.randn(B, V, 3) * 0.002)
        tj = fw['joints'] + t(rs.randn(B, J, 3) * 0.002)

        def composition():
            r = f.fit(tv, tj, **kw)
            g = m(glob_rotmats=r['orientations'], shape_betas=r['shape_betas'], trans=r['trans'])
            r.update(vertices=g['vertices'], joints=g['joints'],
                     vertex_error=torch.linalg.vector_norm(g['vertices'] - tv, dim=-1),
                     joint_error=torch.linalg.vector_norm(g['joints'] - tj, dim=-1))
            return r

        fused = lambda: f.fit(tv, tj, requested_keys=['pose_rotvecs'] + KEYS, **kw)  # noqa: E731
        errors_only = lambda: f.fit(tv, tj, requested_keys=['pose_rotvecs', 'vertex_error', 'joint_error'], **kw)  # noqa: E731
        plain = lambda: f.fit(tv, tj, **kw)  # noqa: E731
        r = fused()
        c = composition()
        assert torch.equal(r['vertices'], c['vertices']) and torch.equal(r['joints'], c['joints'])
        dev_err = float((r['vertex_error'].double() - c['vertex_error'].double()).abs().max())
        p = dict(glob_rotmats=r['orientations'], shape_betas=r['shape_betas'], trans=r['trans'])

        def forward_norm():
            g = m(**p)
            return (torch.linalg.vector_norm(g['vertices'] - tv, dim=-1), torch.linalg.vector_norm(g['joints'] - tj, dim=-1))

        step = lambda: m.mesh_error(tv, tj, return_mesh=True, **p)  # noqa: E731
        step_errors = lambda: m.mesh_error(tv, tj, **p)  # noqa: E731
        comp_ms, fused_ms = alternate(composition, fused, a.reps)
        plain_ms, only_ms = alternate(plain, errors_only, a.reps)
        fn_ms, step_ms = alternate(forward_norm, step, a.reps)
        fwd_ms, step_e_ms = alternate(lambda: m(**p), step_errors, a.reps)
        res['batches'][str(B)] = dict(
            composition_ms=comp_ms, fit_recon_ms=fused_ms, ratio=comp_ms / fused_ms, fit_ms=plain_ms,
            fit_recon_errors_only_ms=only_ms, forward_plus_norms_ms=fn_ms, mesh_error_with_mesh_ms=step_ms,
            forward_ms=fwd_ms, mesh_error_ms=step_e_ms, vertex_error_vs_torch_max_abs=dev_err)
        print(B, json.dumps(res['batches'][str(B)]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(osp.dirname(osp.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
