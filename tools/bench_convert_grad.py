"""Differentiable BodyConverter.convert: per direction (SMPL -> SMPL-X and back, synthetic models and
transfer files) and batch, num_iter 1 — the fused call without gradients, the forward under gradients (the three calls),
forward + backward, ``fit`` forward + backward of the output model at the same size in the same run, and
``smplfit_transfer_f32`` / ``smplfit_transfer_backward_f32`` alone.  Medians of warmed repeats, each call followed by a
device synchronise.  Nothing is gated on these numbers.

    python tools/bench_convert_grad.py [--batches 64 256 4096] [--reps 10] [--out profiles/convert_grad_mi355x.json]
"""

import argparse
import json
import os
import os.path as osp
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

from smplfitter_amd import _lib, synth  # noqa: E402
from smplfitter_amd.pt import BodyConverter, BodyModel  # noqa: E402


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256, 4096])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    warnings.simplefilter('ignore', RuntimeWarning)
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=('smpl', 'smplx_fat'), seed=0)
    os.environ['DATA_ROOT'] = synth.write_transfer_files(osp.join(tempfile.gettempdir(), 'smplfit_bench_convert_data'), seed=0,
                                                         smplx_kind='smplx_fat')
    models = dict(smpl=BodyModel('smpl', 'neutral', model_root=f'{root}/smpl', num_betas=10, device=dev),
                  smplx=BodyModel('smplx', 'neutral', model_root=f'{root}/smplx_fat', num_betas=10, device=dev))
    res = dict(device=torch.cuda.get_device_name(0), library=_lib.load().smplfit_version().decode(), reps=a.reps, num_iter=1,
               directions={})
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)  # noqa: E731
    for tag, (ni, no) in dict(s2x=('smpl', 'smplx'), x2s=('smplx', 'smpl')).items():
        mi, mo = models[ni], models[no]
        conv = BodyConverter(mi, mo)
        assert conv._plan(dev) is not None
        res['directions'][tag] = dict(vertices_in=mi.num_vertices, vertices_out=mo.num_vertices, configs={})
        for B in a.batches:
            rs = np.random.RandomState(B)
            x = dict(pose_rotvecs=t(rs.randn(B, 3 * mi.num_joints) * 0.2), shape_betas=t(rs.randn(B, 10)), trans=t(rs.randn(B, 3)))
            cot = dict(pose_rotvecs=t(rs.randn(B, 3 * mo.num_joints)), shape_betas=t(rs.randn(B, 10)), trans=t(rs.randn(B, 3)))
            with torch.no_grad():
                mesh_in = mi(**x)['vertices']
                mesh_out = conv.convert_vertices(mesh_in)
            g_out, g_in = torch.randn_like(mesh_out), torch.empty_like(mesh_in)
            tr, stream = conv._transfer(dev), torch.cuda.current_stream(dev).cuda_stream
            fit_kw = dict(num_iter=1, beta_regularizer=0.0, final_adjust_rots=False, kid_regularizer=1e9)

            def fused():
                with torch.no_grad():
                    return conv.convert(**x, num_iter=1)

            def forward_grad():
                xs = {k: v.detach().requires_grad_() for k, v in x.items()}
                return xs, conv.convert(**xs, num_iter=1)

            def forward_backward():
                xs, r = forward_grad()
                sum((r[k] * c).sum() for k, c in cot.items()).backward()
                return [v.grad for v in xs.values()]

            def fit_forward_backward():
                tv = mesh_out.detach().requires_grad_()
                r = conv.fitter.fit(tv, **fit_kw)
                sum((r[k] * c).sum() for k, c in cot.items()).backward()
                return tv.grad

            row = dict(fused_no_grad_ms=median_ms(fused, a.reps), forward_grad_ms=median_ms(forward_grad, a.reps),
                       forward_backward_ms=median_ms(forward_backward, a.reps),
                       fit_forward_backward_ms=median_ms(fit_forward_backward, a.reps),
                       transfer_ms=median_ms(lambda: tr.forward(mesh_in.data_ptr(), B, mesh_out.data_ptr(), stream), a.reps),
                       transfer_backward_ms=median_ms(lambda: tr.backward(g_out.data_ptr(), B, g_in.data_ptr(), stream), a.reps))
            res['directions'][tag]['configs'][f'B={B}'] = row
            print(tag, B, json.dumps(row), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(osp.dirname(osp.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
