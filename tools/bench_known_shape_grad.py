"""Differentiable BodyFitter.fit_with_known_shape: the forward alone and forward + backward (target gradients only /
every gradient: betas, targets, weights) on the HIP adjoint (smplfit_fit_known_shape_backward_f32), and the PyTorch
restatement (native_backward=False, fp64) at B = 256 ONLY, as tools/bench_fit_grad.py (that route is not
run at any larger size).  Synthetic SMPL / SMPL-X, target joints, both weights, num_iter 1 and 3, with the refinement.
Medians of warmed repeats, each call followed by a device synchronise.

    python tools/bench_known_shape_grad.py [--batches 4096 64] [--reps 10] [--out profiles/known_shape_grad_mi355x.json]
"""

import argparse
import json
import os
import os.path as osp
import sys
import time
import warnings

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

from smplfitter_amd import _lib, synth  # noqa: E402
from smplfitter_amd.pt import BodyFitter, BodyModel  # noqa: E402

TORCHFIT_BATCH = 256  # the only size the PyTorch route is run at


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


def inputs(bm, B, dev):
    rs = np.random.RandomState(B)
    V, J = bm.num_vertices, bm.num_joints
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)  # noqa: E731
    betas = t(rs.randn(B, 10))
    with torch.no_grad():
        o = bm(t(rs.randn(B, J * 3) * 0.2), betas, t(rs.randn(B, 3)))
    x = dict(shape_betas=betas, target_vertices=o['vertices'] + t(rs.randn(B, V, 3) * 0.005), target_joints=o['joints'] + t(rs.randn(B, J, 3) * 0.005),
             vertex_weights=t(rs.uniform(0.5, 1.5, (B, V))), joint_weights=t(rs.uniform(0.5, 1.5, (B, J))))
    cot = dict(pose_rotvecs=t(rs.randn(B, J * 3)), trans=t(rs.randn(B, 3)))
    return x, cot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[4096, 64])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    warnings.simplefilter('ignore', RuntimeWarning)
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=('smpl', 'smplx'), seed=0)
    res = dict(device=torch.cuda.get_device_name(0), library=_lib.load().smplfit_version().decode(), reps=a.reps, models={})
    targets = ('target_vertices', 'target_joints')
    every = ('shape_betas',) + targets + ('vertex_weights', 'joint_weights')
    for kind in ('smpl', 'smplx'):
        bm = BodyModel(kind, 'neutral', model_root=f'{root}/{kind}', num_betas=10, device=dev)
        fitters = {True: BodyFitter(bm), False: BodyFitter(bm, native_backward=False)}
        res['models'][kind] = dict(vertices=bm.num_vertices, joints=bm.num_joints, configs={})
        for num_iter in (1, 3):
            kw = dict(num_iter=num_iter, final_adjust_rots=True)
            for B in sorted(set(a.batches) | {TORCHFIT_BATCH}, reverse=True):
                x, cot = inputs(bm, B, dev)

                def forward():
                    with torch.no_grad():
                        return fitters[True].fit_with_known_shape(**x, **kw)

                def diff(names, native=True):
                    xs = {k: (v.detach().requires_grad_() if k in names else v) for k, v in x.items()}
                    r = fitters[native].fit_with_known_shape(**xs, **kw)
                    sum((r[k] * c).sum() for k, c in cot.items()).backward()
                    return [xs[k].grad for k in names]

                row = dict(forward_ms=median_ms(forward, a.reps), forward_backward_targets_ms=median_ms(lambda: diff(targets), a.reps),
                           forward_backward_all_ms=median_ms(lambda: diff(every), a.reps))
                if B == TORCHFIT_BATCH:
                    row['torchfit_forward_backward_all_ms'] = median_ms(lambda: diff(every, native=False), max(3, a.reps // 3), warm=1)
                    row['torchfit_over_native'] = row['torchfit_forward_backward_all_ms'] / row['forward_backward_all_ms']
                res['models'][kind]['configs'][f'num_iter={num_iter},B={B}'] = row
                print(kind, num_iter, B, json.dumps(row), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(osp.dirname(osp.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
