"""Throughput of BodyFlipper.flip on one GPU: the fused call (smplfit_flip_f32) against the reference's sequence of calls
(forward + flip_vertices + warm-started fit, same kernels otherwise), for the SMPL- and SMPL-X-shaped synthetic models
at num_iter 1 and 3, beside the fused same-topology BodyConverter.convert for scale.  One JSON line per measurement;
--out FILE also writes them as one JSON list.

Usage:  python tools/bench_flip.py [--batch 4096] [--steps 20] [--warmup 3] [--out profiles/flip_mi355x.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from smplfitter_amd import synth  # noqa: E402
from smplfitter_amd.pt import BodyConverter, BodyFlipper, BodyModel  # noqa: E402


def timed(fn, steps, warmup):
    """Median over `steps` single calls, each timed with HIP events on the current stream (ms)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    B = a.batch
    root = synth.ensure_model_root(kinds=('smpl', 'smplx'))
    os.environ['DATA_ROOT'] = synth.write_transfer_files('/tmp/smplfit_bench_flip_data')
    rows = []
    for kind in ('smpl', 'smplx'):
        m = BodyModel(kind, 'neutral', model_root=f'{root}/{kind}', num_betas=10, device=dev)
        fl = BodyFlipper(m)
        assert fl._plan(dev) is not None, 'the fused flip does not apply'
        conv = BodyConverter(m, m)
        rs = np.random.RandomState(0)
        t = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)  # noqa: E731
        pose, betas, trans = t(rs.randn(B, 3 * m.num_joints) * 0.1), t(rs.randn(B, 10)), t(rs.randn(B, 3))
        for ni in (1, 3):
            legs = dict(
                flip_fused=lambda: fl.flip(pose, betas, trans, num_iter=ni),
                flip_unfused=lambda: fl._flip_unfused(pose, betas, trans, None, ni),
                convert_fused=lambda: conv.convert(pose, betas, trans, num_iter=ni))
            for leg, fn in legs.items():
                med, best = timed(fn, a.steps, a.warmup)
                r = dict(model=kind, leg=leg, num_iter=ni, batch=B, median_ms=round(med, 4), min_ms=round(best, 4),
                         per_s=round(B / med * 1e3))
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
