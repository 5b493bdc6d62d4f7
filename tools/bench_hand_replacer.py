"""HandReplacer.replace_hand: the fused call (smplfit_replace_hands_f32) against the composition of the public entry
points (BodyFitter.fit with a (B, V) weight tensor, BodyModel.forward, three PyTorch elementwise passes), on the synthetic
SMPL-H-shaped model (52 joints, 16 betas), in instances/s with launch counts.

    python tools/bench_hand_replacer.py [--batches 4096 256] [--reps 10] [--out profiles/hand_replacer_mi355x.json]
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
from smplfitter_amd.pt import HandReplacer  # noqa: E402


def rate(fn, batch, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return batch / float(np.median(times)), float(np.median(times) * 1e3)


def launches(fn):
    """Kernel launches of one call, counted by the profiler (memcpy / memset entries excluded)."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    except Exception as e:  # no tracer on this machine: the count is left out, the rates stand
        print(f'launch count unavailable: {e}', flush=True)
        return None
    return int(sum(e.count for e in prof.key_averages()
                   if e.device_type == torch.autograd.DeviceType.CUDA and not e.key.lower().startswith(('memcpy', 'memset'))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[4096, 256])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    root = synth.write_hand_replacer_files(os.getenv('SMPLFIT_SYNTH_DATA_HAND', '/tmp/smplfit_synth_data_hand_seed0'))
    rs = np.random.RandomState(0)
    hr = HandReplacer(torch.from_numpy((rs.randn(156) * 0.3).astype(np.float32)),
                      model_root=f'{root}/body_models/smplh16', data_root=root, device=dev)
    bm = hr.smplh_bm
    assert hr._plan(dev) is not None, 'the fused call does not apply'
    V, J, S = bm.num_vertices, bm.num_joints, bm.num_betas
    res = dict(model=synth.HAND_REPLACER_SMPLH, vertices=V, joints=J, betas=S, device=torch.cuda.get_device_name(0),
               library=_lib.load().smplfit_version().decode(), reps=a.reps, batches={})
    # (B, V, 3) / (B, V) traffic per instance outside the fit's and the forward's own streams, in bytes:
    # fused: input read by the fit, input read by the blend, result written; composition: input read by the fit, the
    # (B, V) weights written by repeat() and read by the fit, the forward's mesh written, and the blend's three
    # elementwise passes (new - in: 2 reads 1 write; * mix: 1 read 1 write; in + ...: 2 reads 1 write)
    res['mesh_bytes_per_instance'] = dict(fused=3 * V * 12, unfused=V * 12 + 2 * V * 4 + V * 12 + 8 * V * 12)
    for B in a.batches:
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)  # noqa: E731
        pose = rs.randn(B, J, 3) * 0.1
        verts = bm(t(pose.reshape(B, -1)), t(rs.randn(B, S) * 0.5), t(rs.randn(B, 3)))['vertices']
        verts = verts + t(rs.randn(B, V, 3) * 0.002)
        fused = lambda: hr._replace_fused(verts)['vertices']  # noqa: E731
        unfused = lambda: hr._replace_unfused(verts)['vertices']  # noqa: E731
        err = float((fused().double() - unfused().double()).norm(dim=-1).max())
        fr, fms = rate(fused, B, a.reps)
        ur, ums = rate(unfused, B, a.reps)
        res['batches'][str(B)] = dict(fused_instances_per_s=fr, fused_ms=fms, unfused_instances_per_s=ur, unfused_ms=ums,
                                      ratio=fr / ur, fused_launches=launches(fused), unfused_launches=launches(unfused),
                                      fused_vs_unfused_max_vertex_l2=err)
        print(B, json.dumps(res['batches'][str(B)]), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(osp.dirname(osp.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
