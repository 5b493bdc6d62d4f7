"""Forward and forward + backward of BodyModel.forward on one GPU, against a plain torch-op forward of the same function
(tests/grad_util.forward in fp32 on the GPU) differentiated by autograd, for the SMPL- and SMPL-X-shaped synthetic models
at B = 64, 4096 and 16384.  Legs: ``forward`` (no grad), ``forward_backward`` (forward under autograd + backward of a
loss over vertices and joints), ``torch_forward_backward`` (the baseline).  Median of HIP-event-timed single calls.
One JSON line per measurement; --out FILE also writes them as one JSON list.

--trace: the per-kernel split of one backward call (SMPL, B = 4096, all cotangents) and of one with no vertex
cotangent (the return_vertices=False path), from a child process run under ``rocprofv3 --kernel-trace``; the second must
launch no vertex-sized kernel (only k_bwd_joint), which the tool asserts.

Usage:  python tools/bench_forward_grad.py [--steps 20] [--warmup 3] [--trace] [--out profiles/forward_grad_mi355x.json]
"""
import argparse
import csv
import glob
import json
import re
import subprocess
import tempfile
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import grad_util  # noqa: E402
from smplfitter_amd import modelio, synth  # noqa: E402
from smplfitter_amd.pt import BodyModel  # noqa: E402


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


VERTEX_KERNELS = ('k_forward_joint', 'k_posedirs_gemm', 'k_bwd_vertex', 'k_bwd_reduce', 'k_bwd_combine')
TRACE_CALLS = 3


def one_backward(mode, B):
    """Child of --trace: TRACE_CALLS backward calls (BodyModel._backward_direct) on SMPL, all cotangents ('full') or
    joints and orientations only ('novert')."""
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=('smpl',))
    m = BodyModel('smpl', 'neutral', model_root=f'{root}/smpl', num_betas=10, device=dev)
    rs = np.random.RandomState(0)
    t = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)  # noqa: E731
    pose, betas, trans = t(rs.randn(B, 72) * 0.3), t(rs.randn(B, 10)), t(rs.randn(B, 3))
    gv = t(rs.randn(B, m.num_vertices, 3)) if mode == 'full' else None
    gj, go = t(rs.randn(B, 24, 3)), t(rs.randn(B, 24, 3, 3))
    torch.cuda.synchronize()
    for _ in range(TRACE_CALLS):
        m._backward_direct(pose, betas, trans, None, None, None, gj, go, gv)
    torch.cuda.synchronize()


def trace(B):
    """Per-kernel mean time (us) of one backward call, for both modes, from rocprofv3 kernel traces."""
    res = {}
    for mode in ('full', 'novert'):
        with tempfile.TemporaryDirectory() as d:
            cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', d, '-o', 't', '--', sys.executable,
                   os.path.abspath(__file__), '--one', mode, '--batches', str(B)]
            subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
            per = {}
            for f in glob.glob(f'{d}/**/*kernel_trace.csv', recursive=True):
                for r in csv.DictReader(open(f)):
                    name = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '')
                    name = re.split(r'[(<]', name)[0].strip()
                    dur = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
                    c, s = per.get(name, (0, 0.0))
                    per[name] = (c + 1, s + dur)
        rows = {k: dict(launches_per_call=c / TRACE_CALLS, us_per_call=round(s / TRACE_CALLS, 1))
                for k, (c, s) in sorted(per.items(), key=lambda kv: -kv[1][1])}
        print(json.dumps(dict(trace=mode, batch=B, kernels=rows)), flush=True)
        res[mode] = rows
    bad = [k for k in res['novert'] if k.startswith(VERTEX_KERNELS)]
    assert not bad, f'the backward without a vertex cotangent launched vertex-sized kernels: {bad}'
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,4096,16384')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--one', default=None)
    a = ap.parse_args()
    if a.one:
        return one_backward(a.one, int(a.batches))
    traced = trace(4096) if a.trace else None
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=('smpl', 'smplx'))
    rows = []
    for kind in ('smpl', 'smplx'):
        m = BodyModel(kind, 'neutral', model_root=f'{root}/{kind}', num_betas=10, device=dev)
        md = modelio.load_model(kind, 'neutral', model_root=f'{root}/{kind}', num_betas=10)
        m32 = grad_util.Model64(md, dtype=torch.float32)
        for name in ('v_template', 'shapedirs', 'posedirs', 'J_template', 'J_shapedirs', 'weights', 'kid_shapedir',
                     'kid_J_shapedir'):
            setattr(m32, name, getattr(m32, name).to(dev))
        for B in (int(b) for b in a.batches.split(',')):
            rs = np.random.RandomState(0)
            t = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)  # noqa: E731
            pose, betas, trans = t(rs.randn(B, 3 * m.num_joints) * 0.3), t(rs.randn(B, 10)), t(rs.randn(B, 3))
            cv, cj = t(rs.randn(B, m.num_vertices, 3)), t(rs.randn(B, m.num_joints, 3))
            ps = [x.clone().requires_grad_() for x in (pose, betas, trans)]

            def fwd():
                with torch.no_grad():
                    m(pose, betas, trans)

            def fwd_bwd(f=m):
                o = f(*ps)
                ((o['vertices'] * cv).sum() + (o['joints'] * cj).sum()).backward()

            legs = dict(forward=fwd, forward_backward=fwd_bwd,
                        torch_forward_backward=lambda: fwd_bwd(
                            lambda p, b, tr: grad_util.forward(m32, p, b, tr)))
            for leg, fn in legs.items():
                try:
                    with torch.device(dev):
                        med, best = timed(fn, a.steps, a.warmup)
                except torch.cuda.OutOfMemoryError:
                    torch.cuda.empty_cache()
                    r = dict(model=kind, leg=leg, batch=B, skipped='out of memory')
                    print(json.dumps(r), flush=True)
                    rows.append(r)
                    continue
                r = dict(model=kind, leg=leg, batch=B, median_ms=round(med, 4), min_ms=round(best, 4))
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows, backward_kernels_smpl_4096=traced), f,
                      indent=1)


if __name__ == '__main__':
    main()
