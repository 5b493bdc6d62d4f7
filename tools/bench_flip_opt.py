"""Time of one refinement step of BodyFlipperOpt on one GPU: the fused objective call (smplfit_mesh_objective_f32 per
step) against the unfused step of the same build (BodyModel.forward under autograd, the loss in PyTorch operators, the
HIP backward), SMPL-shaped at B = 256 and 4096 and SMPL-X-shaped at B = 4096.  Both legs run the whole step (6D map,
objective and gradient, Adam).  A window is `--steps` refinement steps between two HIP events, after a warm-up window
of every leg; the legs alternate for `--rounds` rounds in one process, and the median, minimum and maximum window are
reported as ms per step.  One JSON line per measurement; --out FILE also writes them as one JSON list.

Usage:  python tools/bench_flip_opt.py [--steps 20] [--rounds 7] [--out profiles/flip_opt_mi355x.json]
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
from smplfitter_amd.pt import BodyFlipperOpt, BodyModel  # noqa: E402

SHAPES = (('smpl', 256), ('smpl', 4096), ('smplx', 4096))


def window(fl, target, init, steps):
    """ms per step of one refinement of `steps` steps (HIP events on the current stream)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fl._refine(target, init, steps, 0.03, 0.1)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=('smpl', 'smplx'))
    os.environ['DATA_ROOT'] = synth.write_transfer_files('/tmp/smplfit_bench_flip_data')
    rows, models = [], {}
    for kind, B in SHAPES:
        if kind not in models:
            m = BodyModel(kind, 'neutral', model_root=f'{root}/{kind}', num_betas=10, device=dev)
            fused = BodyFlipperOpt(m, fused_objective=True)
            unfused = BodyFlipperOpt(m, fused_objective=False)
            unfused.flipper = fused.flipper  # one mirror matrix
            models[kind] = (m, dict(fused=fused, unfused=unfused))
        m, legs = models[kind]
        rs = np.random.RandomState(0)
        t = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)  # noqa: E731
        pose, betas, trans = t(rs.randn(B, 3 * m.num_joints) * 0.3), t(rs.randn(B, 10)), t(rs.randn(B, 3))
        init = legs['fused'].flipper.flip(pose, betas, trans)
        target = legs['fused'].flipper.flip_vertices(m(pose, betas, trans)['vertices'])
        ms = {leg: [] for leg in legs}
        for leg, fl in legs.items():  # warm-up: every kernel and PyTorch operator of the shape
            window(fl, target, init, a.steps)
        for _ in range(a.rounds):
            for leg, fl in legs.items():
                ms[leg].append(window(fl, target, init, a.steps))
        for leg, v in ms.items():
            r = dict(model=kind, batch=B, leg=leg, steps_per_window=a.steps, windows=a.rounds,
                     median_ms_per_step=round(statistics.median(v), 4), min_ms_per_step=round(min(v), 4),
                     max_ms_per_step=round(max(v), 4))
            print(json.dumps(r), flush=True)
            rows.append(r)
        print(json.dumps(dict(model=kind, batch=B, fused_over_unfused=round(
            statistics.median(ms['fused']) / statistics.median(ms['unfused']), 4))), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
