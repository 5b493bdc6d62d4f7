"""Time of one refinement step of BodyFitterOpt on one GPU, through the public API only:
(fit(refine_steps=N) - fit(refine_steps=0)) / N, both without the final rotation adjustment so that the closed-form
part cancels.  SMPL-shaped at B = 256 and 4096 and SMPL-X-shaped at B = 4096, each without and with target joints (and
joint weights).  Legs: `fused` — BodyFitterOpt(fused_objective=True), one objective-and-gradient call per step — and
`unfused` — fused_objective=False: BodyModel.forward under autograd, the loss in PyTorch operators, the HIP backward.
On a checkout whose BodyFitterOpt has no `fused_objective` argument (the commit before the fused objective) the only
leg is `unfused`, that commit's step: the same script measures the baseline there.  A window is one pair of fits between
HIP events, after a warm-up window of every leg; the legs alternate for `--rounds` rounds in one process, and the
median, minimum and maximum window are reported as ms per step.  One JSON line per measurement; --out FILE also writes
them as one JSON list.

Usage:  python tools/bench_fitter_opt.py [--steps 20] [--rounds 7] [--label this] [--out FILE]
"""
import argparse
import inspect
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from smplfitter_amd import synth  # noqa: E402
from smplfitter_amd.pt import BodyModel  # noqa: E402

try:
    from smplfitter_amd.pt import BodyFitterOpt  # noqa: E402
except ImportError:  # (not exported from the package yet)
    from smplfitter_amd.pt.bodyfitter_opt import BodyFitterOpt  # noqa: E402

SHAPES = (('smpl', 256), ('smpl', 4096), ('smplx', 4096))
FIT_KW = dict(num_iter=1, beta_regularizer=1e-3, final_adjust_rots=False)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def window(fo, args, kw, steps):
    """ms per refinement step: a fit with `steps` steps minus a fit with none."""
    full = timed(lambda: fo.fit(*args, refine_steps=steps, **kw, **FIT_KW))
    base = timed(lambda: fo.fit(*args, refine_steps=0, **kw, **FIT_KW))
    return (full - base) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--label', default='this', help='name of the checkout in the output rows')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=('smpl', 'smplx'))
    has_switch = 'fused_objective' in inspect.signature(BodyFitterOpt.__init__).parameters
    rows, models = [], {}
    for kind, B in SHAPES:
        if kind not in models:
            m = BodyModel(kind, 'neutral', model_root=f'{root}/{kind}', num_betas=10, device=dev)
            if has_switch:
                legs = dict(fused=BodyFitterOpt(m, fused_objective=True), unfused=BodyFitterOpt(m, fused_objective=False))
            else:
                legs = dict(unfused=BodyFitterOpt(m))
            models[kind] = (m, legs)
        m, legs = models[kind]
        rs = np.random.RandomState(0)
        t = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)  # noqa: E731
        with torch.no_grad():
            out = m(t(rs.randn(B, 3 * m.num_joints) * 0.5), t(rs.randn(B, 10)), t(rs.randn(B, 3)))
        tv = out['vertices'] + 0.005 * torch.randn_like(out['vertices'])
        tj = out['joints'] + 0.005 * torch.randn_like(out['joints'])
        jw = t(rs.uniform(0, 2, (B, m.num_joints)))
        del out
        for joints in (False, True):
            args, kw = ((tv, tj), dict(joint_weights=jw)) if joints else ((tv,), {})
            ms = {leg: [] for leg in legs}
            for leg, fo in legs.items():  # warm-up: every kernel and PyTorch operator of the shape
                window(fo, args, kw, a.steps)
            for _ in range(a.rounds):
                for leg, fo in legs.items():
                    ms[leg].append(window(fo, args, kw, a.steps))
            for leg, v in ms.items():
                r = dict(checkout=a.label, model=kind, batch=B, joints=joints, leg=leg, steps_per_window=a.steps,
                         windows=a.rounds, median_ms_per_step=round(statistics.median(v), 4),
                         min_ms_per_step=round(min(v), 4), max_ms_per_step=round(max(v), 4))
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
