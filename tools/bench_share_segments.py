"""share_beta over segments of the batch: many tracks in one call against a loop of share_beta calls.

4096 rows of the SMPL-shaped model with joints, num_iter 3, every track one body in its own poses (+3 mm noise).  Per
layout of tracks — 64 x 64, 128 x 32 and a seeded uneven one of 24 tracks — the legs

    whole     fit(share_beta=True) on all 4096 rows (one shape: the work of a segmented call, without the tables)
    loop      one fit(rows of the track, share_beta=True) per track
    segments  fit(share_beta_segments=sizes)            (when the checkout has it)
    single    fit(share_beta_segments=[4096])           (when the checkout has it)

are medians of warmed calls, each ending in a device synchronise.  `whole` and `loop` use only the API of the commit
before the feature, so the same file measures a checkout of that commit: `--parent DIR` (a built checkout of it) runs
parent and new alternately, `--rounds` times each, one child process per run, and reports the medians over the rounds
with the ratios  single / parent's whole  and  parent's loop / segments.

    python tools/bench_share_segments.py [--parent DIR] [--rounds 3] [--reps 10] [--out profiles/share_segments_mi355x.json]
"""

import argparse
import inspect
import json
import os
import os.path as osp
import subprocess
import sys
import time

import numpy as np

HERE = osp.dirname(osp.dirname(osp.abspath(__file__)))
ROWS = 4096


def layouts():
    rs = np.random.RandomState(0)
    cuts = np.sort(rs.choice(np.arange(1, ROWS), 23, replace=False))
    uneven = np.diff(np.concatenate([[0], cuts, [ROWS]])).tolist()
    return {'64x64': [64] * 64, '128x32': [32] * 128, 'uneven24': uneven}


def measure(root, reps):
    """The legs on the checkout at ``root``, as a dict (run in a process of its own)."""
    sys.path.insert(0, root)
    import torch

    from smplfitter_amd import _lib, synth
    from smplfitter_amd.pt import BodyFitter, BodyModel

    def median_ms(fn, warm=3):
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

    dev = torch.device('cuda:0')
    mroot = synth.ensure_model_root(kinds=('smpl',), seed=0)
    m = BodyModel('smpl', 'neutral', model_root=f'{mroot}/smpl', num_betas=10, device=dev)
    f = BodyFitter(m)
    have = 'share_beta_segments' in inspect.signature(f.fit).parameters
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)  # noqa: E731
    kw = dict(num_iter=3)
    res = dict(library=_lib.load().smplfit_version().decode(), has_segments=have, layouts={})
    for name, sizes in layouts().items():
        rs = np.random.RandomState(len(sizes))
        betas = np.repeat(rs.randn(len(sizes), 10) * 0.5, sizes, 0)
        with torch.no_grad():
            fw = m(t(rs.randn(ROWS, 3 * m.num_joints) * 0.1), t(betas), t(rs.randn(ROWS, 3)))
            tv = fw['vertices'] + torch.randn(fw['vertices'].shape, generator=torch.Generator().manual_seed(1)).to(dev) * 0.003
            tj = fw['joints']
        starts = np.concatenate([[0], np.cumsum(sizes)]).tolist()

        def loop():
            return [f.fit(tv[a:b], tj[a:b], share_beta=True, **kw) for a, b in zip(starts[:-1], starts[1:])]

        row = dict(tracks=len(sizes), whole_ms=median_ms(lambda: f.fit(tv, tj, share_beta=True, **kw)), loop_ms=median_ms(loop))
        if have:
            row['segments_ms'] = median_ms(lambda: f.fit(tv, tj, share_beta_segments=sizes, **kw))
            row['single_ms'] = median_ms(lambda: f.fit(tv, tj, share_beta_segments=[ROWS], **kw))
        res['layouts'][name] = row
    res['device'] = torch.cuda.get_device_name(0)
    return res


def child(root, reps):
    out = subprocess.run([sys.executable, osp.abspath(__file__), '--leg', root, '--reps', str(reps)], capture_output=True, text=True,
                         timeout=300)
    if out.returncode != 0:
        raise SystemExit(f'measuring {root} failed ({out.returncode}):\n{out.stdout}\n{out.stderr}')
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the commit before the feature')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(measure(a.leg, a.reps)))
        return
    runs = dict(new=[], parent=[])
    for _ in range(a.rounds):  # parent and new alternately
        if a.parent:
            runs['parent'].append(child(osp.abspath(a.parent), a.reps))
        runs['new'].append(child(HERE, a.reps))
        print(json.dumps({k: v[-1]['layouts'] for k, v in runs.items() if v}), flush=True)
    res = dict(device=runs['new'][0]['device'], rows=ROWS, num_iter=3, reps=a.reps, rounds=a.rounds, layouts={})
    for side, rr in runs.items():
        if rr:
            res[f'{side}_library'] = rr[0]['library']
    for name, sizes in layouts().items():
        row = dict(tracks=len(sizes), largest_track=max(sizes), smallest_track=min(sizes))
        for side, rr in runs.items():
            for key in ('whole_ms', 'loop_ms', 'segments_ms', 'single_ms'):
                vals = [r['layouts'][name][key] for r in rr if key in r['layouts'][name]]
                if vals:
                    row[f'{side}.{key}'] = float(np.median(vals))
                    row[f'{side}.{key}.rounds'] = vals
        base = 'parent' if a.parent else 'new'
        row['single_over_whole'] = row['new.single_ms'] / row[f'{base}.whole_ms']
        row['loop_over_segments'] = row[f'{base}.loop_ms'] / row['new.segments_ms']
        res['layouts'][name] = row
    res['baseline'] = 'parent checkout' if a.parent else 'the same checkout'
    print(json.dumps(res))
    if a.out:
        os.makedirs(osp.dirname(osp.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
