"""Time of BodyModel.rototranslate on one GPU: the fused call (smplfit_rototranslate_f32, one launch) against a batched
restatement of the reference's lines (pt/bodymodel.py:435-453) in PyTorch operations on the same GPU, forward and
forward + backward, with per-instance and with shared R, t, for the SMPL- and SMPL-X-shaped synthetic models at
B = 64, 4096, 32768 and 262144; at B = 64 also the reference's own usage pattern, a Python loop of unbatched calls of
that restatement.  The restatement lives here and is not the code under test.

Each row: the median and the minimum call time (HIP events around `inner` back-to-back calls, divided by `inner`), the
bytes the call has to move — B (2 * 3J + 9 + 3 + n + 3 + 3 + 1) * 4 for the forward (pose in and out, R, t, betas,
trans in and out, kid), less where R, t are shared; the backward reads the inputs and both cotangents and writes six
gradients — and that over the time as a fraction of the HBM rate HBM_TBS (the linear dwordx4 read rate of
profiles/r02_ubench_stream_read.txt; the write pattern of r02_ubench_stream_write.txt reached 6.1).  One JSON line per
row; --out FILE also writes them as one JSON list.

Usage:  python tools/bench_rototranslate.py [--steps 30] [--warmup 5] [--out profiles/rototranslate_mi355x.json]
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
from smplfitter_amd.pt import BodyModel  # noqa: E402

HBM_TBS = 6.3
BATCHES = (64, 4096, 32768, 262144)
NB = 10


def _div0(a, b):
    return torch.where(b == 0, torch.zeros_like(a), a / torch.where(b == 0, torch.ones_like(b), b))


def _rotvec2mat(rv):
    angle = torch.linalg.norm(rv, dim=-1, keepdim=True)
    ax = _div0(rv, angle)
    s, c = torch.sin(angle) * ax, torch.cos(angle)
    c1 = (1 - c) * ax
    xy, xz, yz = c1[..., 0] * ax[..., 1], c1[..., 0] * ax[..., 2], c1[..., 1] * ax[..., 2]
    d = c1 * ax + c
    m = torch.stack([d[..., 0], xy - s[..., 2], xz + s[..., 1], xy + s[..., 2], d[..., 1], yz - s[..., 0],
                     xz - s[..., 1], yz + s[..., 0], d[..., 2]], -1)
    return m.unflatten(-1, (3, 3))


def _mat2rotvec(M):
    r = M.flatten(-2, -1).unbind(-1)
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = r
    tr = r00 + r11 + r22
    q0 = torch.stack([r21 - r12, r02 - r20, r10 - r01, 1 + tr], -1)
    q1 = torch.stack([(1 - r22) + (r00 - r11), r10 + r01, r02 + r20, r21 - r12], -1)
    q2 = torch.stack([r10 + r01, (1 - r22) - (r00 - r11), r21 + r12, r02 - r20], -1)
    q3 = torch.stack([r02 + r20, r21 + r12, (1 + r22) - (r00 + r11), r10 - r01], -1)
    q = torch.where((tr > 0)[..., None], q0, torch.where(((r00 > r11) & (r00 > r22))[..., None], q1,
                                                         torch.where((r11 > r22)[..., None], q2, q3)))
    xyz, w = q[..., :3], q[..., 3:]
    n = torch.linalg.norm(xyz, dim=-1, keepdim=True)
    return _div0(torch.full_like(n, 2.0), n) * torch.atan2(n, w) * xyz


def restated(m, R, t, pose, betas, trans, kid, post=True):
    """The reference's lines on tensors with any leading batch shape (R / t shared: (3, 3) / (3,))."""
    new_pose = torch.cat([_mat2rotvec(R @ _rotvec2mat(pose[..., :3])), pose[..., 3:]], -1)
    pelvis = m.J_template[0] + betas @ m.J_shapedirs[0, :, :betas.shape[-1]].mT
    if kid is not None:
        pelvis = pelvis + m.kid_J_shapedir[0] * kid[..., None]
    eye = torch.eye(3, device=R.device)
    mv = lambda A, v: (A @ v[..., None])[..., 0]  # noqa: E731
    if post:
        return new_pose, mv(R, trans) + t + mv(R - eye, pelvis)
    return new_pose, mv(R, trans - t) + mv(R - eye, pelvis)


def timed(fn, steps, warmup, inner):
    """Median and minimum over `steps` timings of `inner` back-to-back calls (HIP events), per call, in ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batches', type=int, nargs='*', default=list(BATCHES))
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=('smpl', 'smplx'))
    rows = []
    for kind in ('smpl', 'smplx'):
        m = BodyModel(kind, 'neutral', model_root=f'{root}/{kind}', num_betas=NB, device=dev)
        J3 = 3 * m.num_joints
        for B in a.batches:
            rs = np.random.RandomState(0)
            t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)  # noqa: E731
            rv = rs.randn(B, 3) * 1.5
            ang = np.linalg.norm(rv, axis=-1, keepdims=True)
            K = np.zeros((B, 3, 3))
            ax = rv / ang
            K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
            K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
            Rn = np.eye(3) + np.sin(ang)[..., None] * K + (1 - np.cos(ang))[..., None] * (K @ K)
            R, t = t_(Rn), t_(rs.randn(B, 3))
            pose, betas, trans = t_(rs.randn(B, J3) * 0.4), t_(rs.randn(B, NB)), t_(rs.randn(B, 3))
            kid = t_(rs.uniform(-0.5, 1.5, B))
            cp, ct = t_(rs.randn(B, J3)), t_(rs.randn(B, 3))
            inner = 20 if B <= 4096 else 5
            for shared in (False, True):
                Rs, ts = (R[0].contiguous(), t[0].contiguous()) if shared else (R, t)
                ins = [Rs, ts, pose, betas, trans, kid]

                def fwd_bwd(f):
                    def run():
                        xs = [x.detach().requires_grad_() for x in ins]
                        p, tr = f(*xs)
                        torch.autograd.grad((p * cp).sum() + (tr * ct).sum(), xs)
                    return run

                fused = lambda *x: m.rototranslate(*x)  # noqa: E731
                rest = lambda *x: restated(m, *x)  # noqa: E731
                legs = dict(fused_fwd=lambda: fused(*ins), restated_fwd=lambda: rest(*ins),
                            fused_fwd_bwd=fwd_bwd(fused), restated_fwd_bwd=fwd_bwd(rest))
                if B == 64:
                    def loop():
                        for i in range(B):
                            restated(m, Rs if shared else R[i], ts if shared else t[i], pose[i], betas[i], trans[i], kid[i])
                    legs['restated_loop_fwd'] = loop
                rt = (9 + 3) * (1 if shared else B)
                fwd_bytes = 4 * (B * (2 * J3 + NB + 3 + 3 + 1) + rt)
                bwd_bytes = 4 * (B * (J3 + NB + 3 + 1) + rt + B * (J3 + 3) + B * (9 + 3 + J3 + NB + 3 + 1))
                for leg, fn in legs.items():
                    med, best = timed(fn, a.steps, a.warmup, 1 if leg == 'restated_loop_fwd' else inner)
                    nbytes = fwd_bytes + (bwd_bytes if leg.endswith('fwd_bwd') else 0)
                    r = dict(model=kind, leg=leg, batch=B, shared_R_t=shared, median_us=round(med * 1e3, 2),
                             min_us=round(best * 1e3, 2), bytes=nbytes,
                             hbm_fraction=round(nbytes / (med * 1e-3) / (HBM_TBS * 1e12), 4))
                    print(json.dumps(r), flush=True)
                    rows.append(r)
    by = {(r['model'], r['batch'], r['shared_R_t'], r['leg']): r['median_us'] for r in rows}
    slower = [k for k in by if k[3].startswith('fused') and by[k] > by[k[:3] + (k[3].replace('fused', 'restated'),)]]
    print(json.dumps(dict(fused_slower_than_restatement=slower)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), hbm_tbs=HBM_TBS, steps=a.steps, warmup=a.warmup,
                           rows=rows, fused_slower_than_restatement=slower), f, indent=1)


if __name__ == '__main__':
    main()
