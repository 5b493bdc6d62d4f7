"""Aligned mesh errors: ``BodyModel.mesh_error(align='similarity', align_on='each')``
(smplfit_mesh_error_aligned_f32), with and without ``return_mesh``, against the composition a caller wrote before it —
``forward``, fp32 centring, a batched 3 x 3 ``torch.linalg.svd`` with the determinant fix, the transform applied, the
norms and their means, for the vertices and for the joints — on the synthetic SMPL and SMPL-X models.  The two sides
of a pair run alternately, call by call; medians of ``--reps`` warmed calls, each ending in a device synchronise.
Row 2 of every batch lies ~1000 m from the origin: the largest deviation of both sides from the same arithmetic in fp64
on the same fp32 mesh is recorded for that row and for the others.

    python tools/bench_mesh_align.py [--models smpl smplx] [--batches 64 4096] [--reps 10] [--out profiles/mesh_align_mi355x.json]
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
from smplfitter_amd.pt import BodyModel  # noqa: E402
from smplfitter_amd.pt import align as A  # noqa: E402

FAR = 2


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


def naive_aligned_error(x, y):
    """What a caller composes in fp32: (errors (B, N), their row means) under the similarity Procrustes transform."""
    xm, ym = x.mean(1, keepdim=True), y.mean(1, keepdim=True)
    xc, yc = x - xm, y - ym
    K = yc.transpose(1, 2) @ xc
    U, S, Vh = torch.linalg.svd(K)
    d = torch.sign(torch.linalg.det(U @ Vh))
    D = torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1)
    R = (U * D[:, None, :]) @ Vh
    s = (S * D).sum(-1) / (xc * xc).sum((1, 2))
    t = ym[:, 0] - s[:, None] * (R @ xm[:, 0, :, None])[..., 0]
    e = torch.linalg.vector_norm(s[:, None, None] * (x @ R.transpose(1, 2)) + t[:, None] - y, dim=-1)
    return e, e.mean(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', nargs='+', default=['smpl', 'smplx'])
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 4096])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    root = synth.ensure_model_root(kinds=tuple(a.models))
    res = dict(device=torch.cuda.get_device_name(0), library=_lib.load().smplfit_version().decode(), reps=a.reps,
               align='similarity', align_on='each', far_row=FAR, models={})
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)  # noqa: E731
    for name in a.models:
        m = BodyModel(name, 'neutral', model_root=f'{root}/{name}', num_betas=10, device=dev)
        V, J, S = m.num_vertices, m.num_joints, m.num_betas
        out = dict(vertices=V, joints=J, kernel_path=m.kernel_path(), batches={})
        # (B, V, 3)-sized traffic per instance behind the forward's LBS pass, in bytes.  Native: the mesh written once; mesh
        # and targets read by the moments and again by the measuring kernel; the (B, V) errors written and read by the
        # row means.  Composition: the mesh written; mesh and targets read for the means; two centred copies written and
        # read for K and the spread; the mesh read and a moved copy written; moved and target read, the difference
        # written, read by the norm; the errors written and read by the mean.
        out['mesh_bytes_per_instance'] = dict(native=5 * V * 12 + 2 * V * 4, composition=12 * V * 12 + 2 * V * 4)
        rs = np.random.RandomState(0)
        for B in a.batches:
            trans = rs.randn(B, 3)
            trans[FAR] += (1000.0, -1000.0, 1000.0)
            p = dict(pose_rotvecs=t(rs.randn(B, 3 * J) * 0.1), shape_betas=t(rs.randn(B, S) * 0.5), trans=t(trans))
            fw = m(**p)
            tv = 1.2 * fw['vertices'] + t(rs.randn(B, 1, 3)) + t(rs.randn(B, V, 3) * 0.002)
            tj = 1.2 * fw['joints'] + t(rs.randn(B, 1, 3)) + t(rs.randn(B, J, 3) * 0.002)

            def composition():
                g = m(**p)
                ev, mv = naive_aligned_error(g['vertices'], tv)
                ej, mj = naive_aligned_error(g['joints'], tj)
                return dict(vertex_error=ev, joint_error=ej, mean_vertex_error=mv, mean_joint_error=mj, vertices=g['vertices'])

            native = lambda: m.mesh_error(tv, tj, align='similarity', **p)  # noqa: E731
            native_mesh = lambda: m.mesh_error(tv, tj, align='similarity', return_mesh=True, **p)  # noqa: E731
            r, c = native_mesh(), composition()
            assert torch.equal(r['vertices'], c['vertices'])
            # fp64 on the same fp32 mesh
            ref = A.aligned_errors(r['vertices'], tv, *A.procrustes(r['vertices'], tv, None, 'similarity'))
            others = torch.arange(B, device=dev) != FAR
            dev_of = lambda e: (float((e.double() - ref)[FAR].abs().max()), float((e.double() - ref)[others].abs().max()))  # noqa: E731
            comp_ms, native_ms = alternate(composition, native, a.reps)
            comp2_ms, native_mesh_ms = alternate(composition, native_mesh, a.reps)
            fwd_ms, plain_ms = alternate(lambda: m(**p), lambda: m.mesh_error(tv, tj, **p), a.reps)
            out['batches'][str(B)] = dict(
                composition_ms=comp_ms, native_ms=native_ms, ratio=comp_ms / native_ms, composition_again_ms=comp2_ms,
                native_with_mesh_ms=native_mesh_ms, ratio_with_mesh=comp2_ms / native_mesh_ms, forward_ms=fwd_ms,
                mesh_error_unaligned_ms=plain_ms,
                composition_vs_fp64_far_row_m=dev_of(c['vertex_error'])[0], composition_vs_fp64_other_rows_m=dev_of(c['vertex_error'])[1],
                native_vs_fp64_far_row_m=dev_of(r['vertex_error'])[0], native_vs_fp64_other_rows_m=dev_of(r['vertex_error'])[1])
            print(name, B, json.dumps(out['batches'][str(B)]), flush=True)
        res['models'][name] = out
    print(json.dumps(res))
    if a.out:
        os.makedirs(osp.dirname(osp.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
