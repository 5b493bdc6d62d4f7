"""Helpers of the BodyFlipperOpt tests (tests/test_flipper_opt_host.py, tests/test_gpu_flipper_opt.py) and of the fixture
generator tests/golden/make_golden_flip_opt.py: the mirrored target and the refinement objective in the fp64 oracle."""

import numpy as np

CASES = ('it1', 'kid.it1')
STEPS = 100


def target64(om64, mirror, pose, betas, trans, kid):
    """The refinement's target in fp64: the oracle forward of the inputs (with kid_factor), mirrored, x negated."""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)  # noqa: E731
    v = om64.forward(pose_rotvecs=f64(pose), shape_betas=f64(betas), trans=f64(trans), kid_factor=f64(kid))['vertices']
    m = mirror.astype(np.float64)
    v = np.stack([m @ v[b] for b in range(v.shape[0])])
    v[..., 0] = -v[..., 0]
    return v


def objective64(om64, res, target):
    """Batch-mean vertex distance (m) between the fp64 oracle forward of a flip result and the target."""
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    v = om64.forward(f64(res['pose_rotvecs']), f64(res['shape_betas']), f64(res['trans']),
                     kid_factor=f64(res['kid_factor']))['vertices']
    return float(np.linalg.norm(np.asarray(v, np.float64) - target, axis=-1).mean())
