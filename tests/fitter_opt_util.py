"""Helpers of the BodyFitterOpt tests (tests/test_fitter_opt_host.py, tests/test_gpu_fit_objective.py) and of the fixture
generator tests/golden/make_golden_fitter_opt.py: the noisy targets rebuilt from the fixture's parameters and the
refinement objective in the fp64 oracle."""

import numpy as np

CASES = ('v', 'vj', 'kid.v', 'kid.vj')  # vertices only | vertices and weighted joints, without | with enable_kid
STEPS = 100
FIT_KW = dict(num_iter=1, beta_regularizer=1e-3)
NOISE_M = 0.005  # sigma of the Gaussian noise on target vertices and joints
NOISE_SEED = 7


def case_args(case):
    """(target joints and joint weights given, enable_kid) of a fixture case."""
    return case.endswith('vj'), case.startswith('kid.')


def targets(om64, g):
    """(target_vertices, target_joints) of the fixture, fp32: the fp64 oracle forward of the stored parameters rounded to
    fp32, plus seeded Gaussian noise of NOISE_M (the fixture stores parameters only)."""
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    f = om64.forward(f64(g['pose']), f64(g['betas']), f64(g['trans']))
    rs = np.random.RandomState(NOISE_SEED)
    tv = f['vertices'].astype(np.float32) + (rs.randn(*f['vertices'].shape) * NOISE_M).astype(np.float32)
    tj = f['joints'].astype(np.float32) + (rs.randn(*f['joints'].shape) * NOISE_M).astype(np.float32)
    return tv, tj


def objective64(om64, res, tv, tj=None, jw=None):
    """The refinement's objective without the ridge (m): the mean vertex distance, plus the mean of joint_weights times
    the joint distance when target joints are given; the result's mesh by the fp64 oracle forward."""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)  # noqa: E731
    f = om64.forward(f64(res['pose_rotvecs']), f64(res['shape_betas']), f64(res['trans']),
                     kid_factor=f64(res.get('kid_factor')))
    obj = np.linalg.norm(f['vertices'] - f64(tv), axis=-1).mean()
    if tj is not None:
        d = np.linalg.norm(f['joints'] - f64(tj), axis=-1)
        obj += (d if jw is None else f64(jw) * d).mean()
    return float(obj)
