"""Helpers of the BodyFlipper tests (tests/test_flipper_host.py, tests/test_gpu_flipper.py) and of the fixture
generator tests/golden/make_golden_flip.py: the fp64 flip of the oracle and the checks against golden_flip.npz."""

import os

import numpy as np

import util

# fixture model tags -> golden-set names of util.load_md (the SMPL-X side is the fat-part variant, as for the
# cross-topology BodyConverter fixture: the thin-finger one is ill-conditioned in the reference itself)
FLIP_MODELS = dict(smpl='smpl', smplx='smplxfat')
FLIP_CASES = ('it1', 'it3', 'kid.it1')
FLIP_KEYS = ('pose_rotvecs', 'shape_betas', 'trans', 'kid_factor')
MESH_GATE = 1e-4   # max vertex L2 (m) between the fp64 forwards of two results (util.check_convert's gate)
TRANS_GATE = 2e-5


def canonical_csr(m):
    """A scipy CSR matrix in canonical form (sorted indices, duplicates summed, no stored zeros) for util.csr_digest."""
    import scipy.sparse as sp

    m = sp.csr_matrix(m, copy=True)
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def case_args(case):
    """(num_iter, with kid_factor) of a fixture case."""
    return (3 if case == 'it3' else 1), case.startswith('kid')


def naive_flip(pose, perm):
    """naive_flip_rotvecs in numpy: joints reordered by the mirror map, rotation vectors times (1, -1, -1)."""
    B = pose.shape[0]
    return (np.asarray(pose).reshape(B, -1, 3)[:, np.asarray(perm)] * np.array([1, -1, -1], pose.dtype)).reshape(B, -1)


def oracle_flip(om, mirror, perm, pose, betas, trans, kid, num_iter):
    """BodyFlipper.flip evaluated by the oracle in om's precision: forward with kid_factor, mirror (x negated), fit with
    the kid unknown warm-started from the naive flip and the input betas, ridge 1e-2 / 1e-2, final adjustment, kid ridge
    1e9 without kid_factor else 0."""
    dt = om.dtype
    f = om.forward(pose_rotvecs=np.asarray(pose, dt), shape_betas=np.asarray(betas, dt), trans=np.asarray(trans, dt),
                   kid_factor=None if kid is None else np.asarray(kid, dt))
    m = mirror.astype(dt)
    v = np.stack([m @ f['vertices'][b] for b in range(f['vertices'].shape[0])])
    v[..., 0] = -v[..., 0]
    fitter = util.O.OracleFitter(om, enable_kid=True)
    r = fitter.fit(v, num_iter=num_iter, beta_regularizer=1e-2, beta_regularizer2=1e-2, final_adjust_rots=True,
                   kid_regularizer=1e9 if kid is None else 0.0, initial_pose_rotvecs=naive_flip(np.asarray(pose, dt), perm),
                   initial_shape_betas=np.asarray(betas, dt))
    return {k: r[k] for k in FLIP_KEYS}


def mesh_distance(om64, a, b):
    """max vertex L2 between the fp64 forwards of two flip results (each with its kid factor)."""
    va = om64.forward(a['pose_rotvecs'], a['shape_betas'], a['trans'], kid_factor=a['kid_factor'])['vertices']
    vb = om64.forward(b['pose_rotvecs'], b['shape_betas'], b['trans'], kid_factor=b['kid_factor'])['vertices']
    return float(np.linalg.norm(np.asarray(va, np.float64) - vb, axis=-1).max())


def check_flip(om64, tag, case, o, gf, gate=MESH_GATE):
    """One flip result against the reference's fixture: the result keys, max vertex L2 of the fp64 forwards, trans."""
    pre = f'{tag}.{case}.'
    assert set(o) == set(FLIP_KEYS), (tag, case, sorted(o))
    ref = {k: gf[pre + k] for k in FLIP_KEYS}
    err = mesh_distance(om64, o, ref)
    dtr = float(np.abs(np.asarray(o['trans']) - ref['trans']).max())
    if os.getenv('SMPLFIT_TEST_VERBOSE'):
        print(f'[flip] {tag} {case}: vertex L2 {err:.2e}, trans {dtr:.1e}')
    assert err <= gate, (tag, case, err)
    assert dtr <= TRANS_GATE, (tag, case, dtr)
    return err
