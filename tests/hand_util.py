"""Helpers of the HandReplacer tests (tests/test_hand_replacer_host.py, tests/test_gpu_hand_replacer.py) and of the
fixture generator tests/golden/make_golden_hand_replacer.py: the synthetic files, the fp64 restatement of
``replace_hand`` on the oracle, and the gate against golden_hand_replacer.npz."""

import os

import numpy as np

import flip_util
import util

HAND_START, HAND_JOINTS = 22, 15
# The parity gate is the flip tests' (flip_util.MESH_GATE, max vertex L2 in metres), under the flip tests' margin rule:
# their fixture's own fp32-vs-fp64 floor (1.8e-5 m) is at most a fifth of the gate, so that the gate measures the code
# under test and not the reference's rounding.  check_floor() asserts the same of this fixture's recorded floor.
GATE = flip_util.MESH_GATE
FLOOR_MARGIN = 5.0


def check_floor(floor):
    assert FLOOR_MARGIN * float(floor) <= GATE, (float(floor), GATE)


def data_root():
    """The synthetic files HandReplacer reads (synth.write_hand_replacer_files), written when one of them is missing."""
    import os.path as osp

    from smplfitter_amd import synth

    root = os.getenv('SMPLFIT_SYNTH_DATA_HAND', '/tmp/smplfit_synth_data_hand_seed0')
    files = ('smplh16/neutral/model.npz', 'smplh16/kid_template.npy', 'smplx/MANO_SMPLX_vertex_ids.pkl',
             'smplx2smpl_deftrafo_setup.pkl')
    if not all(osp.exists(osp.join(root, 'body_models', f)) for f in files):
        synth.write_hand_replacer_files(root)
    return root


def load_md(root):
    from smplfitter_amd import modelio

    return modelio.load_model('smplh16', 'neutral', model_root=f'{root}/body_models/smplh16')


def replacement(hand_pose_source):
    """The 90 values copy_hand_params writes over the joints 22..51: the source's RIGHT hand mirrored, then as it is."""
    src = np.asarray(hand_pose_source)
    right = src[(HAND_START + HAND_JOINTS) * 3:(HAND_START + 2 * HAND_JOINTS) * 3]
    return np.concatenate([(right.reshape(-1, 3) * np.array([1, -1, -1], src.dtype)).reshape(-1), right])


def blend(verts, new, mix):
    return verts + (new - verts) * np.asarray(mix)[:, None]


def oracle_replace(om, verts, vertex_weights, mix, hand_pose_source):
    """replace_hand evaluated by the oracle in om's precision: fit (num_iter 3, no ridge, no final adjustment, the (V)
    weights for every instance), hand joints overwritten, forward, blend.  -> (vertices, parameters)"""
    dt = om.dtype
    v = np.asarray(verts, dt)
    vw = np.repeat(np.asarray(vertex_weights, dt).reshape(1, -1), v.shape[0], 0)
    r = util.O.OracleFitter(om).fit(v, vertex_weights=vw, num_iter=3, beta_regularizer=0.0, final_adjust_rots=False)
    pose = np.array(r['pose_rotvecs'], dt)
    pose[:, HAND_START * 3:] = replacement(np.asarray(hand_pose_source, dt))
    new = om.forward(pose_rotvecs=pose, shape_betas=r['shape_betas'], trans=r['trans'])['vertices']
    return blend(v, new, np.asarray(mix, dt)), dict(pose_rotvecs=pose, shape_betas=r['shape_betas'], trans=r['trans'])


def vertex_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64), axis=-1).max())
