"""HandReplacer without a GPU: the public name, the constants the class derives from the synthetic files against the
reference's fixture (tests/golden/make_golden_hand_replacer.py), its helpers, the fp64 restatement against the fixture's
result, the new C symbols and the host-side checks of the plan."""

import ctypes as C

import numpy as np
import pytest
import torch

import hand_util


@pytest.fixture(scope='module')
def gh(golden):
    return golden('hand_replacer')


@pytest.fixture(scope='module')
def hand_root():
    return hand_util.data_root()


@pytest.fixture(scope='module')
def replacer(gh, hand_root):
    from smplfitter_amd.pt import HandReplacer

    return HandReplacer(torch.from_numpy(gh['hand_pose_source']), model_root=f'{hand_root}/body_models/smplh16',
                        data_root=hand_root)


def test_handreplacer_exported():
    import smplfitter_amd.pt as pt

    assert 'HandReplacer' in pt.__all__
    from smplfitter_amd.pt import HandReplacer  # noqa: F401


def test_synthetic_smplh_shape(hand_root):
    from smplfitter_amd import synth

    md = hand_util.load_md(hand_root)
    assert (md.num_vertices, md.num_joints, md.shapedirs.shape[2]) == (6890, 52, 16)
    assert md.kintree_parents == [-1] + synth.SMPLH_PARENTS[1:]
    assert md.kintree_parents[22] == 20 and md.kintree_parents[37] == 21 and md.kintree_parents[51] == 50


def test_constants_match_reference(replacer, gh):
    """hand_indices_all and vertex_weights exactly; hand_mix_weight to the rounding of the fp32 rest mesh: the reference
    takes it from a full fp32 forward, the class from the rest-pose identity, so |x| and hand_min_x each differ by a few
    ulps of a coordinate in [0.5, 1) (6e-8 m; 4 ulps = 2.5e-7 m), and the smootherstep's slope is at most
    1.875 / 0.1 per metre: 18.75 * 2 * 2.5e-7 = 1e-5."""
    np.testing.assert_array_equal(replacer.hand_indices_all.numpy(), gh['hand_indices_all'])
    np.testing.assert_array_equal(replacer.vertex_weights.numpy(), gh['vertex_weights'])
    assert replacer.vertex_weights.shape == (1, 6890) and replacer.hand_mix_weight.shape == (6890,)
    mix = replacer.hand_mix_weight.numpy()
    assert np.abs(mix - gh['hand_mix_weight']).max() <= 1e-5
    np.testing.assert_array_equal(mix == 0, gh['hand_mix_weight'] == 0)
    assert (mix == 0).sum() > 3445 and (mix == 1).sum() > 0 and ((mix > 0) & (mix < 1)).sum() > 0
    assert (mix[gh['hand_indices_all']] == 1).all()


def test_default_roots(gh, hand_root, monkeypatch):
    from smplfitter_amd.pt import HandReplacer

    monkeypatch.setenv('DATA_ROOT', hand_root)
    monkeypatch.delenv('SMPLFITTER_BODY_MODELS', raising=False)
    hr = HandReplacer(torch.from_numpy(gh['hand_pose_source']))
    np.testing.assert_array_equal(hr.hand_indices_all.numpy(), gh['hand_indices_all'])
    assert hr.smplh_bm.num_betas == 16
    with pytest.raises(ValueError):
        HandReplacer(torch.zeros(24 * 3))


def test_helpers_match_reference(replacer, gh):
    out = replacer.mirror_rotvecs(torch.from_numpy(gh['mirror_in'])).numpy()
    np.testing.assert_array_equal(out, gh['mirror_out'])
    pose = torch.from_numpy(gh['copy_in'].copy())
    assert replacer.copy_hand_params(pose) is None
    np.testing.assert_array_equal(pose.numpy(), gh['copy_out'])
    # both hands from the source's RIGHT-hand block: left = right mirrored
    src = gh['hand_pose_source']
    right = src[37 * 3:52 * 3]
    np.testing.assert_array_equal(pose.numpy()[0, 37 * 3:], right)
    np.testing.assert_array_equal(pose.numpy()[0, 22 * 3:37 * 3], (right.reshape(-1, 3) * [1, -1, -1]).reshape(-1).astype(np.float32))
    np.testing.assert_array_equal(pose.numpy()[:, :66], gh['copy_in'][:, :66])
    np.testing.assert_array_equal(replacer.replacement_rotvecs().numpy(), hand_util.replacement(src))


def test_input_checks_need_no_device(replacer):
    with pytest.raises(ValueError):
        replacer.replace_hand(torch.zeros(2, 100, 3))
    with pytest.raises(NotImplementedError):
        replacer.replace_hand(torch.zeros(2, 6890, 3, requires_grad=True))


def test_oracle_replace_matches_fixture(gh, hand_root):
    """The fp64 restatement (weighted fit, hand joints overwritten, forward, blend) reproduces the reference's result
    within the floor the fixture recorded, which leaves the gate its margin; mix == 0 vertices are the input."""
    import util

    om64 = util.O.OracleModel(hand_util.load_md(hand_root), np.float64, 'smplh16')
    o, _ = hand_util.oracle_replace(om64, gh['verts'], gh['vertex_weights'], gh['hand_mix_weight'].astype(np.float64),
                                    gh['hand_pose_source'])
    floor = float(gh['fp32_vs_fp64'])
    hand_util.check_floor(floor)
    assert hand_util.vertex_l2(o[:, gh['out_idx']], gh['out_vertices_sub']) <= max(2 * floor, 1e-5)
    zero = gh['hand_mix_weight'] == 0
    np.testing.assert_array_equal(o[:, zero].astype(np.float32), gh['verts'][:, zero])


def test_symbols_exported():
    from smplfitter_amd import _lib

    lib = _lib.load()
    for name in ('smplfit_replace_hands_plan_create', 'smplfit_replace_hands_plan_destroy',
                 'smplfit_replace_hands_workspace_bytes', 'smplfit_replace_hands_f32'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_plan_validation_host_only(hand_root):
    """smplfit_replace_hands_plan_create checks the vector lengths and the joint range before it needs a device."""
    from smplfitter_amd import _lib

    md = hand_util.load_md(hand_root)
    desc, keep = _lib.make_desc(md.v_template, md.shapedirs, md.posedirs, md.weights, md.J_template, md.J_shapedirs,
                                md.kintree_parents, md.J_regressor_post_lbs)
    h = _lib.Handle(desc, host_only=True)
    V, J = md.num_vertices, md.num_joints
    lib = _lib.load()
    w = np.ones(V + 1, np.float32)
    rv = np.zeros(3 * J + 3, np.float32)
    fp = lambda a: a.ctypes.data_as(_lib._fp)  # noqa: E731

    def create(nv, j0, n, nrv, weights=w):
        p = C.c_void_p()
        rc = lib.smplfit_replace_hands_plan_create(h.ptr, fp(weights), fp(w), nv, j0, n, fp(rv), nrv, C.byref(p))
        assert not p.value
        return rc

    for bad in ((V - 1, 22, 30, 90), (V + 1, 22, 30, 90),      # weight vectors of the wrong length
                (V, 22, 30, 89), (V, 22, 30, 93), (V, 22, 30, 30),  # rotation vectors of the wrong length
                (V, 23, 30, 90), (V, -1, 2, 6), (V, J, 1, 3), (V, 0, J + 1, 3 * J + 3), (V, 5, 0, 0),
                (V, 2**31 - 1, 2, 6)):
        assert create(*bad) == _lib.SMPLFIT_ERR_BAD_ARG, bad
    p = C.c_void_p()
    assert lib.smplfit_replace_hands_plan_create(h.ptr, None, fp(w), V, 22, 30, fp(rv), 90, C.byref(p)) == _lib.SMPLFIT_ERR_BAD_ARG
    assert create(V, 22, 30, 90) == _lib.SMPLFIT_ERR_HIP  # valid arguments: a host-only handle has no device
    assert create(V, 0, J, 3 * J) == _lib.SMPLFIT_ERR_HIP
    assert lib.smplfit_replace_hands_workspace_bytes(None, 8) == 0
    with pytest.raises(ValueError):
        _lib.ReplaceHandsPlan(h, w[:V], w[:V], 40, 30, rv[:90])
    del keep
