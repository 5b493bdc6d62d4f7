"""CPU: what tests/test_gpu_general_shapes.py relies on without a GPU — the launch rules of the general path as
general_util.launch_rules restates them, pinned at the thresholds kernels_gen.inc states, with the sweep's counts on both
sides of every switch; and the share of (instance, part) pairs the fp64 oracle alone puts under a distance gate on every
(model, family) of the stage harness, so that a change of inputs cannot quietly empty a gate of check_rotations."""

import pytest

import general_util as G
import stage_util as S

SWITCHES = ('accum_threads', 'accum_tile', 'accum_staged', 'mfma_waves', 'mfma_blocks_per_wave', 'mfma_groups', 'mfma_staged')


def test_launch_rules_at_the_stated_thresholds():
    r = lambda n, J=24, B=1: G.launch_rules(n, J, B)  # noqa: E731
    assert (r(88)['accum_threads'], r(89)['accum_threads']) == (64, 256)
    assert (r(128)['accum_tile'], r(129)['accum_tile']) == (32, 8)
    assert [r(n)['accum_passes'] for n in (176, 177, 252, 253)] == [1, 2, 2, 3]
    shape = lambda n: (r(n)['mfma_nb'], r(n)['mfma_waves'], r(n)['mfma_blocks_per_wave'])  # noqa: E731
    assert [shape(n) for n in (27, 28, 59, 60, 155, 156)] == [(1, 4, 1), (2, 4, 1), (2, 4, 1), (3, 16, 1), (5, 16, 1), (6, 8, 7)]
    assert (r(315)['mfma_groups'], r(316)['mfma_groups']) == (1, 2)
    assert [r(n)['mfma_extra'] for n in (26, 27, 28, 31, 32)] == ['inside', 'fill', 'straddle', 'straddle', 'inside']
    # the joint rows: SMPL at 300 staged, the 55-joint model not (201 KB)
    assert r(300)['mfma_staged'] and not r(300, 55)['mfma_staged'] and 55 * G._jd_stride(300) * 4 == 201520
    # k_gen_lbs: four instances per workgroup from S = 48 and B = 2048; above 64 KB of LDS on 55 joints only
    assert [r(n, 24, B)['lbs_ni'] for n, B in ((47, 2048), (48, 2047), (48, 2048))] == [1, 1, 4]
    assert r(64, 55, 2049)['lbs_lds'] == 67968 and r(48, 55, 2049)['lbs_lds'] == 67712 and r(48, 24, 2048)['lbs_lds'] < 65536
    assert all(r(n)['mfma_blocks_covered'] and r(n, 55)['mfma_blocks_covered'] for n in range(17, 1024))


def test_sweep_reaches_both_sides_of_every_switch():
    """Every count from 18 to 401 at which a launch rule of the SMPL skeleton changes has itself and its predecessor
    among the sweep's unknown counts (a count, or a count + the kid unknown); so have the 1 | 2 | 3 passes of
    k_gen_accum, and the three placements of the extra columns on each of the three workgroup shapes."""
    reached = set(G.SWEEP) | {n + 1 for n in G.SWEEP}
    assert set(G.SWEEP_LISTED) <= set(G.SWEEP) and max(reached) == 401
    for n in range(18, 402):
        a, b = G.launch_rules(n - 1, 24), G.launch_rules(n, 24)
        flips = [k for k in SWITCHES if a[k] != b[k]]
        assert not flips or {n - 1, n} <= reached, (n, flips)
    assert {176, 177, 252, 253} <= reached
    placed = {(G.launch_rules(n, 24)['mfma_waves'], G.launch_rules(n, 24)['mfma_extra']) for n in reached}
    assert placed == {(w, e) for w in (4, 16, 8) for e in ('inside', 'fill', 'straddle')}
    assert any(G.launch_rules(n, 24)['mfma_idle_waves'] for n in reached if G.launch_rules(n, 24)['mfma_groups'] == 2)


@pytest.fixture(scope='module')
def groot(model_root):
    from smplfitter_amd import synth

    return synth.ensure_model_root(root=model_root, kinds=('smplx_fat_b300',))


@pytest.mark.parametrize('name,nb', list(G.STAGE_MODELS))
def test_oracle_gated_share(name, nb, groot):
    """check_rotations asks for 90 % of the pairs of an unmasked family under a distance gate; the fp64 oracle alone
    gives 1.000 on 'pose1' and 'betas5' (also at 64 and 300 unknowns: the +-5 mesh stays one the rotation pass can be
    judged on), 0.991 .. 1.000 on 'mirror', 0.955 (SMPL) / 0.981 (SMPL-X-shaped) on the masked 'part_off'."""
    c = G.setup(groot, name, nb)
    for family in G.STAGE_MODELS[name, nb]:
        share = G.oracle_gated_share(c, family)
        print(f'[gated share] {name} nb={nb} {family}: {share:.3f}')
        assert share >= S.MIN_GATED, (name, nb, family, share)
        if family in ('pose1', 'betas5'):
            assert share == 1.0, (name, nb, family, share)
