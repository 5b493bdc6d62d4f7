"""The scaled-fit stage chain of tests/scale_chain_util.py with the host emulation (hostemu_util.fit_warm: the product's
stage code of sf_stages.h compiled for the CPU, which mirrors k_scale_extras + k_shape_solve_scaled and k_scale_refs)
standing in for the device, B = 8; fit_with_known_pose (SS0), which the emulation does not have, and the model with 32
betas, for which it has no instance, by the fp32 oracle's own entry points.  It pins what the GPU test rests on:

* the references and the criteria are reachable in fp32 on every (model, case, option) the GPU test runs;
* the floor cap: on every kept case the fp32 oracle's own distance from the fp64 one stays within
  scale_chain_util.FLOOR_CAP x the fixed gate on every row (check_solve(cap=True)); 'betas5' without a ridge is outside
  it (test_betas5_needs_the_ridge: its figures) and is therefore run under the ridge only;
* the share exemptions of the rotation steps (scale_chain_util.SHARE_EXEMPT), measured;
* the oracle's weight rules for the scaled solve (test_scaled_solve_weight_rules);
* the identities of the chain on the emulation: A and D return the same first pass, B keeps A's solve.

'mirror' misses distance gates here as it does in the unscaled chains (tests/test_known_shape_chain_host.py: the hands 22 /
23, the ankles 7 / 8 and the fingers of the fat-part SMPL-X have gaps / kappa of 0.01 .. 0.07 under the reflected target;
two fp32 evaluations of such a pair scatter by more than a factor of two).  HOST_MISS lists the steps per (model, option);
figures, emulation against the fp32 oracle on that pair (gate 5e-4, 2e-3 on smplxfat): smpl F (6, 7) 1.39e-3 / 3.3e-4,
with scale_fit (4, 7) 1.21e-3 / 4.7e-4; smplxfat R1 (1, 33) 2.26e-3 / 9.7e-4, R2 (4, 38) 2.49e-3 / 1.02e-3, F with
scale_fit (7, 8) 2.61e-3 / 1.02e-3; smpl_w6 R1 (2, 22) 6.3e-4 / 2.9e-4, F (4, 7) 1.04e-3 / 3.9e-4, R2 (6, 22) 1.61e-3 /
6.4e-4; smpl_kid R2 (0, 23) 1.58e-3 / 2.9e-4, F with scale_fit (3, 7) 8.6e-4 / 2.3e-4; smpl_b16 R2 (5, 23) 1.86e-3 /
8.7e-4, F with scale_fit (1, 7) 5.3e-4 / 6.0e-6; smpl_b16_kid F with scale_fit (3, 7) 5.2e-4 / 1.8e-4.  Every deficit of
these steps is <= 7e-7: the rotations are optima of the fp64 covariance to rounding.  The steps are deferred and raised by
test_known_miss, expected to fail, strictly; every other gate of the 'mirror' case, and every gate of every other case,
holds — and test_chain_hostemu fails when a step not listed misses or a listed one no longer does."""

import numpy as np
import pytest

import hostemu_util as H
import scale_chain_util as X
import stage_util as S

FULL = X.FULL
FEW = ('smpl_kid', 'smpl_w6', 'smpl_b16', 'smpl_b16_kid')     # the wave-only instantiations
# 'mirror': the rotation steps whose distance gate misses on a loose pair (module docstring)
HOST_MISS = {('smpl', 'scale_target'): ('F',), ('smpl', 'scale_fit'): ('F',),
             ('smplxfat', 'scale_target'): ('R1', 'R2'), ('smplxfat', 'scale_fit'): ('R1', 'F', 'R2'),
             ('smpl_w6', 'scale_target'): ('R1', 'F', 'R2'), ('smpl_w6', 'scale_fit'): ('R1', 'F', 'R2'),
             ('smpl_kid', 'scale_target'): ('R2',), ('smpl_kid', 'scale_fit'): ('F', 'R2'),
             ('smpl_b16', 'scale_target'): ('R2',), ('smpl_b16', 'scale_fit'): ('F', 'R2'),
             ('smpl_b16_kid', 'scale_fit'): ('F',)}
MIRROR_LOOSE = pytest.mark.xfail(strict=True, reason="'mirror': hands and ankles with gap / kappa of 0.01 .. 0.07 scatter by more "
                                                     'than 2 x the fp32 oracle on that pair (module docstring)')
_checked = {}


def model_cases(name):
    """The cases of the GPU test; on the fat-part SMPL-X, whose oracle is three times the work, every unmasked family, one
    case of each weight setting and the two without target joints (the GPU test asserts the floor cap on all of them)."""
    keep = S.UNMASKED + ('part_off-j_reg1_w=vj', 'mask01-j_reg1_w=v', 'joint_off-j_reg1_w=j')
    return [k for k in X.cases(name) if name != 'smplxfat' or not k.joints or k.id in keep or (k.family in keep and not k.weights and not k.warm and not k.scale_reg)]


def chain(name, case, mode, model_root, golden):
    """check_chain's figures of one (model, case, option), computed once."""
    key = (name, case.id, mode)
    if key not in _checked:
        c = X.host_setup(name, model_root, golden)
        case = X.bound(c, case)
        outs = X.host_chain(c, name, case, mode, H)
        outs['SS0'] = X.known_pose_oracle(c, name, case, mode)
        defer = ('R1', 'F', 'R2') if case.family == 'mirror' else ()
        _checked[key] = X.check_chain(name, c, case, mode, outs, f'hostemu {"st" if mode == 1 else "sf"}', defer=defer)
    return _checked[key]


@pytest.mark.parametrize('mode', X.MODES)
@pytest.mark.parametrize('name', FULL + FEW)
def test_chain_hostemu(name, mode, model_root, golden, capsys):
    """Every case of the model through SS0, A, B, C and D; prints each step's figures, then the lowest gated share per
    (family, step), which must be under the cap exactly where SHARE_EXEMPT says."""
    seen = {}
    with capsys.disabled():
        print()
        for case in model_cases(name):
            for k, v in X.gated_shares(name, case, chain(name, case, X.MODES[mode], model_root, golden)).items():
                seen[k] = min(seen.get(k, 1.0), v)
        print(f'[gated shares {name} {mode}] ' + ' '.join(f'{f}/{s} {v:.4f}' for (_, f, s), v in seen.items()))
        for case in model_cases(name):
            d = chain(name, case, X.MODES[mode], model_root, golden)['deferred']
            if d:
                print(f'[deferred {name} {mode} {case.id}] ' + ' | '.join(f'{k}: {str(e)[:300]}' for k, e in d.items()))
        missed = {case.id: tuple(chain(name, case, X.MODES[mode], model_root, golden)['deferred']) for case in model_cases(name)}
    assert {k: v for k, v in missed.items() if v} == ({'mirror-' + X.Case('mirror', reg=X.ridge(name, 'mirror')).tag.replace(' ', '_'): HOST_MISS[name, mode]}
                                                      if HOST_MISS.get((name, mode)) else {}), missed
    low = {k: v for k, v in seen.items() if k[1] in S.UNMASKED and v < S.MIN_GATED}
    listed = {k: v for k, v in X.SHARE_EXEMPT.items() if k[0] == name}
    assert set(low) == set(listed) and all(abs(low[k] - listed[k][X.MODES[mode] - 1]) < 5e-3 for k in low), (low, listed)


@pytest.mark.parametrize('mode', X.MODES)
def test_general_path_fp32_oracle(mode, model_root, golden, capsys):
    """smpl_b32 (33 / 34 unknowns: the general k_shape_solve_scaled<true>; no instance in the emulation): the chain with
    the fp32 oracle's entry points standing in."""
    c = X.host_setup('smpl_b32', model_root, golden)
    case = X.Case('pose1')
    with capsys.disabled():
        print()
        X.check_chain('smpl_b32', c, case, X.MODES[mode], X.oracle_chain(c, 'smpl_b32', case, X.MODES[mode]), f'fp32 oracle {mode}')


@pytest.mark.parametrize('mode', X.MODES)
def test_betas5_needs_the_ridge(mode, model_root, golden, capsys):
    """'betas5' with beta_regularizer 0: the fp32 oracle's own scaled solve at the fp64 first pass is outside the floor
    cap (scale_corr > 1e-4 or betas > 3e-3 or mesh > 1e-3 on some row), with the ridge inside — so the chain keeps the
    ridged case alone.  (figures: DESIGN.md §5)"""
    c = X.host_setup('smpl', model_root, golden)
    figs = {}
    for reg in (0.0, 1.0):
        case = X.Case('betas5', reg=reg)
        r64, r32 = X.refs(c, 'smpl', case)
        G = r64.R1()[0].astype(np.float32)
        a64, a32 = r64.solve(G, X.MODES[mode]), r32.solve(G, X.MODES[mode])
        figs[reg] = dict(scale=np.abs(a32['scale_corr'] - a64['scale_corr']).max(),
                         betas=np.abs(a32['shape_betas'] - a64['shape_betas']).max(),
                         mesh=np.linalg.norm((a32['vertices'] - a32['trans'][:, None]) - (a64['vertices'] - a64['trans'][:, None]), axis=-1).max())
    with capsys.disabled():
        print(f'\n[betas5 {mode}] ' + '  '.join(f'reg{r:g}: ' + ' '.join(f'{k} {v:.2e}' for k, v in f.items()) for r, f in figs.items()))
    gates = dict(scale=X.SCALE_GATE, betas=S.BETA_GATE, mesh=S.MESH_GATE)
    assert any(figs[0.0][k] > X.FLOOR_CAP * g for k, g in gates.items()), figs[0.0]
    assert all(figs[1.0][k] <= X.FLOOR_CAP * g for k, g in gates.items()), figs[1.0]


@pytest.mark.parametrize('mode', X.MODES)
def test_scaled_solve_weight_rules(mode, model_root, golden):
    """What the oracle's scaled solve takes as weights (the facts the cases 'v' and 'j' rest on): with target joints,
    vertex weights alone or joint weights alone leave it UNWEIGHTED, both weight it; without target joints the vertex
    weights do enter — and on 'mask01' each of these moves scale_corr by more than ten times its gate, so the cases tell
    a kernel that weights wrongly from one that does not."""
    c = X.host_setup('smpl', model_root, golden)
    m = X.MODES[mode]
    r = {w: X.refs(c, 'smpl', X.Case('mask01', weights=w))[0] for w in (None, 'vj', 'v', 'j')}
    G = r[None].R1()[0]
    s = {w: x.solve(G, m) for w, x in r.items()}
    for w in ('v', 'j'):
        assert all(np.array_equal(s[w][k], s[None][k]) for k in ('scale_corr', 'trans', 'shape_betas')), w
    assert np.abs(s['vj']['scale_corr'] - s[None]['scale_corr']).max() > 10 * X.SCALE_GATE
    rn = {w: X.refs(c, 'smpl', X.Case('mask01', joints=False, weights=w))[0] for w in (None, 'v')}
    sn = {w: x.solve(G, m) for w, x in rn.items()}
    assert np.abs(sn['v']['scale_corr'] - sn[None]['scale_corr']).max() > 10 * X.SCALE_GATE


def test_scale_is_recovered(model_root, golden):
    """The targets really carry the factors: on 'pose1' the fp64 scaled solve returns scale_corr within 15 % of
    1 / factor (scale_target) and of factor (scale_fit) — one pass of rotations from the rest pose leaves the rest to the
    shape —, and every row but the first is gated more than 0.05 away from 1."""
    c = X.host_setup('smpl', model_root, golden)
    r64 = X.refs(c, 'smpl', X.Case('pose1'))[0]
    G = r64.R1()[0]
    st, sf = r64.solve(G, 1)['scale_corr'], r64.solve(G, 2)['scale_corr']
    assert np.abs(st * X.FACTORS - 1).max() < 0.15 and np.abs(sf / X.FACTORS - 1).max() < 0.15, (st, sf)
    assert np.abs(st[1:] - 1).min() > 0.05 and np.abs(sf[1:] - 1).min() > 0.05, (st, sf)
    assert X.FACTORS[0] == 1 and X.FACTORS[1] == np.float32(1.1) and X.FACTORS.min() == np.float32(0.8) and X.FACTORS.max() == 1.25


@MIRROR_LOOSE
@pytest.mark.parametrize('name,mode,step', [k + (s,) for k, steps in HOST_MISS.items() for s in steps])
def test_known_miss(name, mode, step, model_root, golden, capsys):
    """The steps of 'mirror' whose distance gate misses on a hand or an ankle (module docstring): raises the deferred
    assertion of one such step, unchanged.  Every other gate of the case holds (test_chain_hostemu)."""
    with capsys.disabled():
        figs = chain(name, X.Case('mirror', reg=X.ridge(name, 'mirror')), X.MODES[mode], model_root, golden)
    if step in figs['deferred']:
        raise figs['deferred'][step]
