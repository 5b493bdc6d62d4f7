"""The known-shape stage chain of tests/known_shape_chain_util.py with the host emulation (hostemu_util.fit_known_shape:
the product's stage code of sf_stages.h compiled for the CPU) standing in for the device, B = 8: the references and the
criteria are reachable in fp32, on all three models and on every family and option of the GPU test, and the condition the
GPU test depends on holds — on every (model, family, step) the fp64 oracle alone puts at least stage_util.MIN_GATED of the
(instance, part) pairs under a distance gate, except for the combinations known_shape_chain_util.SHARE_EXEMPT names with
their measured share.

'mirror' misses distance gates here as it does in a fit (tests/test_gpu_stage_chain.py: KNOWN_MISS), only on more pairs:
with the known shape the reflected target is matched against the posed mesh of its own betas, and the part covariances of
the hands (22 / 23: gap 0.02 .. 0.07) and ankles (7 / 8 as bone parts: kappa 0.01 .. 0.02; as adjustable parts of the
refinement: gap 0.011) are loose in fp32.  HOST_MISS lists the steps; figures per pair, host emulation against the fp32
oracle, |G - G64| with the bone factor (gate 5e-4 / 2e-3 on smplxfat, floor 2 x the fp32 oracle on THAT pair):
  smpl     R1 (1, 7) 6.0e-4 / 9.6e-5, (6, 23) 6.5e-4 / 2.5e-4      R2 (0, 22) 1.07e-3 / 4.8e-4, (1, 8) 5.4e-4 / 2.0e-5
           F and F with scale_fit (3, 7) 1.14e-3 / 2.6e-5 (1.1e-4 with scale_fit)
  smpl_w6  R1 (0, 23) 3.1e-3 / 1.3e-3, (4, 22) 1.35e-3 / 5.6e-4, (7, 23) 1.8e-3 / 2.6e-4
           R2 (0, 21) 7.3e-4 / 3.5e-4, (2, 22) 1.8e-3 / 9.1e-4, (4, 22) 1.2e-3 / 4.6e-4, (4, 23) 7.1e-4 / 3.3e-4, (7, 22) 1.6e-3 / 1.0e-4
  smplxfat R1 (3, 24) 2.5e-3 / 1.1e-3, (7, 51) 3.2e-3 / 4.4e-5
It is conditioning, not a wrong term: every deficit of these steps is <= 5.5e-7, the fp32 oracle's <= 6.3e-7 (the
rotations are optima of the fp64 covariance to rounding), the family maxima of the two fp32 evaluations agree (smpl R1
2.7e-3 / 2.7e-3, R2 2.3e-3 / 2.6e-3; smpl_w6 R1 3.1e-3 / 2.3e-3; smplxfat R1 3.2e-3 / 2.1e-3), and on the SAME part of a
neighbouring row the fp32 oracle is as far off where the emulation is not (smpl part 7 at F: row 2 oracle 1.8e-3, emulation
2.3e-4; smplxfat part 51 at R1: row 4 oracle 1.7e-3, emulation 8.5e-4): a floor from one fp32 evaluation of a pair does
not bound another by a factor of two.  Those steps are deferred and raised by test_known_miss, expected to fail, strictly;
every other gate of the 'mirror' case, and every gate of every other case, holds."""

import numpy as np
import pytest

import hostemu_util as H
import known_shape_chain_util as K
import stage_util as S
import util

MODELS = ('smpl', 'smplxfat', 'smpl_w6')
HOST_MISS = {'smpl': ('R1', 'R2', 'F', 'F/s'), 'smpl_w6': ('R1', 'R2'), 'smplxfat': ('R1',)}  # 'mirror', target joints given
MIRROR_LOOSE = pytest.mark.xfail(strict=True, reason="'mirror': hands and ankles with gap / kappa of 0.01 .. 0.07 scatter by more "
                                                     'than 2 x the fp32 oracle on that pair (module docstring)')
_checked = {}


def chain(name, case, model_root, golden):
    """check_chain's figures of one (model, case), computed once."""
    key = (name, case.id)
    if key not in _checked:
        c = S.host_setup(name, model_root, golden)
        kind, md = util.load_md(model_root, name, golden(name))
        defer = HOST_MISS[name] if case.id == 'mirror-j' else ()
        _checked[key] = K.check_chain(name, c, case, K.host_chain(md, kind, c, case, H), 'hostemu', defer=defer)
    return _checked[key]


def test_family_betas_are_the_families_own(model_root, golden):
    """The replayed betas pose 'betas5' again bit for bit (asserted in family_betas); they are the corners, and every
    other family's are the first draw."""
    c = S.host_setup('smpl', model_root, golden)
    b = K.family_betas(c['om64'], c['fams'])
    assert set(b) == set(c['fams']) and np.all(np.abs(b['betas5']) == 5) and np.array_equal(b['pose1'], b['far'])
    assert np.abs(b['pose1']).max() < 2.5


@pytest.mark.parametrize('name', MODELS)
def test_chain_hostemu(name, model_root, golden, capsys):
    """Every case of known_shape_chain_util.cases() through the six calls; prints each step's figures, then the lowest
    gated share per (family, step), which must be under the cap exactly where SHARE_EXEMPT says."""
    seen = {}
    with capsys.disabled():
        print()
        for case in K.cases(name):
            for k, v in K.gated_shares(name, case, chain(name, case, model_root, golden)).items():
                seen[k] = min(seen.get(k, 1.0), v)
        print(f'[gated shares {name}] ' + ' '.join(f'{f}/{s} {v:.3f}' for (_, f, s), v in seen.items()))
    low = {k: v for k, v in seen.items() if k[1] in S.UNMASKED and v < S.MIN_GATED}
    listed = {k: v for k, v in K.SHARE_EXEMPT.items() if k[0] == name}
    assert set(low) == set(listed) and all(abs(low[k] - listed[k]) < 5e-3 for k in low), (low, listed)


@MIRROR_LOOSE
@pytest.mark.parametrize('name,step', [(n, s) for n, steps in HOST_MISS.items() for s in steps])
def test_known_miss(name, step, model_root, golden, capsys):
    """The steps of 'mirror' whose distance gate misses on a hand or an ankle (module docstring): raises the deferred
    assertion of one such step, unchanged."""
    with capsys.disabled():
        figs = chain(name, K.Case('mirror'), model_root, golden)
    if step in figs['deferred']:
        raise figs['deferred'][step]


def test_alignment_weight_rules(model_root, golden):
    """What the oracle's alignment takes as weights (the facts the GPU cases 'v' and 'j' rest on): with target joints,
    vertex weights alone or joint weights alone leave it UNWEIGHTED, both weight it; without target joints the vertex
    weights do enter — and on 'mask01' each of these moves the translation by more than ten times the gate, so the cases
    tell a kernel that weights wrongly from one that does not."""
    c = S.host_setup('smpl', model_root, golden)
    r = {w: K.refs(c, K.Case('mask01', weights=w))[0] for w in (None, 'vj', 'v', 'j')}
    G = r[None].R1()[0]
    t = {w: x.T(G, True) for w, x in r.items()}
    for w in ('v', 'j'):
        assert np.array_equal(t[w][1], t[None][1]) and np.array_equal(t[w][0], t[None][0]), w
    assert np.abs(t['vj'][1] - t[None][1]).max() > 10 * K.ALIGN_GATE
    rn = {w: K.refs(c, K.Case('mask01', joints=False, weights=w))[0] for w in (None, 'v')}
    tn = {w: x.T(G, True) for w, x in rn.items()}
    assert np.abs(tn['v'][1] - tn[None][1]).max() > 10 * K.ALIGN_GATE
