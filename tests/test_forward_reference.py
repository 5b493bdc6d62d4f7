"""The fp64 side of tests/test_gpu_forward.py, checked without a GPU: ``util.forward64`` (the oracle's forward with every
input form of ``BodyModel.forward``) against the reference's forward goldens, and the generated inputs of
``util.forward_inputs`` against the gates — a subtly wrong kernel must move the result by far more than a gate allows,
and a GPU failure must point at the kernel, not at the test."""

import numpy as np
import pytest

import util

GOLDEN_GATE = 2e-6


def _max(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize('name', ['smpl', 'smplx', 'smpl1024'])
def test_forward64_goldens(name, model_root, golden):
    """Every input form against the reference's fp32 forward: pose rotation vectors, the global rotations composed in
    fp64 and rounded once, the relative ones (composed back in fp64 by the helper); the kid blend shape; chunking and
    row selection change nothing."""
    g = golden(name)
    kind, md = util.load_md(model_root, name, g)
    om = util.O.OracleModel(md, np.float64, kind)
    glob32, rel32 = util.rotation_forms(g['pose'], om.parents)
    forms = dict(pose=dict(pose_rotvecs=g['pose']), glob=dict(glob_rotmats=glob32), rel=dict(rel_rotmats=rel32))
    for form, rot in forms.items():
        f = util.forward64(om, shape_betas=g['betas'], trans=g['trans'], **rot)
        errs = (_max(f['vertices'], g['target_vertices']), _max(f['joints'], g['fwd_joints']),
                _max(f['orientations'], g['fwd_orientations']))
        assert max(errs) < GOLDEN_GATE, (form, errs)
    f = util.forward64(om, g['pose'], g['betas'], g['trans'])
    fc = util.forward64(om, g['pose'], g['betas'], g['trans'], chunk=3)
    fr = util.forward64(om, g['pose'], g['betas'], g['trans'], rows=[6, 1])
    for k in f:
        assert _max(fc[k], f[k]) < 1e-12 and _max(fr[k], f[k][[6, 1]]) < 1e-12, k
    if 'kid' in g:
        fk = util.forward64(om, g['pose'], g['betas'], g['trans'], kid_factor=g['kid'])
        assert _max(fk['vertices'], g['kid.target_vertices']) < GOLDEN_GATE
        assert _max(fk['joints'], g['kid.fwd_joints']) < GOLDEN_GATE


@pytest.mark.parametrize('kind', list(util.GENERAL_KINDS))
def test_forward64_general_goldens(kind, model_root, golden):
    """The general-path models of golden_general.npz (32 and 300 betas, twelve skinning weights), and fewer betas given
    than the model holds."""
    gg = golden('general')
    om = util.O.OracleModel(util.load_general_md(model_root, kind), np.float64, 'smpl')
    p = kind + '.'
    f = util.forward64(om, gg[p + 'pose'], gg[p + 'betas'], gg[p + 'trans'])
    assert _max(f['vertices'], gg[p + 'target_vertices']) < GOLDEN_GATE
    assert _max(f['joints'], gg[p + 'target_joints']) < GOLDEN_GATE
    assert _max(f['orientations'], gg[p + 'fwd_orientations']) < GOLDEN_GATE
    if p + 'fwd10_joints' in gg:
        f = util.forward64(om, gg[p + 'pose'], gg[p + 'betas'][:, :10], gg[p + 'trans'])
        assert _max(f['vertices'][:, ::50], gg[p + 'fwd10_vertices_every_50th']) < GOLDEN_GATE
        assert _max(f['joints'], gg[p + 'fwd10_joints']) < GOLDEN_GATE


def test_forward64_input_forms(model_root, golden):
    """The forms without a fixture of their own, against the explicit form they stand for: no rotation input = zero
    rotation vectors, no betas = zero betas, a (1, 3) translation and a scalar kid factor = the same value on every
    instance; the row cache returns what forward64 returns."""
    g = golden('smpl')
    kind, md = util.load_md(model_root, 'smpl', g)
    om = util.O.OracleModel(md, np.float64, kind)
    x = util.forward_inputs(9, om.J, om.S, seed=4)
    B = 9
    a = util.forward64(om, shape_betas=x['shape_betas'], trans=x['trans'][:1])
    b = util.forward64(om, np.zeros((B, 3 * om.J), np.float32), x['shape_betas'], np.repeat(x['trans'][:1], B, 0))
    c = util.forward64(om, x['pose_rotvecs'], trans=x['trans'], kid_factor=np.float32(0.7))
    d = util.forward64(om, x['pose_rotvecs'], np.zeros((B, 10), np.float32), x['trans'], kid_factor=np.full(B, 0.7, np.float32))
    for k in a:
        assert _max(a[k], b[k]) < 1e-12 and _max(c[k], d[k]) < 1e-12, k
    ref = util.Ref64(om, **x)
    r = ref.rows([8, 0, 3])
    f = util.forward64(om, **x)
    for k in r:
        assert _max(r[k], f[k][[8, 0, 3]]) < 1e-12, k
    assert sorted(ref.cache) == [0, 3, 8]


def test_forward_gates_see_subtle_bugs(model_root, golden):
    """On the generated inputs each of the kernel bugs the GPU file is there to catch moves the fp64 result by at least
    10x the vertex gate: the last posedirs feature dropped, the last beta dropped, the kid term dropped, two instances
    of the last 64-instance block swapped.  The inputs hold every branch value forward_inputs promises."""
    g = golden('smpl')
    kind, md = util.load_md(model_root, 'smpl', g)
    om = util.O.OracleModel(md, np.float64, kind)
    B = 70
    x = util.forward_inputs(B, om.J, om.S, seed=1)
    # the inputs themselves
    r = np.linalg.norm(x['pose_rotvecs'].reshape(B, om.J, 3).astype(np.float64), axis=-1)
    assert (r == 0).all(axis=1).any() and ((r == 0) & ~(r == 0).all(axis=1, keepdims=True)).any()
    assert ((r > 0) & (r <= 1e-4)).any() and (r > np.pi).any() and np.abs(x['pose_rotvecs']).max() > 2.5
    assert np.abs(x['shape_betas']).max() == 5 and np.abs(x['shape_betas'][:, -1]).min() >= 0.5
    assert np.abs(x['trans'][util.FWD_FAR]).min() > 990 and np.abs(np.delete(x['trans'], util.FWD_FAR, 0)).max() < 10
    base = util.forward64(om, **x)
    floor = 10 * util.FWD_GATE_M
    om_pd = util.O.OracleModel(md, np.float64, kind)
    om_pd.posedirs = om_pd.posedirs.copy()
    om_pd.posedirs[..., -1] = 0
    moved = dict(
        posedirs_last=util.forward64(om_pd, **x),
        beta_last=util.forward64(om, **dict(x, shape_betas=np.concatenate([x['shape_betas'][:, :-1], 0 * x['shape_betas'][:, -1:]], 1))),
        kid=util.forward64(om, **dict(x, kid_factor=None)),
    )
    sw = np.arange(B)
    sw[[B - 1, B - 3]] = sw[[B - 3, B - 1]]  # rows 67 and 69: both in the last instance block 64..69
    moved['swap_last_block'] = {k: v[sw] for k, v in base.items()}
    for what, f in moved.items():
        for k in ('vertices', 'joints'):
            if what == 'posedirs_last' and k == 'joints':
                continue  # posedirs does not move the joints
            d = _max(f[k], base[k])
            assert d >= floor, (what, k, d)
    # every row sees the dropped beta and the dropped kid term, not only the worst one
    for what in ('beta_last', 'kid'):
        per_row = np.abs(moved[what]['vertices'] - base['vertices']).reshape(B, -1).max(1)
        assert per_row.min() >= floor, (what, per_row.min())
