"""-m gpu: the general path (kernels_gen.inc: any number of shape unknowns) at every launch shape of its kernels, at the
batch edge of the four-instances-per-workgroup LBS kernel, on an SMPL-X-shaped model and on the hard targets of
tests/stage_util.py — always against the fp64 oracle of the same operation, the fp32 oracle as the floor.

1. test_accumulate_shapes: one shape solve per count of unknowns on both sides of every switch of k_gen_accum_mfma and
   k_gen_accum (general_util.sweep_branches names the branch of each count), both forms, with the kid and the scale
   unknowns and the three ways weights enter a solve.
2. test_ni4_*: k_gen_lbs<MODE, WEIGHTED, 4> (S >= 48 and B >= 2048) at B = 2048..2051 on SMPL and at 2049 on the
   SMPL-X-shaped model (its LDS above 64 KB): forward, fit with and without joints, weighted, poisoned rows.
3. test_smplx_*: a 55-joint general model at 20, 64 and 300 betas: forward, the stages, whole fits, both accumulate forms.
4. test_stage_families / test_poisoned_row_general: stage_util's families and the poisoned row through the general kernels.

Figures of one MI355X run are in the docstrings of the tests, next to the fp32 oracle's.  What no test here can show is
WHICH instantiation ran: the library reports the kernel family of a model (kernel_path() == 'general') but no per-call
route.  general_util.launch_rules restates the launch rules and tests/test_general_shapes_host.py pins them at the
thresholds; that SMPLFIT_GEN_MFMA switched the accumulate form is shown by the bits of the two results."""

import numpy as np
import pytest
import torch

import general_util as G
import stage_util as S
import util
from test_gpu_forward import GATE_M
from test_gpu_parity import t, to_np

pytestmark = pytest.mark.gpu

FORMS = (('mfma', None), ('valu', '0'))  # SMPLFIT_GEN_MFMA: k_gen_accum_mfma (default) / k_gen_accum
# the stage harness on this path: an unmasked family runs the unweighted ridge solve and the weighted one without a ridge
# (add_mean), a masked family the latter with its own weights (the four SOLVE_CASES of test_shape_solve_hard cost four
# fp64 solves of up to 300 unknowns per family)
STAGE_CASES = tuple(c for c in S.SOLVE_CASES if c[0] in ('reg1', 'reg0_w_mean'))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def groot(model_root):
    """The session's model root with the SMPL-X-shaped 300-beta file beside smpl_b100 / smpl_b400."""
    from smplfitter_amd import synth

    return synth.ensure_model_root(root=model_root, kinds=('smplx_fat_b300',))


_models = {}


def model(root, name, nb, dev, keep=True):
    """(BodyModel, BodyFitter, BodyFitter with the kid unknown) of ``name`` at ``nb`` betas; cached unless ``keep`` is off."""
    from smplfitter_amd.pt import BodyFitter, BodyModel

    key = (name, nb)
    if key in _models:
        return _models[key]
    m = BodyModel(G.MODELS[name][0], 'neutral', model_root=f'{root}/{name}', num_betas=nb, device=dev)
    assert m.num_betas == nb and m.kernel_path() == 'general' and m.kernel_path(enable_kid=True) == 'general'
    r = (m, BodyFitter(m), BodyFitter(m, enable_kid=True))
    if keep:
        _models[key] = r
    return r


def forward_gate(nb, floor):
    """Vertices and joints of a forward (m, + 4 ulp): the gate tests/test_gpu_forward.py holds a kind of that many betas
    to — util.FWD_GATE_M, at 300 betas its smpl_b300 entry — else twice the fp32 floor (general_util.forward_floors)."""
    return max(GATE_M['smpl_b300'] if nb >= 300 else util.FWD_GATE_M, 2 * floor)


def worst(figs):
    """'mesh 1.2e-06 (3.4e-05) ...': the maxima of check_solve's figures, ours (the fp32 oracle's)."""
    keys = ('mesh', 'joints', 'betas', 'trans')
    return ' '.join(f'{k} {max(f[k] for f in figs):.1e} ({max(f[k + "32"] for f in figs):.1e})' for k in keys)


# ---- 1. the accumulate kernels at every launch shape ------------------------------------------------------------------
def sweep_cases(c, n, V, J):
    """(tag, kid, family, vertex weights, joint weights, beta_regularizer, add_mean, scale_mode) of one count."""
    p1 = c['fams']['pose1']
    fam = G.head(p1, G.ROWS)
    vw, jw = (w[:G.ROWS] for w in S.solve_weights(p1, V, J))
    cases = [('reg1', False, fam, None, None, 1.0, False, 0), ('reg0_w_mean', False, fam, vw, jw, 0.0, True, 0),
             ('kid_reg1', True, fam, None, None, 1.0, False, 0)]
    if n in G.ENTRY_COUNTS:
        for tag, (tj, v, j) in G.entry_weights(p1, V, J).items():
            sl = lambda a: None if a is None else a[:G.ROWS]  # noqa: E731
            cases.append((tag, False, dict(fam, tj=sl(tj)), sl(v), sl(j), 1.0, False, 0))
    if n in G.SCALE_COUNTS:
        cases += [(f'scale{mode}', False, G.scaled_targets(fam), None, None, 1.0, False, mode) for mode in (1, 2)]
    return cases


@pytest.mark.parametrize('n', G.SWEEP)
def test_accumulate_shapes(n, groot, dev, smplfit_env, capsys):
    """BodyFitter._shape_solve on smpl_b400 at ``n`` betas, at the fp64 oracle's rotations rounded to fp32, four rows of
    'pose1', on k_gen_accum_mfma and on k_gen_accum (SMPLFIT_GEN_MFMA=0): unweighted with beta_regularizer 1; weighted
    (0/1 masks, a joint at 0) without a ridge, add_mean; the kid fitter (n + 1 unknowns: every block boundary from the
    other side); at 30 and 156 the three ways weights enter; at 27, 30, 60, 156, 316 the scale unknown in both modes
    (matrix-core form; the other form must refuse it with SMPLFIT_ERR_UNSUPPORTED).  Gates of stage_util.check_solve
    against OracleFitter.fit_shape in fp64; the kid factor and the scale correction are held to the beta gate, a scaled
    solve's mesh is the fp64 forward at its unknowns (general_util.solve_view).  The two forms must differ somewhere in
    bits: the switch took effect.
    (one MI355X, worst case over the 23 counts, ours (the fp32 oracle's) — matrix-core form: mesh 1.1e-5 m (4.3e-4), joints
    6.0e-6 m (3.6e-4), betas 3.8e-4 (1.4e-3), trans 5.0e-6 (1.7e-5); vector form, which has no scaled case: 1.2e-5
    (4.3e-5), 6.2e-6 (1.9e-5), 3.8e-4 (1.1e-3), 5.4e-6 (1.7e-5); all at 393 betas with the kid unknown, no family maximum
    above 0.45 of its gate.  Before the accumulate kernels added their fp32 sums to the fp64 record every 512 vertices
    (kGenFlushVertices) the vector form, one fp32 chain over all 20670 rows, missed the beta gate in the weighted
    ridge-free case at 20, 21, 27 and 28 betas, four of the five counts that run reached — 4.0e-4 .. 4.8e-4 where the fp32
    oracle has 2.3e-5 .. 1.2e-4 on the same row; with the flushes: 1.7e-5 at 20.)"""
    c = G.setup(groot, 'smpl_b400', n, transient=True)
    m, f, fk = model(groot, 'smpl_b400', n, dev, keep=False)
    Gr = G.rotations(c, 'pose1')[0][0][:G.ROWS].astype(np.float32)
    rows = np.arange(G.ROWS)
    out, figs = {}, []
    with capsys.disabled():
        print(f'\n[sweep n={n}] plain {G.launch_rules(n, 24)}\n[sweep n={n}] kid   {G.launch_rules(n + 1, 24)}')
        for form, env in FORMS:
            smplfit_env('SMPLFIT_GEN_MFMA', env)
            for tag, kid, fam, vw, jw, reg, add_mean, scale in sweep_cases(c, n, m.num_vertices, m.num_joints):
                args = (t(Gr, dev), t(fam['tv'], dev), t(fam['tj'], dev), t(vw, dev), t(jw, dev))
                kw = dict(beta_regularizer=reg, add_mean=add_mean, scale_mode=scale, want_mesh=not scale)
                if scale and form == 'valu':
                    with pytest.raises(NotImplementedError, match='SMPLFIT_GEN_MFMA=0'):
                        f._shape_solve(*args, **kw)
                    continue
                r = to_np((fk if kid else f)._shape_solve(*args, **kw))
                out[form, tag] = r
                r64, r32, mean64 = G.oracle_solve(c, fam, Gr, reg, vw, jw, kid, scale, key=('sweep', tag))
                figs.append(S.check_solve('smpl_b400', 'pose1', tag, G.solve_view(c, r, Gr, kid, scale), r32, r64, mean64,
                                          add_mean, f'n={n} {form}', rows=rows))
        print(f'[sweep n={n}] worst {worst(figs)}')
    differs = any(not np.array_equal(out['mfma', tag][k], out['valu', tag][k]) for (form, tag) in out if form == 'valu'
                  for k in out[form, tag])
    assert differs, (n, 'SMPLFIT_GEN_MFMA=0 changed nothing: k_gen_accum did not run')


# ---- 2. four instances per workgroup -----------------------------------------------------------------------------------
NI4 = {'smpl_b100': 48, 'smplx_fat_b300': 64}
NI4_CASES = [('smpl_b100', B) for B in (2048, 2049, 2050, 2051)] + [('smplx_fat_b300', 2049)]
FIT_KW = dict(num_iter=2, beta_regularizer=1.0, requested_keys=['pose_rotvecs'])
FIT_KEYS = ('pose_rotvecs', 'shape_betas', 'trans')
_ni4 = {}


def fit_inputs(c, rows, seed):
    """Targets of a whole fit, as test_general_full_size makes them (poses of 0.1 rad a component, + 5 mm of noise on
    the vertices) but from the fp64 forward; weights: 0/1 vertex masks times [0.5, 1.5), one joint at 0."""
    om = c['om64']
    rs = np.random.RandomState(seed)
    pose = (rs.randn(rows, 3 * om.J) * 0.1).astype(np.float32)
    betas = (rs.randn(rows, om.S) * (0.5 if om.S <= 32 else 0.15)).astype(np.float32)
    trans = rs.randn(rows, 3).astype(np.float32)
    fw = util.forward64(om, pose_rotvecs=pose, shape_betas=betas, trans=trans)
    tv = (fw['vertices'] + 0.005 * rs.randn(rows, om.V, 3)).astype(np.float32)
    vw = ((rs.rand(rows, om.V) < 0.7) * (rs.rand(rows, om.V) + 0.5)).astype(np.float32)
    jw = (rs.rand(rows, om.J) + 0.5).astype(np.float32)
    jw[:, om.J // 2] = 0
    return dict(pose=pose, betas=betas, trans=trans, tv=tv, tj=fw['joints'].astype(np.float32), vw=vw, jw=jw)


def fit_variants(x):
    """tag -> keyword arguments of fit: MODE 0 of k_gen_lbs (joints given), MODE 1 (joints regressed from the mesh, the
    padding slots written), and their WEIGHTED instantiations."""
    return dict(j=dict(target_joints=x['tj']), nj=dict(target_joints=None),
                j_w=dict(target_joints=x['tj'], vertex_weights=x['vw'], joint_weights=x['jw']),
                nj_w=dict(target_joints=None, vertex_weights=x['vw']))


def fit_gate(om64, o, ref, ref32, what):
    """The criterion of test_general_full_size: the mesh of the result against the fp64 oracle's, evaluated in fp64,
    under max(2 x the fp32 oracle's own distance, 3e-5) and 1e-4 m."""
    err, floor = util.vertex_l2(om64, o, ref), util.vertex_l2(om64, ref32, ref)
    print(f'[fit] {what}: vtx {err:.2e} (fp32 oracle {floor:.2e})')
    assert err < max(2 * floor, 3e-5) and err < 1e-4, (what, err, floor)
    return err, floor


def ni4_setup(root, name):
    """Eight source rows of forward and fit inputs with the oracles' results: computed once, shared, read only."""
    if name not in _ni4:
        c = G.setup(root, name, NI4[name])
        om64 = c['om64']
        fi = util.forward_inputs(S.B, om64.J, om64.S, seed=3)
        fin = dict(pose_rotvecs=fi['pose_rotvecs'], shape_betas=fi['shape_betas'], trans=fi['trans'])
        x = fit_inputs(c, S.B, seed=11)
        fits = {}
        for tag, kw in fit_variants(x).items():
            okw = dict(kw, num_iter=FIT_KW['num_iter'], beta_regularizer=FIT_KW['beta_regularizer'])
            fits[tag] = (c['of64'].fit(x['tv'], **okw), c['of32'].fit(x['tv'], **okw))
        fw64 = util.forward64(om64, **fin)
        _ni4[name] = dict(c=c, fin=fin, fw64=fw64, floors=G.forward_floors(c, fin, fw64), x=x, fits=fits)
    return _ni4[name]


def same_source_rows(v, Bn):
    """Every row of ``v`` (Bn rows tiling 8 sources) equals, bit for bit, the first row of its source."""
    return bool(torch.equal(v, v[:S.B][torch.arange(Bn, device=v.device) % S.B]))


@pytest.mark.parametrize('name,Bn', NI4_CASES)
def test_ni4_forward(name, Bn, groot, dev, smplfit_env, capsys):
    """BodyModel.forward (k_gen_lbs MODE 2, NI = 4) on 8 source rows of util.forward_inputs tiled to the batch: every row
    against the fp64 forward of its source — vertices and joints under forward_gate (util.FWD_GATE_M, else 2 x the fp32
    floor of general_util.forward_floors) + 4 ulp, orientations 1e-6 (the gates of test_gpu_forward.py; these kinds have no gate of their own there)
    — and rows of one source bit for bit equal whatever their slot in a group of four or their workgroup.  The same 8
    rows run as a batch of 8 (NI = 1) are NOT the same bits: the source states one sequence of operations per instance,
    but the two instantiations are compiled separately and the compiler contracts their multiply-adds differently, so
    the batch of 8 is held to the same gates and the distance between the two is a record.
    (one MI355X: excess over 4 ulp, vertices 7.5e-7 m on smpl_b100 and 1.2e-6 on smplx_fat_b300 (the fp32 floor:
    2.9e-7 / 3.2e-7), joints 1.3e-7 / 1.7e-7, orientations 3.7e-7 / 6.1e-7, the same figures for the batch of 8; NI = 4
    against the batch of 8: 2.4e-7 m, one ulp of a coordinate between 2 and 4 m; joints and orientations bit for bit)"""
    s = ni4_setup(groot, name)
    m, _, _ = model(groot, name, NI4[name], dev)
    assert G.launch_rules(NI4[name], m.num_joints, Bn)['lbs_ni'] == 4
    rows = torch.arange(Bn, device=dev) % S.B
    x = {k: t(v, dev) for k, v in s['fin'].items()}
    fw = m(x['pose_rotvecs'][rows], x['shape_betas'][rows], x['trans'][rows])
    fw8 = m(x['pose_rotvecs'], x['shape_betas'], x['trans'])
    fv, fj = s['floors']
    with capsys.disabled():
        print()
        for tag, res in (('NI = 4', fw), ('batch of 8', fw8)):
            ev, ej, eo = util.forward_errors({k: v[:S.B].cpu().numpy() for k, v in res.items()}, s['fw64'])
            print(f'[ni4 forward] {name} B={Bn} {tag}: excess vertices {ev:.2e} ({fv:.2e}) joints {ej:.2e} ({fj:.2e}) orientations {eo:.2e}')
            assert ev <= forward_gate(NI4[name], fv) and ej <= forward_gate(NI4[name], fj) and eo <= 1e-6, (tag, ev, fv, ej, fj, eo)
        print(f'[ni4 forward] {name} B={Bn}: NI = 4 against the batch of 8, vertices {(fw["vertices"][:S.B] - fw8["vertices"]).abs().max().item():.2e}')
    for k in fw:
        assert same_source_rows(fw[k], Bn), (k, 'rows of one source differ')
    for k in ('joints', 'orientations'):  # (k_forward_joint: a workgroup per instance whatever the batch)
        assert torch.equal(fw[k][:S.B], fw8[k]), k


@pytest.mark.parametrize('name,Bn', NI4_CASES)
def test_ni4_fit(name, Bn, groot, dev, smplfit_env, capsys):
    """fit(num_iter=2) with k_gen_lbs NI = 4 in MODE 0 (joints given), MODE 1 (target_joints=None: the regression source
    and its padding slots) and their WEIGHTED forms, on 8 source rows tiled to the batch (SMPLFIT_CHUNKS=1: a 55-joint
    model would otherwise split 2049 rows into 1024 + 1025, both below the NI = 4 threshold; a 24-joint model runs one
    chunk anyway, chunk_count).  Rows of one source agree bit for bit; the 8 sources, and the same 8 rows fitted as a
    batch of 8 (NI = 1: other bits, see test_ni4_forward), against OracleFitter.fit in fp64 under the criterion of
    test_general_full_size, the distance between the two a record.
    (one MI355X, mesh against the fp64 fit: 2.7e-6 .. 5.5e-6 m on smpl_b100, 5.1e-6 .. 8.7e-6 on smplx_fat_b300 — the
    fp32 oracle 1.4e-5 .. 3.2e-5 — the batch of 8 within 5e-7 of that; NI = 4 against the batch of 8: 1.1e-6 .. 4.8e-6 m)"""
    s = ni4_setup(groot, name)
    c = s['c']
    smplfit_env('SMPLFIT_CHUNKS', '1')
    _, f, _ = model(groot, name, NI4[name], dev)
    rows = torch.arange(Bn, device=dev) % S.B
    xd = {k: t(v, dev) for k, v in s['x'].items()}
    with capsys.disabled():
        print()
        for tag, kw in fit_variants(xd).items():
            big = {k: (None if v is None else v[rows]) for k, v in kw.items()}
            r = f.fit(xd['tv'][rows], **big, **FIT_KW)
            r8 = f.fit(xd['tv'], **kw, **FIT_KW)
            for k in FIT_KEYS:
                assert same_source_rows(r[k], Bn), (tag, k, 'rows of one source differ')
            ref, ref32 = s['fits'][tag]
            o, o8 = ({k: x[k][:S.B].cpu().numpy() for k in FIT_KEYS} for x in (r, r8))
            fit_gate(c['om64'], o, ref, ref32, f'ni4 {name} B={Bn} {tag} NI = 4')
            fit_gate(c['om64'], o8, ref, ref32, f'ni4 {name} B={Bn} {tag} batch of 8')
            print(f'[fit] ni4 {name} B={Bn} {tag}: NI = 4 against the batch of 8, vtx {util.vertex_l2(c["om64"], o, o8):.2e}')


def test_ni4_poisoned_row(groot, dev):
    """B = 2050 (the last workgroup holds rows 2048, 2049 and two clamped copies of 2049): one row NaN — in turn 2049
    (the row the clamped slots compute again), 2047 (the last slot of a full group) and 2 — in forward, fit and fit
    without joints.  Every other row is bit-identical to the clean run; the poisoned row is non-finite."""
    name, Bn, poison = 'smpl_b100', 2050, float('nan')
    s = ni4_setup(groot, name)
    m, f, _ = model(groot, name, NI4[name], dev)
    rows = torch.arange(Bn, device=dev) % S.B
    fin = {k: t(v, dev)[rows] for k, v in s['fin'].items()}
    xd = {k: t(v, dev)[rows] for k, v in s['x'].items()}
    clean_fw = m(fin['pose_rotvecs'], fin['shape_betas'], fin['trans'])
    clean = {tag: f.fit(xd['tv'], xd['tj'] if tag == 'j' else None, **FIT_KW) for tag in ('j', 'nj')}
    assert all(torch.isfinite(v).all() for v in clean_fw.values())
    assert all(torch.isfinite(r[k]).all() for r in clean.values() for k in FIT_KEYS)
    for row in (2049, 2047, 2):
        keep = torch.arange(Bn, device=dev) != row
        pose = fin['pose_rotvecs'].clone()
        pose[row] = poison
        fw = m(pose, fin['shape_betas'], fin['trans'])
        for k in fw:
            assert torch.equal(fw[k][keep], clean_fw[k][keep]), (row, k)
        assert not torch.isfinite(fw['vertices'][row]).any(), row
        tv, tj = xd['tv'].clone(), xd['tj'].clone()
        tv[row], tj[row] = poison, poison
        for tag in ('j', 'nj'):
            r = f.fit(tv, tj if tag == 'j' else None, **FIT_KW)
            for k in FIT_KEYS:
                assert torch.equal(r[k][keep], clean[tag][k][keep]), (row, tag, k)
            assert not torch.isfinite(r['shape_betas'][row]).any() and not torch.isfinite(r['trans'][row]).any(), (row, tag)


# ---- 4. (and the stage part of 3.) stage_util's families through the general kernels ---------------------------------
STAGE_PARAMS = [pytest.param(name, nb, fam, id=f'{name}-{nb}-{fam}') for (name, nb), fams in G.STAGE_MODELS.items() for fam in fams]


def stage_rows(nb):
    return S.B if nb < 300 else G.ROWS


@pytest.mark.parametrize('name,nb,family', STAGE_PARAMS)
def test_stage_families(name, nb, family, groot, dev, smplfit_env, capsys):
    """BodyFitter._part_rotations (its part sums: k_gen_lbs MODE 0 at the template) and _shape_solve (the record of the
    accumulate kernels, both forms, WEIGHTED for the masks) on the families of stage_util.families: smpl_b400 at 32 and
    300 betas, the SMPL-X-shaped smplx_fat_b300 at 20, 64 and 300 (J = 55: k_gen_lbs, the joint rows of the matrix-core
    kernel — unstaged at 300, 201 KB — and the blocked ldlt_solve).  check_rotations / check_solve, unchanged.
    'betas5' stays in at every count: the fp64 oracle alone puts every pair of it under a distance gate at 64 and 300
    unknowns as well (gated share 1.000, its fp32 form within 7.1e-4: tests/test_general_shapes_host.py asserts the
    share), so the +-5 mesh remains one the rotation pass can be judged on.
    (one MI355X.  Rotations: deficit <= 5.7e-8; largest distance, with the bone factor, 1.6e-3 on smplx_fat_b300
    'mirror' (the fp32 oracle's 4.5e-3), 6.4e-4 on smpl_b400 'mirror' (2.3e-3), <= 2.2e-4 off the mirrored family
    (4.0e-4).  Solve, worst case over the families, the same on both forms to two digits — smpl_b400: mesh 8.1e-6 m,
    joints 8.8e-7 m, betas 2.9e-4, trans 3.7e-7 (the fp32 oracle: 3.7e-5, 4.7e-6, 9.0e-4, 1.1e-5); smplx_fat_b300:
    1.7e-5, 2.7e-6, 3.9e-4, 6.7e-7 (9.2e-5, 1.5e-5, 1.8e-3, 1.8e-5), 'betas5' at 64 betas.  With the fp32 sums added
    to the fp64 record every 2048 vertices only, 'betas5' at 32 betas missed the beta gate on the matrix-core form —
    5.1e-4, the fp32 oracle 6.6e-5 on that row — and the vector form, with one chain, every family: up to 1.0e-3.)"""
    c = G.setup(groot, name, nb)
    m, f, _ = model(groot, name, nb, dev)
    n = stage_rows(nb)
    fam = G.head(c['fams'][family], n)
    (G64, info), G32 = G.rotations(c, family)
    info_n = {k: (v if k == 'kind' else v[:n]) for k, v in info.items()}
    rows = np.arange(n)
    with capsys.disabled():
        print()
        Go = f._part_rotations(t(fam['tv'], dev), t(fam['tj'], dev), t(fam['vw'], dev), t(fam['jw'], dev)).cpu().numpy()
        S.check_rotations(name, family, S.rotation_figures(Go, G32[:n], G64[:n], info_n, S.dist_gate(c['kind'])), f'general nb={nb}')
        Gr = G64[:n].astype(np.float32)
        out = {}
        for form, env in FORMS:
            smplfit_env('SMPLFIT_GEN_MFMA', env)
            for tag, reg, weights, add_mean in STAGE_CASES:
                if fam['vw'] is not None and not weights:
                    continue
                vw, jw = (w[:n] for w in S.solve_weights(c['fams'][family], m.num_vertices, m.num_joints)) if weights else (None, None)
                r = to_np(f._shape_solve(t(Gr, dev), t(fam['tv'], dev), t(fam['tj'], dev), t(vw, dev), t(jw, dev),
                                         beta_regularizer=reg, add_mean=add_mean))
                out[form, tag] = r
                r64, r32, mean64 = G.oracle_solve(c, fam, Gr, reg, vw, jw, key=('stage', family, tag))
                S.check_solve(name, family, tag, G.solve_view(c, r, Gr), r32, r64, mean64, add_mean, f'nb={nb} {form}', rows=rows)
    differs = any(not np.array_equal(out['mfma', tag][k], out['valu', tag][k]) for (form, tag) in out if form == 'valu'
                  for k in out[form, tag])
    assert differs, (name, nb, family, 'SMPLFIT_GEN_MFMA=0 changed nothing')


@pytest.mark.parametrize('Bn,rows', [(8, (3,)), (65, (5, 63, 64)), (63, (62,))])
@pytest.mark.parametrize('poison', [float('nan'), float('inf')])
def test_poisoned_row_general(poison, Bn, rows, groot, dev):
    """The poisoned-row test of test_gpu_stages_hard.py on smpl_b400 at 32 betas: one instance with NaN (or Inf) targets
    — inside the batch, at both sides of 64, the last of 63 — beside good ones.  Every other row of both stages is
    bit-identical to the clean run, no part of the poisoned row is a finite matrix and its solve is non-finite."""
    c = G.setup(groot, 'smpl_b400', 32)
    _, f, _ = model(groot, 'smpl_b400', 32, dev)
    fam = c['fams']['pose1']
    rep = (Bn + S.B - 1) // S.B
    tv = t(np.tile(fam['tv'], (rep, 1, 1))[:Bn], dev)
    tj = t(np.tile(fam['tj'], (rep, 1, 1))[:Bn], dev)
    G0 = f._part_rotations(tv, tj)
    s0 = f._shape_solve(G0, tv, tj, beta_regularizer=1.0)
    assert torch.isfinite(G0).all() and all(torch.isfinite(v).all() for v in s0.values())
    s0 = {k: v.clone() for k, v in s0.items()}
    for row in rows:
        tvp, tjp = tv.clone(), tj.clone()
        tvp[row], tjp[row] = poison, poison
        Gp = f._part_rotations(tvp, tjp)
        s = f._shape_solve(G0, tvp, tjp, beta_regularizer=1.0)
        keep = torch.arange(Bn, device=dev) != row
        assert torch.equal(Gp[keep], G0[keep]), row
        assert not torch.isfinite(Gp[row]).all(-1).all(-1).any(), row  # no joint's matrix is finite
        for k in s0:
            assert torch.equal(s[k][keep], s0[k][keep]), (row, k)
        assert not torch.isfinite(s['shape_betas'][row]).any() and not torch.isfinite(s['trans'][row]).any(), row


# ---- 3. the SMPL-X-shaped general model: forward and whole calls -------------------------------------------------------
SMPLX_COUNTS = (20, 64, 300)
_smplx = {}


@pytest.mark.parametrize('nb', SMPLX_COUNTS)
def test_smplx_forward(nb, groot, dev, capsys):
    """BodyModel.forward of smplx_fat_b300 at B = 1 and 65 (prefixes of one set of util.forward_inputs) against the fp64
    oracle, every row: vertices and joints under forward_gate (util.FWD_GATE_M, at 300 betas the 4e-6 of smpl_b300 in
    tests/test_gpu_forward.py; else 2 x the fp32 floor of general_util.forward_floors over the 65 rows) + 4 ulp,
    orientations 1e-6.
    (one MI355X, excess over 4 ulp at B = 65: vertices 1.7e-6 / 1.7e-6 / 2.4e-6 m at 20 / 64 / 300 betas (the fp32
    floor 7.0e-7 / 4.8e-7 / 7.3e-7), joints <= 4.2e-7, orientations 6.0e-7)"""
    c = G.setup(groot, 'smplx_fat_b300', nb)
    m, _, _ = model(groot, 'smplx_fat_b300', nb, dev)
    om64 = c['om64']
    fi = util.forward_inputs(65, om64.J, om64.S, seed=5)
    fin = dict(pose_rotvecs=fi['pose_rotvecs'], shape_betas=fi['shape_betas'], trans=fi['trans'])
    ref = util.forward64(om64, **fin)
    fv, fj = G.forward_floors(c, fin, ref)
    x = {k: t(v, dev) for k, v in fin.items()}
    with capsys.disabled():
        print()
        for Bn in (1, 65):
            ours = to_np(m(x['pose_rotvecs'][:Bn], x['shape_betas'][:Bn], x['trans'][:Bn]))
            r = {k: v[:Bn] for k, v in ref.items()}
            ev, ej, eo = util.forward_errors(ours, r)
            print(f'[smplx forward] nb={nb} B={Bn}: excess vertices {ev:.2e} ({fv:.2e}) joints {ej:.2e} ({fj:.2e}) orientations {eo:.2e}')
            assert ev <= forward_gate(nb, fv) and ej <= forward_gate(nb, fj) and eo <= 1e-6, (Bn, ev, fv, ej, fj, eo)


def smplx_refs(root, nb):
    """Inputs and the oracles' results of the whole calls at ``nb`` betas (four rows): computed once for both forms."""
    if nb not in _smplx:
        c = G.setup(root, 'smplx_fat_b300', nb)
        x = fit_inputs(c, G.ROWS, seed=21)
        ref = {}
        for dt, of in (('64', c['of64']), ('32', c['of32'])):
            ref['fit', dt] = of.fit(x['tv'], x['tj'], num_iter=3, beta_regularizer=1.0)
            ref['pose', dt] = of.fit_with_known_pose(x['pose'], x['tv'], x['tj'], beta_regularizer=1.0)
            ref['shape', dt] = of.fit_with_known_shape(x['betas'], x['tv'], x['tj'], num_iter=2)
        _smplx[nb] = (c, x, ref)
    return _smplx[nb]


@pytest.mark.parametrize('form,env', FORMS)
@pytest.mark.parametrize('nb', SMPLX_COUNTS)
def test_smplx_whole_calls(nb, form, env, groot, dev, smplfit_env, capsys):
    """fit(num_iter=3), fit_with_known_pose and fit_with_known_shape(num_iter=2) of smplx_fat_b300 at B = 4, on both
    accumulate forms, against the fp64 oracle of the same call under the criterion of test_general_full_size (the mesh of
    the result, evaluated in fp64: max(2 x the fp32 oracle's distance, 3e-5) and 1e-4 m).
    (one MI355X, at 20 / 64 / 300 betas — fit: 5.5e-6 / 5.5e-6 / 8.7e-6 m (the fp32 oracle 2.0e-5 / 1.7e-5 / 3.7e-5),
    known pose 4.0e-7 / 5.5e-7 / 1.4e-6 (2.1e-6 / 4.5e-6 / 8.5e-6), known shape 6.4e-6 / 1.2e-5 / 7.6e-6 (2.3e-5 /
    2.7e-5 / 2.7e-5); the vector form within 7e-7 of the matrix-core one)"""
    c, x, ref = smplx_refs(groot, nb)
    _, f, _ = model(groot, 'smplx_fat_b300', nb, dev)
    smplfit_env('SMPLFIT_GEN_MFMA', env)
    xd = {k: t(v, dev) for k, v in x.items()}
    om64 = c['om64']
    with capsys.disabled():
        print()
        r = to_np(f.fit(xd['tv'], xd['tj'], num_iter=3, beta_regularizer=1.0, requested_keys=['pose_rotvecs']))
        fit_gate(om64, {k: r[k] for k in FIT_KEYS}, ref['fit', '64'], ref['fit', '32'], f'smplx nb={nb} {form} fit')
        kp = to_np(f.fit_with_known_pose(pose_rotvecs=xd['pose'], target_vertices=xd['tv'], target_joints=xd['tj'], beta_regularizer=1.0))
        full = lambda o: dict(pose_rotvecs=x['pose'], shape_betas=o['shape_betas'], trans=o['trans'])  # noqa: E731
        fit_gate(om64, full(kp), full(ref['pose', '64']), full(ref['pose', '32']), f'smplx nb={nb} {form} known pose')
        ks = to_np(f.fit_with_known_shape(shape_betas=xd['betas'], target_vertices=xd['tv'], target_joints=xd['tj'], num_iter=2,
                                          requested_keys=['pose_rotvecs']))
        full = lambda o: dict(pose_rotvecs=o['pose_rotvecs'], shape_betas=x['betas'], trans=o['trans'])  # noqa: E731
        fit_gate(om64, full(ks), full(ref['shape', '64']), full(ref['shape', '32']), f'smplx nb={nb} {form} known shape')
