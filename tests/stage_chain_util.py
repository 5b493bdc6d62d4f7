"""The stages of a fit, one at a time, against the fp64 oracle of that stage alone — for the kernels that only run inside
a whole fit (the lane = instance k_rotations_bm / k_rotations_bm_rounds, k_prologue_bm, k_solve_bm, k_refine_bm and the
wave kernels behind them).  Plain numpy; used by tests/test_stage_chain_host.py (the fp32 oracle standing in for the
device) and tests/test_gpu_stage_chain.py.

Three fits expose every stage without an entry point of its own:
  fit(num_iter=1, final_adjust_rots=False)   orientations = the first rotation pass (R1); shape_betas / trans = the solve
                                             at those rotations (S1: prologue, GEMM, residual, solve)
  fit(num_iter=1)                            adds exactly the refinement (F): orientations
  fit(num_iter=2, final_adjust_rots=False)   adds exactly the second rotation pass (R2) and the solve at it (S2)
and each stage is compared with the oracle function of that stage (fit_global_rotations, fit_shape,
fit_global_rotations_dependent) evaluated AT THE OUTPUT OF THE STAGE BEFORE of the build under test — nothing is
amplified over iterations.  The model is posed at that state by the oracle's forward in the reference's own dtype; the
targets are centred as every entry point centres them (stage_util.centred).

The criteria are those of stage_util (rotation_figures / check_rotations with dist_gate, the per-pair floors from the fp32
oracle, the kappa factor of bone parts, toes as bit copies; check_solve): no tolerance of its own.  F and R2 compose a
delta rotation with the previous one: deficit and gap are taken on the delta against the stage's covariance, the distance
on the composed rotation."""

import numpy as np

import stage_util as S
import util

STEPS = ('R1', 'S1', 'F', 'R2', 'S2')

# (model, family, step) -> the share of (instance, part) pairs the fp64 oracle ALONE puts under a distance gate, where that
# is below stage_util.MIN_GATED: these are exempt from the share condition and from nothing else (deficit, properness and
# the distance gate on the pairs that are gated hold for every pair).  Measured by tests/test_stage_chain_host.py, which
# fails when a combination not listed here falls below the cap or a listed one no longer does.
# 'mirror' at the refinement: the delta covariance of an adjustable part of the reflected target is itself close to a
# reflection, and about half of the pairs have s2 - s3 <= 1e-2 s1.
SHARE_EXEMPT = {
    ('smpl', 'mirror', 'F'): 0.5375,
    ('smplxfat', 'mirror', 'F'): 0.425,
    ('smpl_w6', 'mirror', 'F'): 0.55,
}


class Case:
    """One family with the options of the three fits.  ``weights``: None, 'v' (the family's vertex weights alone: they
    enter the part sums, not the solve) or 'j' (its joint weights alone); ``warm``: dict(initial_pose_rotvecs,
    initial_shape_betas) or None."""

    def __init__(self, family, joints=True, reg=1.0, weights=None, warm=None):
        self.family, self.joints, self.reg, self.weights, self.warm = family, joints, float(reg), weights, warm

    def inputs(self, fam):
        return dict(tv=fam['tv'], tj=fam['tj'] if self.joints else None, vw=fam['vw'] if self.weights == 'v' else None,
                    jw=fam['jw'] if self.weights == 'j' else None)

    def fit_kwargs(self):
        return dict(beta_regularizer=self.reg, **(self.warm or {}))

    @property
    def tag(self):
        return (f'{"j" if self.joints else "nj"} reg{self.reg:g}' + (f' w={self.weights}' if self.weights else '') +
                (' warm' if self.warm else ''))


def warm_start(of64, fam):
    """A warm start near the answer: the fp64 oracle's one-iteration fit of the family, its pose rounded to 0.05 rad and
    its betas to 0.25."""
    r = of64.fit(fam['tv'], fam['tj'], num_iter=1)
    return dict(initial_pose_rotvecs=(np.round(r['pose_rotvecs'] / 0.05) * 0.05).astype(np.float32),
                initial_shape_betas=(np.round(r['shape_betas'] / 0.25) * 0.25).astype(np.float32))


class Refs:
    """The references of one (model, case) in one dtype (``of``: an OracleFitter, with the kid unknown or without)."""

    def __init__(self, of, fam, case):
        self.of, self.dt, self.case = of, of.m.dtype, case
        inp = case.inputs(fam)
        self.tv, self.tj, self.mean = S.centred(self.dt, inp['tv'], inp['tj'])
        w = lambda a: None if a is None else np.asarray(a, self.dt)  # noqa: E731
        self.vw, self.jw = w(inp['vw']), w(inp['jw'])
        self.inp = inp
        self._memo = {}
        self.reg_ref = None
        if case.warm is not None:
            self.reg_ref = np.zeros((self.tv.shape[0], of.S_all), np.float64)
            b0 = np.asarray(case.warm['initial_shape_betas'], np.float64)
            self.reg_ref[:, :b0.shape[1]] = b0

    def _once(self, what, arrays, compute):
        """Each reference is computed once per state (the stand-in chain of the host test asks for them twice)."""
        key = (what,) + tuple(hash(np.ascontiguousarray(a).tobytes()) for a in arrays)
        if key not in self._memo:
            self._memo[key] = compute()
        return self._memo[key]

    def R1(self):
        """(G, info, prev): the first rotation pass; prev is None, or the warm start's orientations it is composed with."""
        return self._once('R1', (), self._R1)

    def _R1(self):
        of = self.of
        if self.case.warm is None:
            G, info = S.oracle_rotations(of, self.inp)
            return G, info, None
        f = of.m.forward(pose_rotvecs=np.asarray(self.case.warm['initial_pose_rotvecs'], self.dt),
                         shape_betas=np.asarray(self.case.warm['initial_shape_betas'], self.dt))
        R, info = of.fit_global_rotations(self.tv, self.tj, f['vertices'], f['joints'], self.vw, self.jw, return_cov=True)
        return R @ f['orientations'], info, f['orientations']

    def solve(self, G):
        """fit_shape at the rotations ``G``: the dict stage_util.check_solve reads (the kid unknown, if any, as one more
        column of shape_betas: it is one more shape unknown under the same gate)."""
        return self._once('solve', (G,), lambda: self._solve(G))

    def _solve(self, G):
        r = self.of.fit_shape(np.asarray(G, self.dt), self.tv, self.tj, self.vw, self.jw, self.case.reg, 0.0,
                              reg_ref=self.reg_ref)
        out = {k: np.asarray(r[k], np.float64) for k in ('shape_betas', 'trans', 'vertices', 'joints')}
        if self.of.enable_kid:
            out['shape_betas'] = np.concatenate([out['shape_betas'], np.asarray(r['kid_factor'], np.float64)[:, None]], 1)
        return out

    def _posed(self, state):
        """The oracle's forward at a state (G, betas incl. the kid column, trans WITH the mean), centred frame."""
        return self._once('posed', state, lambda: self._posed_at(state))

    def _posed_at(self, state):
        G, beta_all, trans = (np.asarray(x, self.dt) for x in state)
        nb = self.of.m.S
        kid = beta_all[:, nb] if self.of.enable_kid else None
        tr = (trans - self.mean).astype(self.dt)
        f = self.of.m.forward(glob_rotmats=G, shape_betas=beta_all[:, :nb], trans=tr, kid_factor=kid)
        return G, beta_all, tr, f

    def F(self, state):
        """(G, info, prev) of the dependent refinement at ``state``."""
        return self._once('F', state, lambda: self._F(state))

    def _F(self, state):
        G, beta_all, tr, f = self._posed(state)
        R, info = self.of.fit_global_rotations_dependent(self.tv, self.tj, f['vertices'], f['joints'], self.vw, self.jw, G,
                                                         beta_all, tr, return_cov=True)
        return R, info, G

    def R2(self, state):
        """(G, info, prev) of the second rotation pass at ``state``."""
        return self._once('R2', state, lambda: self._R2(state))

    def _R2(self, state):
        G, _, _, f = self._posed(state)
        R, info = self.of.fit_global_rotations(self.tv, self.tj, f['vertices'], f['joints'] if self.tj is not None else None,
                                               self.vw, self.jw, return_cov=True)
        return R @ G, info, G


def state_of(out):
    """(G, betas incl. the kid column, trans) of a fit's result dict (numpy)."""
    b = out['shape_betas']
    if 'kid_factor' in out:
        b = np.concatenate([b, np.asarray(out['kid_factor']).reshape(-1, 1)], 1)
    return out['orientations'], b, out['trans']


def solved_mesh(om64, out):
    """What check_solve needs of a fit's result: the mesh and the joints at (orientations, shape_betas, kid_factor) by
    the fp64 forward — a fit does not return them —, in the centred frame convention of add_mean (trans carries the
    mean, vertices / joints are relative to trans - mean: here simply the mesh at zero translation)."""
    G, b, trans = state_of(out)
    nb = om64.S
    fw = util.forward64(om64, glob_rotmats=G, shape_betas=b[:, :nb], kid_factor=b[:, nb] if b.shape[1] > nb else None)
    return fw


def check_step_rotations(name, case, step, ours, r32, r64, label, rows=None):
    """One rotation stage of the build under test (``ours`` (B', J, 3, 3)) against the references (G, info, prev) of both
    dtypes; ``rows``: the reference row of each of our rows.  Parts the stage does not own keep the bits they had."""
    rows = np.arange(ours.shape[0]) if rows is None else np.asarray(rows)
    (G64, info, prev), G32 = r64, r32[0]
    info = {k: (v[rows] if isinstance(v, np.ndarray) and v.ndim > 1 else v) for k, v in info.items()}
    if step == 'F':
        adj = info['kind'] >= 0
        info['toes'] = [j for j in (10, 11) if j < len(adj) and not adj[j] and adj[j - 3]]
        kept = [j for j in np.nonzero(~adj)[0] if j not in info['toes']]
        assert np.array_equal(ours[:, kept], np.asarray(prev[rows][:, kept], ours.dtype)), (name, case.family, 'unadjusted parts changed')
    fig = S.rotation_figures(ours, G32[rows], G64[rows], info, S.dist_gate(name), prev=None if prev is None else prev[rows])
    S.check_rotations(name, case.family, fig, f'{label} {step} {case.tag}',
                      share_exempt=(name, case.family, step) in SHARE_EXEMPT)
    return fig


def check_step_solve(name, case, step, fw, out, s32, s64, mean64, label, rows=None):
    """One solve of the build under test (a fit's result dict, trans with the mean; ``fw``: solved_mesh of it) under
    stage_util.check_solve."""
    _, b, trans = state_of(out)
    trans = np.asarray(trans, np.float64)
    r = np.arange(len(trans)) if rows is None else np.asarray(rows)
    tc = trans - mean64[r]
    ours = dict(shape_betas=b, trans=trans, vertices=fw['vertices'] + tc[:, None], joints=fw['joints'] + tc[:, None])
    return S.check_solve(name, case.family, f'{step} {case.tag}', ours, s32, s64, mean64, True, label, rows=rows)


def joint_errors(out, s64, rows=None):
    """Per (row, joint): |joints - trans| against the fp64 solve (m) — the FK chains of k_prologue_bm joint by joint.
    ``out``: solved_mesh of a fit's result (zero translation) or a solve of Refs."""
    rel = out['joints'] - out['trans'][:, None] if 'trans' in out else out['joints']
    rows = np.arange(rel.shape[0]) if rows is None else np.asarray(rows)
    return np.linalg.norm(rel - (s64['joints'][rows] - s64['trans'][rows][:, None]), axis=-1)


def fitters(c, kid):
    """(fp64, fp32) OracleFitter of a stage_util.host_setup dict, with the kid unknown or without."""
    if not kid:
        return c['of64'], c['of32']
    if 'of_kid' not in c:
        c['of_kid'] = (util.O.OracleFitter(c['om64'], enable_kid=True), util.O.OracleFitter(c['om32'], enable_kid=True))
    return c['of_kid']


def check_chain(name, c, case, outs, label, rows=None, kid=False, r32=None, defer=()):
    """The five stages of the three fits ``outs`` (result dicts as numpy arrays: num_iter=1 without the final
    adjustment, num_iter=1, num_iter=2 without it) under the criteria above.  ``c``: stage_util.host_setup(name);
    ``rows``: the source row (of the family's B) of each row of the batch — every source row must occur, and the
    references are built at the state of its first occurrence; ``r32``: the fp32 Refs, if the caller has them; ``defer``: rotation
    steps whose AssertionError is not raised here but returned under figs['deferred'][step] — every other gate of the
    case still holds, and the caller raises the deferred one in a test of its own.  Returns step -> figures (plus
    'S1_joints': the per (row, joint) errors of S1 and the fp32 oracle's)."""
    fam = c['fams'][case.family]
    of64, of32 = fitters(c, kid)
    r64, r32 = Refs(of64, fam, case), r32 or Refs(of32, fam, case)
    o1, o2, o3 = outs
    fw1, fw3 = solved_mesh(c['om64'], o1), solved_mesh(c['om64'], o3)
    rows = np.arange(len(o1['trans'])) if rows is None else np.asarray(rows)
    first = [int(np.nonzero(rows == k)[0][0]) for k in range(S.B)]
    key = ('R1', case.family, case.joints, case.weights, case.warm is not None)
    if key not in c:  # (the first pass does not depend on the build under test, the kid unknown or the ridge)
        c[key] = (r64.R1(), r32.R1())
    figs = {'deferred': {}}

    def rotations(step, ours, a32, a64):
        try:
            figs[step] = check_step_rotations(name, case, step, ours, a32, a64, label, rows)
        except AssertionError as e:
            if step not in defer:
                raise
            figs['deferred'][step] = e

    rotations('R1', o1['orientations'], c[key][1], c[key][0])
    st1 = state_of({k: v[first] for k, v in o1.items()})
    s64, s32 = r64.solve(st1[0]), r32.solve(st1[0])
    figs['S1'] = check_step_solve(name, case, 'S1', fw1, o1, s32, s64, r64.mean, label, rows)
    e, e32 = joint_errors(fw1, s64, rows), joint_errors(s32, s64)[rows]
    bad = np.argwhere(e > np.maximum(S.MESH_GATE, 2 * e32))
    assert not len(bad), (name, case.family, 'S1 joints', [(int(b), int(j), float(e[b, j]), float(e32[b, j])) for b, j in bad])
    figs['S1_joints'] = (e, e32)
    for k in ('shape_betas', 'trans', 'kid_factor'):
        if k in o1:  # the refinement changes rotations only
            assert np.array_equal(o1[k], o2[k]), (name, case.family, k)
    rotations('F', o2['orientations'], r32.F(st1), r64.F(st1))
    rotations('R2', o3['orientations'], r32.R2(st1), r64.R2(st1))
    st3 = state_of({k: v[first] for k, v in o3.items()})
    figs['S2'] = check_step_solve(name, case, 'S2', fw3, o3, r32.solve(st3[0]), r64.solve(st3[0]), r64.mean, label, rows)
    return figs


def oracle_chain(refs):
    """The three fits by the step functions of one Refs, every result rounded to the oracle's dtype as a fit returns it:
    the stand-in for the device of tests/test_stage_chain_host.py."""
    dt, kid = refs.dt, refs.of.enable_kid
    nb = refs.of.m.S

    def result(G, s):
        out = dict(orientations=np.asarray(G, dt), shape_betas=s['shape_betas'][:, :nb].astype(dt),
                   trans=(s['trans'].astype(dt) + refs.mean).astype(dt))
        if kid:
            out['kid_factor'] = s['shape_betas'][:, nb].astype(dt)
        return out

    G1 = refs.R1()[0]
    o1 = result(G1, refs.solve(G1))
    o2 = dict(o1, orientations=np.asarray(refs.F(state_of(o1))[0], dt))
    G2 = refs.R2(state_of(o1))[0]
    return o1, o2, result(G2, refs.solve(G2))


def ancestors(parents):
    """Number of ancestors of each joint."""
    n = [0] * len(parents)
    for i in range(1, len(parents)):
        n[i] = n[parents[i]] + 1
    return np.array(n)
