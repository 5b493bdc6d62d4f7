"""The stages of a SCALED fit — fit(scale_target=True) / fit(scale_fit=True) and the same options of fit_with_known_pose —
one at a time against the fp64 oracle of that stage alone: the counterpart of tests/stage_chain_util.py and
tests/known_shape_chain_util.py for the code only a scale unknown reaches (k_accum_w_bm<.., EXTRAS> + k_accum_combine over
NE1 + 16 entries on the batch-major route, k_scale_extras<S, KW> on the wave route, k_shape_solve_scaled<false|true>,
k_scale_refs and the refinement behind it, and the unscaled solves of a scaled fit behind k_joint_stage + k_jd_transpose).
Plain numpy; used by tests/test_scale_chain_host.py (the host emulation, or the fp32 oracle, standing in for the device)
and tests/test_gpu_scale_chain.py.

Per option (scale_target, scale_fit) five calls expose every stage:
  SS0  fit_with_known_pose(<scale>) at the fp64 first-pass rotations      the scaled solve alone (also with share_beta)
  A    fit(num_iter=1, final_adjust_rots=False, <scale>)                  orientations = R1; betas / trans / scale_corr =
                                                                          the scaled solve at R1 (SS1)
  B    fit(num_iter=1, <scale>)                                           adds exactly k_scale_refs + the scaled
                                                                          refinement (F); the solve keeps A's bits
  D    fit(num_iter=1, final_adjust_rots=False), NO scale, on the route   the unscaled solve S1 — the state in front of
       a scaled call takes                                                C's second pass, which C does not return
  C    fit(num_iter=2, final_adjust_rots=False, <scale>)                  R2 (gated at D's state) and SS2 (at C's R2)
and every stage is compared with the oracle function of that stage (fit_global_rotations, fit_shape(scale_mode,
scale_reg), fit_global_rotations_dependent called as OracleFitter.fit calls it for the option) evaluated AT THE OUTPUT OF
THE STAGE BEFORE of the build under test.

Gates: nothing of its own.  Rotations: stage_util.rotation_figures / check_rotations with dist_gate (F and R2 as delta
rotations, as stage_chain_util judges them).  Solves: stage_util.check_solve — mesh and joints 1e-4 m, betas 3e-4 (the
kid unknown one more column), trans 1e-5, each max(gate, 2 x the fp32 oracle on that row); the translation WITH the mean
the entry point adds (fit: mean * s under scale_target, mean / s under scale_fit; fit_with_known_pose: the unscaled
mean), the row 1000 m away relative to max(1, |that mean|).  scale_corr: row by row max(SCALE_GATE, 2 x the fp32 oracle
on that row), the rule of known_shape_chain_util.  So that the floor cannot hide a failure, every solve also asserts
that the fp32 oracle's own distance stays within FLOOR_CAP x the fixed gate on every row (check_solve(cap=True))."""

import numpy as np

import stage_chain_util as C
import stage_util as S
import util
from smplfitter_amd import modelio

O = util.O
MODES = {'scale_target': 1, 'scale_fit': 2}
SCALE_GATE = 1e-5
FLOOR_CAP = 10.0
# per source row: the targets are the family's times this (factor 1: scale_corr is gated at 1 too; 1.1: the row the
# floor figures of DESIGN.md §5 were taken at)
FACTORS = np.array([1.0, 1.1, 0.8, 1.25, 0.9, 1.2, 0.85, 1.15], np.float32)
CALLS = dict(A=dict(num_iter=1, final_adjust_rots=False), B=dict(num_iter=1, final_adjust_rots=True),
             C=dict(num_iter=2, final_adjust_rots=False))
# name -> (the model whose setup it shares, num_betas where that is not 10, the kid unknown)
MODELS = {'smpl': ('smpl', None, False), 'smplxfat': ('smplxfat', None, False), 'smpl_w6': ('smpl_w6', None, False),
          'smpl_kid': ('smpl', None, True), 'smpl_b16': ('smpl_b16', 16, False), 'smpl_b16_kid': ('smpl_b16', 16, True),
          'smpl_b32': ('smpl_b32', 32, False)}

# (model, family, step) -> the share of (instance, part) pairs the fp64 oracle ALONE puts under a distance gate, where
# that is below stage_util.MIN_GATED, per option: exempt from the share condition and from nothing else.  By name only:
# every option of a family stands under one entry (the lowest share).  Measured by tests/test_scale_chain_host.py,
# which fails when a combination not listed here falls below the cap or a listed one no longer does.  'mirror' at the
# refinement: as stage_chain_util.SHARE_EXEMPT.
SHARE_EXEMPT = {  # (scale_target, scale_fit)
    ('smpl', 'mirror', 'F'): (0.6625, 0.5250),
    ('smplxfat', 'mirror', 'F'): (0.5125, 0.3375),
    ('smpl_w6', 'mirror', 'F'): (0.6375, 0.5375),
    ('smpl_kid', 'mirror', 'F'): (0.6125, 0.5250),
    ('smpl_b16', 'mirror', 'F'): (0.4750, 0.5125),
    ('smpl_b16_kid', 'mirror', 'F'): (0.5000, 0.5125),
}


def host_setup(name, model_root, golden):
    """stage_util.host_setup of the model ``name`` stands on (MODELS), plus ``md`` / ``kind`` for the host emulation;
    the models with 16 / 32 betas, which stage_util does not load, are set up here the same way."""
    base, nb, _ = MODELS[name]
    if nb is None:
        c = S.host_setup(base, model_root, golden)
        if 'md' not in c:
            c['kind'], c['md'] = util.load_md(model_root, base, golden(base))
        return c
    if base not in S._setups:
        md = modelio.load_model('smpl', 'neutral', model_root=f'{model_root}/{base}', num_betas=nb)
        om64, of64 = util.make_oracle(md, 'smpl', np.float64)
        om32, of32 = util.make_oracle(md, 'smpl', np.float32)
        S._setups[base] = dict(om64=om64, om32=om32, of64=of64, of32=of32, fams=S.families(om64, of64), md=md, kind='smpl')
    return S._setups[base]


class Case(C.Case):
    """One family with the options of the calls.  ``weights``: None, 'vj' (both: they enter the part sums AND the
    solve), 'v' (vertex weights alone: with target joints the part sums only, without them the solve too) or 'j'
    (joint weights alone: the rotations only); ``warm``: True for stage_chain_util.warm_start of the UNSCALED family
    (bound to the arrays by ``bound``); ``scale_reg``: scale_regularizer."""

    def __init__(self, family, joints=True, reg=1.0, weights=None, warm=None, scale_reg=0.0):
        super().__init__(family, joints=joints, reg=reg, weights=weights, warm=warm)
        self.scale_reg = float(scale_reg)

    def inputs(self, fam):
        w = self.weights or ''
        f = FACTORS[:, None, None]
        return dict(tv=np.ascontiguousarray(fam['tv'] * f, np.float32),
                    tj=np.ascontiguousarray(fam['tj'] * f, np.float32) if self.joints else None,
                    vw=fam['vw'] if 'v' in w else None, jw=fam['jw'] if 'j' in w else None)

    def fit_kwargs(self):
        return dict(beta_regularizer=self.reg, **(self.warm if isinstance(self.warm, dict) else {}))

    @property
    def tag(self):
        return (f'{"j" if self.joints else "nj"} reg{self.reg:g}' + (f' w={self.weights}' if self.weights else '') +
                (' warm' if self.warm else '') + (f' sreg{self.scale_reg:g}' if self.scale_reg else ''))

    @property
    def id(self):
        return f'{self.family}-{self.tag.replace(" ", "_")}'


def bound(c, case):
    """``case`` with its warm start as arrays (computed once per setup)."""
    if case.warm is not True:
        return case
    key = ('sc_warm', case.family)
    if key not in c:
        c[key] = C.warm_start(c['of64'], c['fams'][case.family])
    return Case(case.family, case.joints, case.reg, case.weights, c[key], case.scale_reg)


FULL = ('smpl', 'smplxfat')  # the models of both routes: every case


def ridge(name, family):
    """beta_regularizer of a model's cases.  With the kid unknown the scale column is close to a combination of the kid
    and the first shape direction (all three grow the body): under the default ridge of 1 the fp32 oracle's own
    scale_corr is up to 5.2e-4 from the fp64 one (17 unknowns, 'hard_pose'), outside FLOOR_CAP on most cases; under 10
    (which is the kid ridge too) it is inside on all but 'betas5' with 17 unknowns (2.1e-4), which takes 30 (7.3e-5).
    (measured at the fp64 first pass; tests/test_scale_chain_host.py holds every kept case to the cap)"""
    return 1.0 if not MODELS[name][2] else 30.0 if family in ('betas5', 'mirror') else 10.0


def few_cases(name='smpl'):
    """The cases of the batches that get four: plain, joints omitted, both weights, the row 1000 m away."""
    return [Case('hard_pose', reg=ridge(name, 'hard_pose')), Case('pose1', joints=False, reg=ridge(name, 'pose1')),
            Case('mask01', weights='vj', reg=ridge(name, 'mask01')), Case('far', reg=ridge(name, 'far'))]


def cases(name):
    """Every family and option of the chain on one model.  FULL models: the unmasked families ('betas5' under the ridge
    only: without it the fp32 oracle itself is outside FLOOR_CAP, tests/test_scale_chain_host.py); the masked ones with
    both weights, with vertex weights alone and with joint weights alone; joints omitted (k_scale_refs in its regressed
    form), plain and with vertex weights (which then do enter the solve); a warm start; scale_regularizer 0.5 with and
    without joints; no ridge (SMPL).  The wave-only instantiations (k_scale_extras<11, 4>, <10, 8>, <16, 4>, <17, 4>): the four
    of few_cases, 'mirror', 'betas5' and the warm start, under ridge(name, family)."""
    if name not in FULL:
        return few_cases(name) + [Case(f, reg=ridge(name, f)) for f in ('mirror', 'betas5')] + [Case('pose1', reg=ridge(name, 'pose1'), warm=True)]
    return ([Case(f) for f in S.UNMASKED] + [Case(f, weights=w) for f in S.MASKED for w in ('vj', 'v', 'j')] +
            [Case('pose1', joints=False), Case('mask01', joints=False, weights='v'), Case('pose1', warm=True),
             Case('pose1', scale_reg=0.5), Case('hard_pose', joints=False, scale_reg=0.5)] +
            # (no ridge: on the fat-part SMPL-X the fp32 oracle's scale_corr is 1.0e-4 .. 1.7e-4 off without one, at the cap)
            ([Case('pose1', joints=False, reg=0.0)] if name == 'smpl' else []))


def pose_of(G, parents):
    """pose_rotvecs (B, 3J) float32 of the global rotations ``G`` (fp64 arithmetic)."""
    G = np.asarray(G, np.float64)
    par = np.asarray(parents)
    Gpar = np.concatenate([np.broadcast_to(np.eye(3), (G.shape[0], 1, 3, 3)), G[:, par[1:]]], 1)
    return O.mat2rotvec(np.swapaxes(Gpar, -1, -2) @ G).reshape(G.shape[0], -1).astype(np.float32)


class Refs(C.Refs):
    """The references of one (model, case) in one dtype; ``rows``: the source row of each instance (default: the
    family's 8) — a shared solve sums over the batch, so its references are those of the whole tiled batch.  ``twin``:
    the fp64 Refs of the same case (the fp32 refinement starts from the fp64 solve's mesh, as the fp64 one does: the
    floor is the fp32 evaluation of THAT stage alone)."""

    def __init__(self, of, fam, case, rows=None, twin=None):
        super().__init__(of, fam, case)
        self.twin = twin or self
        if rows is not None:
            rows = np.asarray(rows)
            self.tv, self.mean = self.tv[rows], self.mean[rows]
            for k in ('tj', 'vw', 'jw', 'reg_ref'):
                if getattr(self, k) is not None:
                    setattr(self, k, getattr(self, k)[rows])

    def mean_out(self, s, mode, entry):
        """The mean the entry point adds to trans, in fp64 from this dtype's mean and scale."""
        mean, s = np.asarray(self.mean, np.float64), np.asarray(s, np.float64)[:, None]
        return mean if entry == 'known_pose' or not mode else mean * s if mode == 1 else mean / s

    def raw(self, G, mode, share=False, segments=None):
        """fit_shape at ``G`` in this dtype (centred frame), per segment of the batch where ``segments`` are given."""
        return self._once(('raw', mode, share, tuple(segments or ())), (G,), lambda: self._raw(G, mode, share, segments))

    def _raw(self, G, mode, share, segments):
        G = np.asarray(G, self.dt)
        sl = lambda a, i, j: None if a is None else a[i:j]  # noqa: E731
        ends = np.cumsum(segments or [len(G)])
        parts = [self.of.fit_shape(G[i:j], self.tv[i:j], sl(self.tj, i, j), sl(self.vw, i, j), sl(self.jw, i, j),
                                   self.case.reg, 0.0, reg_ref=sl(self.reg_ref, i, j), share_beta=share or bool(segments),
                                   scale_mode=mode, scale_reg=self.case.scale_reg)
                 for i, j in zip(np.concatenate([[0], ends[:-1]]), ends)]
        keys = ('shape_betas', 'trans', 'vertices', 'joints', 'beta_all') + (('scale_corr',) if mode else ())
        return {k: np.concatenate([np.asarray(p[k], np.float64) for p in parts]) for k in keys}

    def solve(self, G, mode, entry='fit', share=False, segments=None):
        """What check_solve reads: shape_betas (the kid unknown one more column), trans WITH the mean of the entry point,
        vertices / joints in that frame, scale_corr (ones without a scale), mean (the one added)."""
        r = self.raw(G, mode, share, segments)
        s = r['scale_corr'] if mode else np.ones(len(r['trans']))
        mean = self.mean_out(s, mode, entry)
        trans = np.asarray((r['trans'] + mean).astype(self.dt), np.float64)
        shift = (trans - r['trans'])[:, None]
        return dict(shape_betas=r['beta_all'], trans=trans, vertices=r['vertices'] + shift, joints=r['joints'] + shift,
                    scale_corr=s, mean=mean, trans_centred=r['trans'])

    def F(self, G, a, mode):
        """(G, info, prev) of the refinement behind the scaled solve: fit_global_rotations_dependent as the oracle's
        driver calls it for the option, at the outputs ``a`` of call A (shape_betas incl. the kid column, trans with the
        mean, scale_corr) and the mesh and joints of the fp64 fit_shape at ``G`` (evaluated at shape / scale under
        scale_fit), placed at A's translation."""
        return self._once(('F', mode), (G, a['shape_betas'], a['trans'], a['scale_corr']), lambda: self._F_scaled(G, a, mode))

    def _F_scaled(self, G, a, mode):
        dt = self.dt
        r = self.twin.raw(G, mode)
        G = np.asarray(G, dt)
        s = np.asarray(a['scale_corr'], dt)
        s3 = s[:, None, None]
        tr = (np.asarray(a['trans'], np.float64) - self.mean_out(s, mode, 'fit')).astype(dt)
        v = ((r['vertices'] - r['trans'][:, None]) + tr[:, None].astype(np.float64)).astype(dt)
        j = ((r['joints'] - r['trans'][:, None]) + tr[:, None].astype(np.float64)).astype(dt)
        beta = np.asarray(a['shape_betas'], dt)
        if mode == 1:
            R, info = self.of.fit_global_rotations_dependent(self.tv * s3, None if self.tj is None else self.tj * s3, v, j,
                                                             self.vw, self.jw, G, beta, tr, return_cov=True)
        else:
            shift = (1 - s3) * tr[:, None]
            R, info = self.of.fit_global_rotations_dependent(self.tv, self.tj, (s3 * v + shift).astype(dt), (s3 * j + shift).astype(dt),
                                                             self.vw, self.jw, G, beta, tr, scale_corr=s3, return_cov=True)
        return R, info, G


def refs(c, name, case, rows=None):
    """(fp64, fp32) Refs of a bound case, kept in ``c``: every build, route and batch under test shares their memo."""
    key = ('sc_refs', MODELS[name][2], case.id, None if rows is None else len(rows))
    if key not in c:
        of64, of32 = C.fitters(c, MODELS[name][2])
        fam = c['fams'][case.family]
        r64 = Refs(of64, fam, case, rows)
        c[key] = (r64, Refs(of32, fam, case, rows, twin=r64))
    return c[key]


def state_of(out):
    """dict(orientations, shape_betas incl. the kid column, trans, scale_corr (ones without the key)) of a result."""
    G, b, trans = C.state_of(out)
    return dict(orientations=G, shape_betas=b, trans=trans, scale_corr=out.get('scale_corr', np.ones(len(trans), np.float32)))


def solved_mesh(om64, st, mode):
    """The mesh and joints of a result at zero translation by the fp64 forward: at shape / scale under scale_fit, where
    the returned betas (and kid factor) stay undivided."""
    nb = om64.S
    b = np.asarray(st['shape_betas'], np.float64)
    if mode == 2:
        b = b / np.asarray(st['scale_corr'], np.float64)[:, None]
    return util.forward64(om64, glob_rotmats=st['orientations'], shape_betas=b[:, :nb], kid_factor=b[:, nb] if b.shape[1] > nb else None)


def check_solve(name, case, step, om64, out, mode, a32, a64, label, rows=None, cap=True):
    """One scaled solve of the build under test (a result dict, numpy) under stage_util.check_solve plus the scale_corr
    rule; ``a32`` / ``a64``: Refs.solve of both dtypes.  ``cap``: also the floor condition (module docstring)."""
    st = state_of(out)
    n = len(st['trans'])
    rows = np.arange(n) if rows is None else np.asarray(rows)
    assert ('scale_corr' in out) == bool(mode), (name, case.id, step)
    fw = solved_mesh(om64, st, mode)
    trans = np.asarray(st['trans'], np.float64)
    ours = dict(shape_betas=st['shape_betas'], trans=trans, vertices=fw['vertices'] + trans[:, None], joints=fw['joints'] + trans[:, None])
    four = lambda r: {k: r[k] for k in ours}  # noqa: E731
    tag = f'{step} {case.tag}'
    if len(a64['trans']) != S.B:  # the references of a shared solve are those of the whole batch, row for row
        assert len(a64['trans']) == n and case.family != 'far', (name, case.id, step)
        rows = np.arange(n)
    fig = S.check_solve(name, case.family, tag, ours, four(a32), four(a64), a64['mean'], False, label, rows=rows)
    es = np.abs(np.asarray(st['scale_corr'], np.float64) - a64['scale_corr'][rows])
    es32 = np.abs(a32['scale_corr'] - a64['scale_corr'])[rows]
    fig.update(scale=float(es.max()), scale32=float(es32.max()))
    print(f'[scale {label}] {name:12s} {case.family:9s} {tag:24s} scale_corr {fig["scale"]:.2e} ({fig["scale32"]:.2e})')
    if mode:
        assert np.isfinite(es).all(), (name, case.id, step)
        bad = np.nonzero(es > np.maximum(SCALE_GATE, 2 * es32))[0]
        assert not len(bad), (name, case.id, step, 'scale_corr', [(int(i), float(es[i]), float(es32[i])) for i in bad])
    if cap:
        # (the translation in the centred frame: with the mean it carries mean * (the error of scale_corr), which the
        # scale entry of the cap bounds already — at a mean of 1 .. 2 m that alone is up to 2e-4 m)
        far = (rows == S.FAR_ROW) & (case.family == 'far')
        rel = np.where(far, np.maximum(1.0, np.abs(a64['mean'][rows]).max(-1)), 1.0)
        fig['trans_c32'] = float((np.abs(a32['trans_centred'] - a64['trans_centred']).max(1)[rows] / rel).max())
        gates = dict(mesh=S.MESH_GATE, joints=S.MESH_GATE, betas=S.BETA_GATE, trans_c=S.TRANS_GATE, scale=SCALE_GATE)
        over = {k: fig[k + '32'] for k, g in gates.items() if fig[k + '32'] > FLOOR_CAP * g}
        assert not over, (name, case.id, step, 'the fp32 oracle itself is outside the floor cap', over)
    return fig


def check_rotations(name, case, step, ours, r32, r64, label, rows):
    """One rotation stage as stage_chain_util.check_step_rotations judges it, under THIS chain's share exemptions."""
    (G64, info, prev), G32 = r64, r32[0]
    info = {k: (v[rows] if isinstance(v, np.ndarray) and v.ndim > 1 else v) for k, v in info.items()}
    if step == 'F':
        adj = info['kind'] >= 0
        info['toes'] = [j for j in (10, 11) if j < len(adj) and not adj[j] and adj[j - 3]]
        kept = [j for j in np.nonzero(~adj)[0] if j not in info['toes']]
        assert np.array_equal(ours[:, kept], np.asarray(prev[rows][:, kept], ours.dtype)), (name, case.family, 'unadjusted parts changed')
    fig = S.rotation_figures(ours, G32[rows], G64[rows], info, S.dist_gate(name), prev=None if prev is None else prev[rows])
    try:
        S.check_rotations(name, case.family, fig, f'{label} {step} {case.tag}', share_exempt=(name, case.family, step) in SHARE_EXEMPT)
    except AssertionError as e:
        e.fig = fig
        raise
    return fig


def check_chain(name, c, case, mode, outs, label, rows=None, defer=(), cap=True):
    """The stages of the calls ``outs`` — dict(A, B, C, D[, SS0]) of result dicts as numpy arrays, for ONE option
    ``mode`` (MODES) — under the criteria above.  ``c``: host_setup(name); ``case``: bound; ``rows``: the source row of
    each row of the batch (every source row must occur; the references are built at the state of its first occurrence).
    ``defer``: steps whose AssertionError is returned under figs['deferred'][step] instead of raised, as
    stage_chain_util.check_chain defers them.  Returns step -> figures."""
    r64, r32 = refs(c, name, case)
    A, Bc, Cc, D = (outs[k] for k in 'ABCD')
    rows = np.arange(len(A['trans'])) if rows is None else np.asarray(rows)
    first = np.array([int(np.nonzero(rows == k)[0][0]) for k in range(S.B)])
    at = lambda o: {k: v[first] for k, v in state_of(o).items()}  # noqa: E731
    om64, figs = c['om64'], {'deferred': {}}

    def step(key, check, *a, **kw):
        try:
            figs[key] = check(name, case, key, *a, **kw)
        except AssertionError as e:
            if key not in defer:
                raise
            figs['deferred'][key] = e
            if hasattr(e, 'fig'):
                figs[key] = e.fig

    if 'SS0' in outs:
        G0 = outs['SS0']['orientations'][first]
        step('SS0', check_solve, om64, outs['SS0'], mode, r32.solve(G0, mode, 'known_pose'), r64.solve(G0, mode, 'known_pose'),
             label, rows, cap=cap)
    # R1 does not see the scale unknown: the unscaled call on the same route returns the same bits
    assert np.array_equal(A['orientations'], D['orientations']), (name, case.id, 'A and D differ in R1')
    assert 'scale_corr' not in D, (name, case.id)
    step('R1', check_rotations, A['orientations'], r32.R1(), r64.R1(), label, rows)
    a = at(A)
    G1 = a['orientations']
    step('SS1', check_solve, om64, A, mode, r32.solve(G1, mode), r64.solve(G1, mode), label, rows, cap=cap)
    for k in ('shape_betas', 'trans', 'scale_corr', 'kid_factor'):  # k_scale_refs copies back what the solve returned
        assert (k in A) == (k in Bc) and (k not in A or np.array_equal(A[k], Bc[k])), (name, case.id, k)
    step('F', check_rotations, Bc['orientations'], r32.F(G1, a, mode), r64.F(G1, a, mode), label, rows)
    d = at(D)
    st1 = (d['orientations'], d['shape_betas'], d['trans'])
    step('R2', check_rotations, Cc['orientations'], r32.R2(st1), r64.R2(st1), label, rows)
    G2 = Cc['orientations'][first]
    step('SS2', check_solve, om64, Cc, mode, r32.solve(G2, mode), r64.solve(G2, mode), label, rows, cap=cap)
    return figs


def gated_shares(name, case, figs):
    """(model, family, step) -> the gated share of the case's rotation steps."""
    return {(name, case.family, k): fig['gated_share'] for k, fig in figs.items() if k in ('R1', 'F', 'R2')}


def fit_options(case, mode):
    """The keyword arguments every call of a case shares (host emulation and device alike)."""
    return dict(scale_target=mode == 1, scale_fit=mode == 2, scale_regularizer=case.scale_reg) if mode else {}


KEYS = ('orientations', 'shape_betas', 'trans', 'kid_factor', 'scale_corr')


def host_chain(c, name, case, mode, H):
    """A, B, C, D of a bound case through the host emulation ``H`` (tests/hostemu_util.py: fit_warm), B = stage_util.B."""
    inp, kid = case.inputs(c['fams'][case.family]), MODELS[name][2]
    call = lambda o, m: {k: v for k, v in H.fit_warm(  # noqa: E731
        c['md'], c['kind'], inp['tv'], inp['tj'], inp['vw'], inp['jw'], enable_kid=kid, **case.fit_kwargs(), **o,
        **fit_options(case, m)).items() if k in KEYS}
    return dict(A=call(CALLS['A'], mode), B=call(CALLS['B'], mode), C=call(CALLS['C'], mode), D=call(CALLS['A'], 0))


def oracle_chain(c, name, case, mode):
    """The same calls, and SS0, by the fp32 oracle's own entry points: the stand-in where the emulation has no instance
    (more than 17 shape unknowns) and for fit_with_known_pose, which it does not emulate."""
    r64, _ = refs(c, name, case)
    of32 = C.fitters(c, MODELS[name][2])[1]
    inp = case.inputs(c['fams'][case.family])
    kw = dict(vertex_weights=inp['vw'], joint_weights=inp['jw'], **case.fit_kwargs())
    fit = lambda o, m: {k: np.asarray(v) for k, v in of32.fit(inp['tv'], inp['tj'], **kw, **o, **fit_options(case, m)).items() if k in KEYS}  # noqa: E731
    return dict(A=fit(CALLS['A'], mode), B=fit(CALLS['B'], mode), C=fit(CALLS['C'], mode), D=fit(CALLS['A'], 0),
                SS0=known_pose_oracle(c, name, case, mode))


def known_pose_oracle(c, name, case, mode, share=False):
    """SS0 by the fp32 oracle's fit_with_known_pose at the fp64 first-pass rotations."""
    r64, _ = refs(c, name, case)
    of32 = C.fitters(c, MODELS[name][2])[1]
    inp = case.inputs(c['fams'][case.family])
    kw = {k: v for k, v in case.fit_kwargs().items() if k == 'beta_regularizer'}
    if isinstance(case.warm, dict):
        kw['beta_regularizer_reference'] = case.warm['initial_shape_betas']
    r = of32.fit_with_known_pose(pose_of(r64.R1()[0], c['om64'].parents), inp['tv'], inp['tj'], inp['vw'], inp['jw'],
                                 share_beta=share, **kw, **fit_options(case, mode))
    return {k: np.asarray(v) for k, v in r.items() if k in KEYS}
