"""Host checks of the differentiable ``BodyFitter.fit`` (no GPU): the fp64 arbiter (tests/fit_grad_util.py: ``TorchFit`` in
fp64) against the reference's own fp32 autograd gradients (tests/golden/golden_fit_grad.npz), the new ``SF_HD`` functions
of csrc/sf_math.h / csrc/sf_stages.h built with g++ (tests/hostemu/hostemu_fit_adjoint.cpp) against that arbiter stage
by stage, and the new C-ABI symbols."""

import ctypes as C
import os
import os.path as osp
import subprocess

import numpy as np
import pytest
import torch

import fit_grad_util as fu
import hostemu_util
import util
from test_known_pose_grad_host import GRAD_REL

HERE = osp.dirname(osp.abspath(__file__))
GOLDEN = osp.join(HERE, 'golden', 'golden_fit_grad.npz')
SRC = osp.join(HERE, 'hostemu', 'hostemu_fit_adjoint.cpp')
SO = osp.join(HERE, 'hostemu', '_build', 'libhostemu_fit_adjoint.so')
CSRC = osp.join(HERE, '..', 'smplfitter_amd', 'csrc')
# twice the largest relative error (max |reference fp32 - fp64| / max |fp64|) tests/golden/make_golden_fit_grad.py
# printed per tensor kind over its nine cases
REF_REL = dict(target_vertices=2 * 7.0e-5, target_joints=2 * 3.0e-5, vertex_weights=2 * 3.8e-4, joint_weights=2 * 2.3e-3)


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLDEN)


def reference_errors(gold, tag, case, grads, V):
    """max |reference fp32 - fp64| per gradient tensor of a fixture case (vertex-sized tensors on the stored subset)."""
    sub = fu.subset(V)
    p = f'{tag}.{case}.'
    return {k: float(np.abs((v[:, sub] if k in ('target_vertices', 'vertex_weights') else v) - gold[p + 'g32.' + k]).max())
            for k, v in grads.items()}


@pytest.mark.parametrize('tag,case', [(t, c) for t, cs in fu.FIXTURE_CASES.items() for c in cs])
def test_arbiter_matches_reference(gold, tag, case, model_root, golden):
    """The fp64 arbiter reproduces the reference's fp32 autograd gradients of ``fit``.  Gate per tensor kind, relative to
    max |fp64|: twice the largest value the fixture's generator printed over its nine cases — target_vertices 7.0e-5,
    target_joints 3.0e-5, vertex_weights 3.8e-4 (all three on SMPL-X-fat A; SMPL alone: 3.7e-5, 2.2e-5, 2.6e-4) and
    joint_weights 2.3e-3 (SMPL-X-fat C, a gradient of order 1e-4; SMPL: 8.5e-5); these are the reference's fp32
    roundings and move with the seed, hence the factor 2."""
    g = golden(tag)
    x, kw, kid = fu.case_inputs(g, case, 2)
    p = f'{tag}.{case}.'
    J = g['target_joints'].shape[1]
    cot = fu.cotangents(int(gold[p + 'seed']), 2, J, 10, kid)
    out, grads = fu.arbiter(fu.torchfit64(model_root, tag, g, kid), x, kw, cot)
    assert set(grads) == {k[len(p) + 4:] for k in gold.files if k.startswith(p + 'g32.')}
    for k in cot:
        tol = 2e-3 if k == 'pose_rotvecs' else 2e-4  # (the reference's fp32 fit against fp64; pose: tests/util.py pose_tol)
        assert np.abs(out[k] - gold[p + 'out.' + k]).max() <= tol, (tag, case, k)
    err = reference_errors(gold, tag, case, grads, g['target_vertices'].shape[1])
    for k, v in grads.items():
        print(f'[fit-grad] arbiter {tag} {case} {k} ref-vs-fp64 {err[k]:.2e} max {np.abs(v).max():.2e} rel {err[k] / np.abs(v).max():.2e}')
        assert err[k] <= REF_REL[k] * np.abs(v).max(), (tag, case, k, err[k])


# ---- the SF_HD functions, stage by stage ----------------------------------------------------------------------------
def _lib():
    deps = [SRC] + [osp.join(CSRC, f) for f in ('sf_math.h', 'sf_stages.h', 'sf_tables.h', 'sf_tables.cpp')]
    if not osp.exists(SO) or any(osp.getmtime(d) > osp.getmtime(SO) for d in deps):
        os.makedirs(osp.dirname(SO), exist_ok=True)
        tmp = SO + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', SRC,
                        osp.join(CSRC, 'sf_tables.cpp'), '-o', tmp], check=True)
        os.replace(tmp, SO)
    return C.CDLL(SO)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a.detach().numpy() if isinstance(a, torch.Tensor) else a, np.float32)


def _close(tag, ours, ref, rel=GRAD_REL):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref
    e, m = np.abs(ours - ref).max(), np.abs(ref).max()
    print(f'[fit-grad] host {tag} ours-vs-fp64 {e:.2e} max {m:.2e} rel {e / max(m, 1e-300):.2e}')
    assert np.all(np.isfinite(ours)) and e <= rel * m, (tag, e, m)


def test_host_projection_adjoint():
    """sf::proj_so3_adjoint against autograd through the SVD form (pt/_autograd.py proj_so3) in fp64, on matrices of
    both determinant signs; inputs rounded to fp32 first (the forward's proj_so3 reads fp32).  Reaches 3e-8 of max
    |gradient| for positive and 1.4e-7 for negative determinants (the fp32 rounding of R); gate 1e-5."""
    from smplfitter_amd.pt._autograd import proj_so3

    rs = np.random.RandomState(0)
    A = rs.randn(64, 3, 3).astype(np.float32)
    A[1::2] *= -np.sign(np.linalg.det(A[1::2]))[:, None, None]  # odd rows: negative determinant
    A[0::2] *= np.sign(np.linalg.det(A[0::2]))[:, None, None]
    Rbar = rs.randn(64, 3, 3)
    At = torch.tensor(A.astype(np.float64), requires_grad=True)
    (proj_so3(At) * torch.tensor(Rbar)).sum().backward()
    R, Abar = np.zeros((64, 3, 3), np.float32), np.zeros((64, 3, 3))
    _lib().hostemu_fa_proj(_p(A), _p(Rbar), _p(R), _p(Abar), 64)
    for sign, rows in (('+', slice(0, None, 2)), ('-', slice(1, None, 2))):
        _close(f'projection det{sign}', Abar[rows], At.grad[rows], 1e-5)


class _Stage:
    """Inputs of the stage checks from SMPL case C (fp64 tensors, centred): the targets, the first rotations G0, the
    solve at G0 with its mesh and joints."""

    def __init__(self, model_root, golden, joints=True):
        g = golden('smpl')
        _, self.md = util.load_md(model_root, 'smpl', g)
        x, kw, _ = fu.case_inputs(g, 'C', 2)
        self.tf = tf = fu.torchfit64(model_root, 'smpl', g, False)
        self.c = c = tf._consts(torch.device('cpu'))
        t = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64))  # noqa: E731
        tv, tj, self.vw, self.jw = (t(x[k]) for k in fu.TENSORS)
        mean = torch.cat([tv, tj], 1).mean(1) if joints else tv.mean(1)
        self.tv, self.tj = tv - mean[:, None], (tj - mean[:, None]) if joints else None
        self.reg = c['J_regressor_post_lbs']
        with torch.no_grad():
            self.G0 = tf._rotations(c, self.tv, self.tj, c['default_mesh'][None], c['J_template'][None], self.vw, self.jw)
            r = tf._shape(c, self.G0, self.tv, self.tj, self.vw, self.jw, 1.0, 0.5, None)
        self.rv, self.rj, self.beta, self.trans = r['vertices'], r['joints'], r['beta_all'], r['trans']
        self.desc, self.keep = hostemu_util.desc_from_md(self.md, 'smpl', False)
        self.B, self.V, self.J = 2, tv.shape[1], tj.shape[1]


@pytest.mark.parametrize('form', ['next', 'first', 'regressed'])
def test_host_rotation_pass_adjoint(form, model_root, golden):
    """sf::fit_rot_adjoint + sf::partsum_vertex_adjoint (one lane, fp32 part sums) against fp64 autograd through
    ``TorchFit._rotations``: a later pass composed with the previous rotations, the first pass against the template, and
    a pass without target joints (both joint sets regressed; their cotangents return through the regressor's transpose).
    Gate GRAD_REL of max |fp64| per tensor.  Reaches: target and reference points, joints and the previous rotations
    <= 8e-7, vertex and joint weights <= 6.4e-6 (with fp32 part sums and the expanded four-term vertex form: 1.5e-4 and
    8e-4)."""
    s = _Stage(model_root, golden, joints=form != 'regressed')
    tf, c, B, V, J = s.tf, s.c, s.B, s.V, s.J
    first = form == 'first'
    rv0, rj0 = (c['default_mesh'][None], c['J_template'][None]) if first else (s.rv, s.rj)
    leaf = lambda a: a.clone().requires_grad_()  # noqa: E731
    tv, vw, jw, rv = leaf(s.tv), leaf(s.vw), leaf(s.jw), leaf(rv0)
    tj = leaf(s.tj) if s.tj is not None else None
    rj = leaf(rj0) if s.tj is not None else None
    Gprev = None if first else leaf(s.G0)
    cotG = torch.tensor(np.random.RandomState(1).randn(B, J, 3, 3))
    out = tf._rotations(c, tv, tj, rv, rj, vw, jw)
    if Gprev is not None:
        out = out @ Gprev
    (out * cotG).sum().backward()
    # the joints the stage reads
    tj_in = tj.detach() if tj is not None else torch.einsum('jv,bvc->bjc', s.reg, s.tv)
    rj_in = rj.detach() if rj is not None else torch.einsum('jv,bvc->bjc', s.reg, rv0.expand(1 if first else B, -1, -1))
    a = dict(tv=_f32(s.tv), tj=_f32(tj_in), rv=_f32(rv0), rj=_f32(rj_in), vw=_f32(s.vw), jw=_f32(s.jw),
             Gprev=None if first else _f32(s.G0), Gbar=_f32(cotG))
    z = lambda *sh: np.zeros(sh, np.float32)  # noqa: E731
    o = dict(Gout=z(B, J, 3, 3), g_tv=z(B, V, 3), g_rv=z(B, V, 3), g_vw=z(B, V), g_tj=z(B, J, 3), g_rj=z(B, J, 3),
             g_jw=z(B, J), g_Gprev=z(B, J, 3, 3))
    rc = _lib().hostemu_fa_rot(C.byref(s.desc), B, _p(a['tv']), _p(a['tj']), _p(a['rv']), _p(a['rj']), int(first),
                               _p(a['vw']), _p(a['jw']), _p(a['Gprev']), _p(a['Gbar']), *(_p(o[k]) for k in o))
    assert rc == 0
    _close(f'rot {form} G', o['Gout'], out, 1e-3)  # (the fp32 forward against fp64: tests/util.py pose_tol)
    g_tv, g_rv = o['g_tv'].astype(np.float64), o['g_rv'].astype(np.float64)
    if tj is None:
        regn = s.reg.numpy()
        g_tv += np.einsum('jv,bjc->bvc', regn, o['g_tj'])
        g_rv += np.einsum('jv,bjc->bvc', regn, o['g_rj'])
    else:
        _close(f'rot {form} target_joints', o['g_tj'], tj.grad)
        _close(f'rot {form} joint_weights', o['g_jw'], jw.grad)
        if not first:
            _close(f'rot {form} reference joints', o['g_rj'], rj.grad)
    _close(f'rot {form} target_vertices', g_tv, tv.grad)
    _close(f'rot {form} vertex_weights', o['g_vw'], vw.grad)
    if not first:
        _close(f'rot {form} reference vertices', g_rv, rv.grad)
        _close(f'rot {form} previous rotations', o['g_Gprev'], Gprev.grad)


@pytest.mark.parametrize('form', ['joints', 'regressed', 'plain'])
def test_host_refinement_adjoint(form, model_root, golden):
    """sf::fit_tail_adjoint (the output stage: log map, relative rotations, orientations; the dependent refinement in
    reverse tree order) + sf::partsum_vertex_adjoint against fp64 autograd through ``TorchFit._refine`` and the output
    stage of ``TorchFit.fit``, with and without target joints, and with the refinement off ('plain': the output stage
    alone).  Gate GRAD_REL of max |fp64| per tensor.  Reaches: <= 1.6e-6 on points, joints,
    rotations, shape and trans, <= 1.2e-5 on the weights; the output stage alone 3.5e-8."""
    from smplfitter_amd.pt._autograd import mat2rotvec

    s = _Stage(model_root, golden, joints=form != 'regressed')
    tf, c, B, V, J = s.tf, s.c, s.B, s.V, s.J
    refine = form != 'plain'
    leaf = lambda a: a.clone().requires_grad_()  # noqa: E731
    tv, vw, jw, rv, rjt = leaf(s.tv), leaf(s.vw), leaf(s.jw), leaf(s.rv), leaf(s.rj)
    tj = leaf(s.tj) if s.tj is not None else None
    G, beta, trans = leaf(s.G0), leaf(s.beta), leaf(s.trans)
    Gf = tf._refine(c, tv, tj, rv, rjt, vw, jw, G, beta, trans) if refine else G
    eye = torch.eye(3, dtype=torch.float64).expand(B, 1, 3, 3)
    rel = torch.cat([eye, Gf[:, tf.par[1:]]], 1).transpose(-1, -2) @ Gf
    rs = np.random.RandomState(2)
    cp, co, cr = rs.randn(B, J, 3), rs.randn(B, J, 3, 3), rs.randn(B, J, 3, 3)
    ((mat2rotvec(rel) * torch.tensor(cp)).sum() + (Gf * torch.tensor(co)).sum() + (rel * torch.tensor(cr)).sum()).backward()
    tj_in = tj.detach() if tj is not None else torch.einsum('jv,bvc->bjc', s.reg, s.tv)
    rjterm = s.rj if tj is not None else torch.einsum('jv,bvc->bjc', s.reg, s.rv)
    z = lambda *sh: np.zeros(sh, np.float32)  # noqa: E731
    a = [_f32(v) for v in (s.G0, s.beta, s.trans, s.tv, tj_in, s.rv, rjterm, s.rj, s.vw, s.jw)]
    o = dict(Gbar=z(B, J, 3, 3), xbar=z(B, 10), tbar=z(B, 3), g_tv=z(B, V, 3), g_rv=z(B, V, 3), g_vw=z(B, V),
             g_tj=z(B, J, 3), g_rjt=z(B, J, 3), g_rj=z(B, J, 3), g_jw=z(B, J))
    cots = [_f32(cp), _f32(co), _f32(cr)]
    rc = _lib().hostemu_fa_tail(C.byref(s.desc), B, *(_p(v) for v in a), int(refine), *(_p(v) for v in cots),
                                *(_p(o[k]) for k in o))
    assert rc == 0
    _close(f'tail {form} rotations', o['Gbar'], G.grad)
    if not refine:
        assert not o['g_tv'].any() and not o['xbar'].any() and not o['tbar'].any()
        return
    _close(f'tail {form} shape', o['xbar'], beta.grad)
    _close(f'tail {form} trans', o['tbar'], trans.grad)
    g_tv, g_rv = o['g_tv'].astype(np.float64), o['g_rv'].astype(np.float64)
    if tj is None:
        regn = s.reg.numpy()
        g_tv += np.einsum('jv,bjc->bvc', regn, o['g_tj'])
        g_rv += np.einsum('jv,bjc->bvc', regn, o['g_rjt'])
        _close(f'tail {form} solve joints', o['g_rj'], rjt.grad)
    else:
        _close(f'tail {form} target_joints', o['g_tj'], tj.grad)
        _close(f'tail {form} solve joints', o['g_rj'] + o['g_rjt'], rjt.grad)
    _close(f'tail {form} joint_weights', o['g_jw'], jw.grad)
    _close(f'tail {form} target_vertices', g_tv, tv.grad)
    _close(f'tail {form} reference vertices', g_rv, rv.grad)
    _close(f'tail {form} vertex_weights', o['g_vw'], vw.grad)


def test_host_centring():
    """The centring step: the gradient of f(points - mean) + g_trans . mean, against autograd in fp64."""
    rs = np.random.RandomState(3)
    n = 1000
    gp, gt = rs.randn(n, 3).astype(np.float32), rs.randn(3).astype(np.float32)
    pts = torch.tensor(rs.randn(n, 3), requires_grad=True)
    mean = pts.mean(0)
    (((pts - mean) * torch.tensor(gp.astype(np.float64))).sum() + (mean * torch.tensor(gt.astype(np.float64))).sum()).backward()
    ours = gp.copy()
    _lib().hostemu_fa_uncenter(_p(ours), n, _p(gt))
    _close('centring', ours, pts.grad, 1e-6)


def test_abi_symbols():
    from smplfitter_amd import _lib as L

    assert L.SMPLFIT_ABI_VERSION == 7
    for s in ('smplfit_fit_backward_workspace_bytes', 'smplfit_fit_backward_f32'):
        assert s in L.EXPORTED_SYMBOLS
    hdr = open(osp.join(HERE, '..', 'include', 'smplfit.h')).read()
    assert '#define SMPLFIT_ABI_VERSION 7' in hdr
    for s in ('smplfit_fit_backward_args', 'smplfit_fit_backward_workspace_bytes(', 'smplfit_fit_backward_f32('):
        assert s in hdr
    # every field of the struct is bound, in the header's order, and the mirror has the header's size
    body = hdr[hdr.index('typedef struct smplfit_fit_backward_args {'):hdr.index('} smplfit_fit_backward_args;')]
    names = []
    for line in body.splitlines()[1:]:
        decl = line.split('/*')[0].strip().rstrip(';')
        if decl:
            names += [n.strip().lstrip('*').strip() for n in decl.split(' ', 1 if not decl.startswith('const') else 2)[-1].split(',')]
    assert names == [f[0] for f in L.FitBackwardArgs._fields_], names
    src = osp.join(HERE, 'hostemu', '_build', 'sizeof_fit_backward_args.c')
    os.makedirs(osp.dirname(src), exist_ok=True)
    with open(src, 'w') as fh:
        fh.write('#include <stdio.h>\n#include "smplfit.h"\nint main(void) { printf("%zu", sizeof(smplfit_fit_backward_args)); return 0; }\n')
    exe = src[:-2]
    subprocess.run(['gcc', '-I', osp.join(HERE, '..', 'include'), src, '-o', exe], check=True)
    assert int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout) == C.sizeof(L.FitBackwardArgs)
