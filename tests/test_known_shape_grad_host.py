"""Host checks of the differentiable ``BodyFitter.fit_with_known_shape`` (no GPU): ``TorchFit.fit_with_known_shape``
against the reference's ``knownshape.*`` fixtures (fp32) and, in fp64 (the arbiter, tests/known_shape_grad_util.py),
against the reference's own fp32 autograd gradients (tests/golden/golden_known_shape_grad.npz); the new ``SF_HD``
functions of csrc/sf_stages.h built with g++ (tests/hostemu/hostemu_known_shape_adjoint.cpp) against that arbiter's
stages; and the new C-ABI symbols."""

import ctypes as C
import os
import os.path as osp
import subprocess

import numpy as np
import pytest
import torch

import known_shape_grad_util as ku
import util
from test_fit_grad_host import _Stage, _f32, _p
from test_known_pose_grad_host import GRAD_REL

HERE = osp.dirname(osp.abspath(__file__))
GOLDEN = osp.join(HERE, 'golden', 'golden_known_shape_grad.npz')
SRC = osp.join(HERE, 'hostemu', 'hostemu_known_shape_adjoint.cpp')
SO = osp.join(HERE, 'hostemu', '_build', 'libhostemu_known_shape_adjoint.so')
CSRC = osp.join(HERE, '..', 'smplfitter_amd', 'csrc')
# twice the largest relative error (max |reference fp32 - fp64| / max |fp64|) tests/golden/make_golden_known_shape_grad.py
# printed per tensor kind over its nine cases.  joint_weights: a known-shape fit whose target joints are a posed model's
# has a joint-weight gradient of order 1e-7 .. 1e-4 (the joints of a part agree on its rotation, whatever their weights):
# the reference's fp32 value of it is rounding noise, up to 150 times the fp64 one.
REF_REL = dict(shape_betas=2 * 3.8e-5, kid_factor=2 * 2.7e-6, target_vertices=2 * 4.5e-5, target_joints=2 * 3.6e-5,
               vertex_weights=2 * 1.3e-3, joint_weights=2 * 1.5e2)


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLDEN)


def reference_errors(gold, tag, case, grads, V):
    """max |reference fp32 - fp64| per gradient tensor of a fixture case (vertex-sized tensors on the stored subset)."""
    sub = ku.subset(V)
    p = f'{tag}.{case}.'
    return {k: float(np.abs((v[:, sub] if k in ku.VERTEX_SIZED else v) - gold[p + 'g32.' + k]).max()) for k, v in grads.items()}


@pytest.mark.parametrize('name', ['smpl', 'smplx'])
def test_torchfit_matches_reference_fixture(name, model_root, golden):
    """``TorchFit.fit_with_known_shape`` in fp32 reproduces the reference's ``knownshape.*`` fixtures of the cases
    without ``scale_fit`` and without a warm start (a, b, f), within the gate of ``util.check_known_shape``."""
    from smplfitter_amd.pt import BodyModel
    from smplfitter_amd.pt._autograd import TorchFit

    g, ge = golden(name), golden(f'ext_{name}')
    kind, md = util.load_md(model_root, name, g)
    om, _ = util.make_oracle(md, kind, np.float64)
    tf = TorchFit(BodyModel(kind, 'neutral', model_root=f'{model_root}/{util.model_dir(name)}', num_betas=10))
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    done = 0
    for case, cfg in util.KNOWN_SHAPE_CASES.items():
        if cfg[3] or cfg[5] or f'knownshape.{case}.trans' not in ge:
            continue
        betas, tv, kw = util.known_shape_inputs(g, case)
        with torch.no_grad():
            o = tf.fit_with_known_shape(T(betas), T(tv), T(kw['target_joints']), T(kw['vertex_weights']), T(kw['joint_weights']),
                                        T(kw['kid_factor']), num_iter=kw['num_iter'], final_adjust_rots=kw['final_adjust_rots'])
        assert o['trans'].dtype == torch.float32
        util.check_known_shape(om, name, case, {k: v.numpy() for k, v in o.items()}, ge, betas, kw)
        done += 1
    assert done >= 2


@pytest.mark.parametrize('tag,case', [(t, c) for t, cs in ku.FIXTURE_CASES.items() for c in cs])
def test_arbiter_matches_reference(gold, tag, case, model_root, golden):
    """The fp64 arbiter reproduces the reference's fp32 autograd gradients of ``fit_with_known_shape``.  Gate per tensor
    kind, relative to max |fp64|: twice the largest value the fixture's generator printed over its nine cases —
    shape_betas 3.8e-5, kid_factor 2.7e-6, target_vertices 4.5e-5, target_joints 3.6e-5, vertex_weights 1.3e-3 (SMPL
    alone: 3.3e-5, 2.7e-6, 4.1e-5, 2.5e-5, 1.0e-3) and joint_weights 1.5e2 (see REF_REL: a gradient of order 1e-7 that
    the reference's fp32 does not resolve; SMPL cases with more than one iteration: 1.1e-2 .. 1.7e-2)."""
    g = golden(tag)
    x, kw = ku.case_inputs(g, case, 2)
    p = f'{tag}.{case}.'
    cot = ku.cotangents(int(gold[p + 'seed']), 2, g['target_joints'].shape[1])
    out, grads = ku.arbiter(ku.torchfit64(model_root, tag, g, False), x, kw, cot)
    assert set(grads) == {k[len(p) + 4:] for k in gold.files if k.startswith(p + 'g32.')}
    for k in cot:
        tol = 2e-3 if k == 'pose_rotvecs' else 2e-4  # (the reference's fp32 fit against fp64; pose: tests/util.py pose_tol)
        assert np.abs(out[k] - gold[p + 'out.' + k]).max() <= tol, (tag, case, k)
    err = reference_errors(gold, tag, case, grads, g['target_vertices'].shape[1])
    for k, v in grads.items():
        print(f'[known-shape-grad] arbiter {tag} {case} {k} ref-vs-fp64 {err[k]:.2e} max {np.abs(v).max():.2e} rel {err[k] / np.abs(v).max():.2e}')
        assert err[k] <= REF_REL[k] * np.abs(v).max(), (tag, case, k, err[k])


# ---- the SF_HD functions ---------------------------------------------------------------------------------------------
def _lib():
    deps = [SRC, osp.join(HERE, 'hostemu', 'hostemu_fit_adjoint.cpp')] + [
        osp.join(CSRC, f) for f in ('sf_math.h', 'sf_stages.h', 'sf_tables.h', 'sf_tables.cpp')]
    if not osp.exists(SO) or any(osp.getmtime(d) > osp.getmtime(SO) for d in deps):
        os.makedirs(osp.dirname(SO), exist_ok=True)
        tmp = SO + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', SRC,
                        osp.join(CSRC, 'sf_tables.cpp'), '-o', tmp], check=True)
        os.replace(tmp, SO)
    return C.CDLL(SO)


def _close(tag, ours, ref, rel=GRAD_REL):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref
    e, m = np.abs(ours - ref).max(), np.abs(ref).max()
    print(f'[known-shape-grad] host {tag} ours-vs-fp64 {e:.2e} max {m:.2e} rel {e / max(m, 1e-300):.2e}')
    assert np.all(np.isfinite(ours)) and e <= rel * m, (tag, e, m)


@pytest.mark.parametrize('weighted', [True, False])
def test_host_alignment_adjoint(weighted):
    """sf::align_point_d / align_translation / align_point_adjoint against fp64 autograd through ``TorchFit._alignment``
    on 1000 points a few centimetres from their references, with weights in [0.5, 1.5) and without.  Gate GRAD_REL of
    max |fp64| per tensor.  Reaches 6e-8 on the points and 2e-6 on the weights."""
    from smplfitter_amd.pt._autograd import TorchFit

    rs = np.random.RandomState(4)
    n = 1000
    r = rs.randn(n, 3).astype(np.float32)
    tau = (r + 0.3 + 0.02 * rs.randn(n, 3)).astype(np.float32)
    w = rs.uniform(0.5, 1.5, n).astype(np.float32) if weighted else None
    tbar = rs.randn(3).astype(np.float32)
    d = lambda a: torch.tensor(a.astype(np.float64)[None], requires_grad=True)  # noqa: E731
    tt, rt, wt = d(tau), d(r), d(w) if weighted else None
    t = TorchFit._alignment(tt, None, rt, None, wt, None)
    (t * torch.tensor(tbar.astype(np.float64))).sum().backward()
    ours_t, g_tau, g_w = np.zeros(3, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    _lib().hostemu_ks_align(_p(tau), _p(r), _p(w), n, _p(tbar), _p(ours_t), _p(g_tau), _p(g_w))
    _close('alignment t', ours_t, t[0], 1e-6)
    _close('alignment targets', g_tau, tt.grad[0])
    _close('alignment references', -g_tau, rt.grad[0])
    if weighted:
        _close('alignment weights', g_w, wt.grad[0])


@pytest.mark.parametrize('form', ['joints', 'regressed', 'vertex_weights_only'])
def test_host_iteration_adjoint(form, model_root, golden):
    """The composition of one iteration of the reverse sweep — sf::fit_tail_adjoint, the alignment adjoint,
    sf::fit_rot_adjoint and the part-sum adjoints, in the order of smplfit_fit_known_shape_backward_f32 — against fp64
    autograd through ``TorchFit._rotations``, ``_alignment``, ``_refine`` and the output stage, with the meshes of the two
    stages as independent inputs: with target joints and both weights, without target joints (regressed joints, vertex
    weights count), and with target joints and vertex weights alone (the alignment is unweighted).  Gate GRAD_REL of
    max |fp64| per tensor.  Reaches: see DESIGN.md section 18."""
    from smplfitter_amd.pt._autograd import mat2rotvec

    s = _Stage(model_root, golden, joints=form != 'regressed')
    tf, c, B, V, J = s.tf, s.c, s.B, s.V, s.J
    c = dict(c, sd_all=c['known'][False][0], J_ext=c['known'][False][1])
    with torch.no_grad():
        rvn0, rjn0 = tf._forward(c, s.G0, s.beta)
    leaf = lambda a: a.clone().requires_grad_()  # noqa: E731
    tv, vw, rv0, rj0, Gprev, rvn, rjn, x = (leaf(a) for a in (s.tv, s.vw, s.rv, s.rj, s.G0, rvn0, rjn0, s.beta))
    tj = leaf(s.tj) if s.tj is not None else None
    jw = leaf(s.jw) if form == 'joints' else None
    G = tf._rotations(c, tv, tj, rv0, rj0 if tj is not None else None, vw, jw) @ Gprev
    t = tf._alignment(tv, tj, rvn, rjn, vw, jw)
    Gf = tf._refine(c, tv, tj, rvn + t[:, None], rjn + t[:, None], vw, jw, G, x, t)
    eye = torch.eye(3, dtype=torch.float64).expand(B, 1, 3, 3)
    rel = torch.cat([eye, Gf[:, tf.par[1:]]], 1).transpose(-1, -2) @ Gf
    rs = np.random.RandomState(5)
    cp, ct = rs.randn(B, J, 3), rs.randn(B, 3)
    ((mat2rotvec(rel) * torch.tensor(cp)).sum() + (t * torch.tensor(ct)).sum()).backward()
    z = lambda *sh: np.zeros(sh, np.float32)  # noqa: E731
    a = [_f32(v) for v in (s.tv, s.tj, s.vw, s.jw if form == 'joints' else None, s.rv, s.rj, s.G0, rvn0, rjn0, s.beta)]
    o = dict(Gout=z(B, J, 3, 3), trans=z(B, 3), g_tv=z(B, V, 3), g_tj=z(B, J, 3), g_vw=z(B, V), g_jw=z(B, J), g_rv0=z(B, V, 3),
             g_rj0=z(B, J, 3), g_Gprev=z(B, J, 3, 3), g_rvn=z(B, V, 3), g_rjn=z(B, J, 3), g_x=z(B, x.shape[1]))
    rc = _lib().hostemu_ks_iteration(C.byref(s.desc), B, *(_p(v) for v in a), 1, _p(_f32(cp)), _p(_f32(ct)),
                                     *(_p(o[k]) for k in o))
    assert rc == 0
    _close(f'iteration {form} G', o['Gout'], G, 1e-3)  # (the fp32 forward against fp64: tests/util.py pose_tol)
    _close(f'iteration {form} t', o['trans'], t, 1e-5)
    pairs = [('target_vertices', 'g_tv', tv), ('vertex_weights', 'g_vw', vw), ('mesh of the rotation pass', 'g_rv0', rv0),
             ('previous rotations', 'g_Gprev', Gprev), ('aligned mesh', 'g_rvn', rvn), ('joints of the aligned mesh', 'g_rjn', rjn),
             ('shape', 'g_x', x)]
    if tj is not None:
        pairs += [('target_joints', 'g_tj', tj), ('joints of the rotation pass', 'g_rj0', rj0)]
    if jw is not None:
        pairs.append(('joint_weights', 'g_jw', jw))
    for name, key, ref in pairs:
        _close(f'iteration {form} {name}', o[key], ref.grad)


def test_abi_symbols():
    from smplfitter_amd import _lib as L

    assert L.SMPLFIT_ABI_VERSION == 7
    for s in ('smplfit_fit_known_shape_backward_workspace_bytes', 'smplfit_fit_known_shape_backward_f32'):
        assert s in L.EXPORTED_SYMBOLS
    hdr = open(osp.join(HERE, '..', 'include', 'smplfit.h')).read()
    for s in ('smplfit_fit_known_shape_backward_args', 'smplfit_fit_known_shape_backward_workspace_bytes(',
              'smplfit_fit_known_shape_backward_f32('):
        assert s in hdr
    # every field of the struct is bound, in the header's order, and the mirror has the header's size
    name = 'smplfit_fit_known_shape_backward_args'
    body = hdr[hdr.index(f'typedef struct {name} {{'):hdr.index(f'}} {name};')]
    names = []
    for line in body.splitlines()[1:]:
        decl = line.split('/*')[0].strip().rstrip(';')
        if decl:
            names += [n.strip().lstrip('*').strip() for n in decl.split(' ', 1 if not decl.startswith('const') else 2)[-1].split(',')]
    assert names == [f[0] for f in L.FitKnownShapeBackwardArgs._fields_], names
    src = osp.join(HERE, 'hostemu', '_build', f'sizeof_{name}.c')
    os.makedirs(osp.dirname(src), exist_ok=True)
    with open(src, 'w') as fh:
        fh.write(f'#include <stdio.h>\n#include "smplfit.h"\nint main(void) {{ printf("%zu", sizeof({name})); return 0; }}\n')
    exe = src[:-2]
    subprocess.run(['gcc', '-I', osp.join(HERE, '..', 'include'), src, '-o', exe], check=True)
    assert int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout) == C.sizeof(L.FitKnownShapeBackwardArgs)
