"""Host checks of BodyModel.forward's backward (no GPU): the fp64 torch restatement (tests/grad_util.py) against the
reference's own fp64 gradients (tests/golden/golden_forward_grad.npz), the per-instance joint backward of
csrc/sf_stages.h built with g++ (tests/hostemu/hostemu_grad.cpp) against that restatement, the angle-0 derivative of
the exponential map against a central fp64 finite difference, and the new C-ABI symbols."""

import ctypes as C
import os
import os.path as osp
import subprocess

import numpy as np
import pytest
import torch

import grad_util
import util

HERE = osp.dirname(osp.abspath(__file__))
GOLDEN = osp.join(HERE, 'golden', 'golden_forward_grad.npz')
SRC = osp.join(HERE, 'hostemu', 'hostemu_grad.cpp')
SO = osp.join(HERE, 'hostemu', '_build', 'libhostemu_grad.so')
CSRC = osp.join(HERE, '..', 'smplfitter_amd', 'csrc')
MODELS = {'smpl': 10, 'smplxfat': 10, 'smpl_w6': 10, 'smpl_b300': None}
_m64 = {}


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLDEN)


def _model(tag):
    if tag not in _m64:
        from smplfitter_amd import modelio, synth

        root = synth.ensure_model_root(kinds=('smpl', 'smplx_fat', 'smpl_w6', 'smpl_b300'), seed=0)
        from grad_util import model_dir

        kind = 'smplx' if tag.startswith('smplx') else 'smpl'
        md = modelio.load_model(kind, 'neutral', model_root=f'{root}/{model_dir(tag)}', num_betas=MODELS[tag])
        _m64[tag] = (md, grad_util.Model64(md))
    return _m64[tag]


def _case(gold, tag, case):
    p = f'{tag}.{case}.'
    x = {k[len(p) + 3:]: gold[k] for k in gold.files if k.startswith(p + 'in.')}
    return x, int(gold[p + 'seed']), bool(gold[p + 'return_vertices']), str(gold[p + 'which']).split(',')


@pytest.mark.parametrize('tag', list(MODELS))
def test_restatement_matches_reference_fp64(gold, tag):
    from grad_util import CASES, cotangents

    md, m64 = _model(tag)
    for case in CASES:
        x, seed, rv, which = _case(gold, tag, case)
        cot = cotangents(seed, len(next(iter(x.values()))) if 'trans' not in x or x['trans'].shape[0] > 1 else 8,
                         m64.J, md.v_template.shape[0], which)
        g = grad_util.grads(m64, x, cot, return_vertices=rv)
        for k, v in g.items():
            ref = gold[f'{tag}.{case}.g64.{k}']
            # (the model loaders differ: the reference derives some constants in fp32 — its fp64 forward agrees with
            # util.forward64 to 1e-7 m — so the gradients agree to that level, not to 1e-10)
            assert np.abs(v - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), (tag, case, k)
            # the same restatement on the reference model's own buffers, recorded by the generator: 1e-10
            assert float(gold[f'{tag}.{case}.restate.{k}']) <= 1e-10, (tag, case, k)


def _lib():
    deps = [SRC, osp.join(CSRC, 'sf_math.h'), osp.join(CSRC, 'sf_stages.h')]
    if not osp.exists(SO) or any(osp.getmtime(d) > osp.getmtime(SO) for d in deps):
        os.makedirs(osp.dirname(SO), exist_ok=True)
        tmp = SO + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', SRC, '-o', tmp], check=True)
        os.replace(tmp, SO)
    return C.CDLL(SO)


def _fk_order(parents):
    J = len(parents)
    level = [0] * J
    for j in range(1, J):
        level[j] = level[parents[j]] + 1
    order = sorted(range(1, J), key=lambda j: (level[j], j))
    starts = [0]
    for lv in range(1, max(level) + 1):
        starts.append(starts[-1] + sum(1 for j in order if level[j] == lv))
    return np.array(order, np.int32), np.array(starts, np.int32), max(level)


@pytest.mark.parametrize('form', ['pose', 'rel', 'glob'])
@pytest.mark.parametrize('tag', ['smpl', 'smplxfat'])
def test_host_joint_backward(tag, form):
    """sf::forward_joint_backward (fp32, one lane) against autograd of the fp64 restatement's joint part, with random
    dA, dfeat, dshape seeds: their fp64 counterparts are the autograd of the sums <dA, (G | t)>, <dfeat, features>,
    <dshape, betas>."""
    md, m64 = _model(tag)
    J, S = m64.J, m64.S
    B, nb = 3, 10
    rs = np.random.RandomState(7)
    x = dict(shape_betas=rs.randn(B, nb).astype(np.float32))
    if form == 'pose':
        x['pose_rotvecs'] = (rs.randn(B, J * 3) * 0.5).astype(np.float32)
    else:
        x[f'{form}_rotmats'] = grad_util.random_rotmats(rs, (B, J)).astype(np.float32)
    dA = rs.randn(B, J, 12).astype(np.float32)
    gj = rs.randn(B, J, 3).astype(np.float32)
    go = rs.randn(B, J, 3, 3).astype(np.float32)
    df = rs.randn(B, 9 * (J - 1)).astype(np.float32)
    ds = rs.randn(B, S).astype(np.float32)
    # fp64: the forward's joint part, differentiated through torch
    ts = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in x.items()}
    par = m64.parents
    if form == 'pose':
        rel = grad_util.rotvec2mat(ts['pose_rotvecs'].reshape(B, J, 3))
    elif form == 'rel':
        rel = ts['rel_rotmats']
    glob = ts['glob_rotmats'] if form == 'glob' else None
    if glob is None:
        g = [rel[:, 0]]
        for j in range(1, J):
            g.append(g[par[j]] @ rel[:, j])
        glob = torch.stack(g, 1)
    p1 = torch.tensor(par[1:])
    feat = glob[:, p1].transpose(-1, -2) @ glob[:, 1:] if form == 'glob' else rel[:, 1:]
    betas = ts['shape_betas']
    jr = m64.J_template + torch.einsum('jcs,bs->bjc', m64.J_shapedirs[:, :, :nb], betas)
    rb = torch.einsum('bjcd,bjd->bjc', glob[:, p1], jr[:, 1:] - jr[:, p1])
    pos = [jr[:, 0]]
    for j in range(1, J):
        pos.append(pos[par[j]] + rb[:, j - 1])
    pos = torch.stack(pos, 1)
    t = pos - torch.einsum('bjcd,bjd->bjc', glob, jr)
    d = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    block = torch.cat([glob.reshape(B, J, 9), t], -1)
    loss = ((block * d(dA)).sum() + (pos * d(gj)).sum() + (glob * d(go)).sum()
            + (feat.reshape(B, -1) * d(df)).sum() + (betas * d(ds[:, :nb])).sum())
    ref = dict(zip(ts, [a.numpy() for a in torch.autograd.grad(loss, list(ts.values()))]))
    lib = _lib()
    fk, starts, nlev = _fk_order(par)
    S1 = S + 1
    j_ext = np.zeros((J, 3, S1), np.float32)
    j_ext[:, :, 0] = md.J_template
    j_ext[:, :, 1:] = md.J_shapedirs
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(C.c_void_p)  # noqa: E731
    out = {k: np.zeros(v.shape, np.float32) for k, v in x.items()}
    g_tr = np.zeros((B, 3), np.float32)
    par32 = np.asarray(par, np.int32)
    keep = [par32, fk, starts, j_ext, x, dA, gj, go, df, ds]  # noqa: F841 (alive during the call)
    lib.hostemu_joint_backward(
        J, S, 0, f(par32) and par32.ctypes.data_as(C.c_void_p), fk.ctypes.data_as(C.c_void_p),
        starts.ctypes.data_as(C.c_void_p), nlev, j_ext.ctypes.data_as(C.c_void_p), B,
        f(x.get('pose_rotvecs')), f(x.get('glob_rotmats')), f(x.get('rel_rotmats')), f(x['shape_betas']), nb, None,
        f(dA), f(gj), f(go), f(df), f(ds), *(out[k].ctypes.data_as(C.c_void_p) if k in out else None
                                            for k in ('pose_rotvecs', 'glob_rotmats', 'rel_rotmats', 'shape_betas')),
        None, g_tr.ctypes.data_as(C.c_void_p))
    for k in ref:
        err = np.abs(out[k] - ref[k]).max()
        assert err <= 1e-5 * np.abs(ref[k]).max(), (tag, form, k, err)
    assert np.allclose(g_tr, gj.sum(1), atol=1e-5)


def test_rodrigues_derivative_at_zero():
    """At r = 0 the derivative of exp([r]x) is [e_i]x (not 0 as the reference's autograd gives), and near zero the series
    matches a central fp64 finite difference of the closed form."""
    lib = _lib()
    rs = np.random.RandomState(3)
    rv = np.concatenate([np.zeros((1, 3)), rs.randn(5, 3) * 1e-4, rs.randn(5, 3) * 0.3, rs.randn(3, 3) * 0.49,
                         rs.randn(3, 3) * 2]).astype(np.float32)
    dR = rs.randn(len(rv), 3, 3).astype(np.float32)
    dr = np.zeros((len(rv), 3), np.float32)
    lib.hostemu_rotvec2mat_vjp(rv.ctypes.data_as(C.c_void_p), dR.ctypes.data_as(C.c_void_p),
                               dr.ctypes.data_as(C.c_void_p), len(rv))

    def rod(r):
        th = np.linalg.norm(r)
        K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        if th == 0:
            return np.eye(3) + K
        return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K

    for n in range(len(rv)):
        r = rv[n].astype(np.float64)
        fd = np.zeros(3)
        for i in range(3):
            h = 1e-6 * np.eye(3)[i]
            fd[i] = ((rod(r + h) - rod(r - h)) / 2e-6 * dR[n]).sum()
        assert np.abs(dr[n] - fd).max() <= 2e-5 * max(1.0, np.abs(fd).max()), (n, dr[n], fd)
    E = [np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]]), np.array([[0, 0, 1], [0, 0, 0], [-1, 0, 0]]),
         np.array([[0, -1, 0], [1, 0, 0], [0, 0, 0]])]
    assert np.allclose(dr[0], [(E[i] * dR[0]).sum() for i in range(3)], atol=1e-6)


def test_abi_symbols():
    from smplfitter_amd import _lib as L

    assert L.SMPLFIT_ABI_VERSION == 7
    for s in ('smplfit_forward_backward_workspace_bytes', 'smplfit_forward_backward_f32'):
        assert s in L.EXPORTED_SYMBOLS
    hdr = open(osp.join(HERE, '..', 'include', 'smplfit.h')).read()
    assert '#define SMPLFIT_ABI_VERSION 7' in hdr and 'smplfit_forward_backward_args' in hdr
