"""Shared pieces of the ``BodyModel.rototranslate`` tests (tests/test_rototranslate_host.py,
tests/test_gpu_rototranslate.py) and of the fixture generator (tests/golden/make_golden_rototranslate.py):

* the fixture's models and cases, and access to ``tests/golden/golden_rototranslate.npz``;
* the fp64 restatement of the reference's lines (pt/bodymodel.py:435-453): ``forward64`` in numpy (the root as a
  rotation MATRIX — near an angle of pi the rotation vector's sign is ambiguous, the matrix is not) and ``grads64``
  through fp64 torch autograd;
* the loader of the host emulation (tests/hostemu/hostemu_rototranslate.cpp: the per-instance bodies of
  csrc/sf_rigid.h, the functions the kernels call, built with g++).
"""

import ctypes as C
import os
import os.path as osp
import subprocess

import numpy as np
import torch

import grad_util

HERE = osp.dirname(osp.abspath(__file__))
GOLDEN = osp.join(HERE, 'golden', 'golden_rototranslate.npz')
SRC = osp.join(HERE, 'hostemu', 'hostemu_rototranslate.cpp')
SO = osp.join(HERE, 'hostemu', '_build', 'libhostemu_rototranslate.so')
CSRC = osp.join(HERE, '..', 'smplfitter_amd', 'csrc')

# tag -> (model kind, directory under the synthetic model root, num_betas of the model)
MODELS = {'smpl': ('smpl', 'smpl', 10), 'smplx': ('smplx', 'smplx', 10), 'smpl_b300': ('smpl', 'smpl_b300', None)}
SYNTH_KINDS = ('smpl', 'smplx', 'smpl_b300')
ROWS, GRAD_ROWS = 16, 8
# case -> (post_translate, kid_factor given, betas given (None: the model's), t given)
CASES = {
    'post_nokid': (True, False, None, True), 'pre_nokid': (False, False, None, True),
    'post_kid': (True, True, None, True), 'pre_kid': (False, True, None, True),
}
SMPL_ONLY_CASES = {'post_nb4_not': (True, False, 4, False)}  # 4 betas to a 10-beta model, and no t
GRAD_CASES = {'post_kid': (True, True, None, True), 'pre_nokid': (False, False, None, True)}
INPUTS = ('R', 't', 'pose_rotvecs', 'shape_betas', 'trans', 'kid_factor')
FLOOR_MARGIN = 5.0  # = hand_util.FLOOR_MARGIN: the reference's own rounding may be at most a fifth of a gate


def cases_of(tag):
    return {**CASES, **(SMPL_ONLY_CASES if tag == 'smpl' else {})}


def load_md(tag, root=None):
    from smplfitter_amd import modelio, synth

    root = synth.ensure_model_root(kinds=SYNTH_KINDS, seed=0) if root is None else root
    kind, d, nb = MODELS[tag]
    return modelio.load_model(kind, 'neutral', model_root=f'{root}/{d}', num_betas=nb)


def select_inputs(rows, flags):
    """The inputs a case gives, of a model's rows (name -> rows-first array): (inputs, post_translate)."""
    post, kid, nb, has_t = flags
    x = dict(rows)
    if not kid:
        x.pop('kid_factor')
    if not has_t:
        x.pop('t')
    if nb is not None:
        x['shape_betas'] = np.ascontiguousarray(x['shape_betas'][:, :nb])
    return x, post


def case_inputs(gold, tag, case, grad=False):
    """(inputs, post_translate) of a fixture case; the rows of a model (``<tag>.in.*``, ``<tag>.grad.in.*``) are
    stored once and shared by its cases."""
    p = f'{tag}.{"grad." if grad else ""}in.'
    rows = {k[len(p):]: gold[k] for k in gold.files if k.startswith(p)}
    return select_inputs(rows, (GRAD_CASES if grad else cases_of(tag))[case])


# ---- fp64 restatement --------------------------------------------------------------------------
def rotvec2mat64(rv):
    """Rodrigues in numpy float64, (..., 3) -> (..., 3, 3); exact at 0."""
    return grad_util.rotvec2mat(torch.as_tensor(np.asarray(rv, np.float64))).numpy()


def _const64(md, name):
    """Joint 0's rows of a model constant as the kernels and the reference hold it: rounded to fp32, then as fp64."""
    return np.asarray(getattr(md, name), np.float32)[0].astype(np.float64)


def pelvis64(md, betas, kid):
    betas = np.asarray(betas, np.float64)
    n = betas.shape[-1]
    p = _const64(md, 'J_template') + betas @ _const64(md, 'J_shapedirs')[:, :n].T
    if kid is not None:
        p = p + np.asarray(kid, np.float64).reshape(-1, 1) * _const64(md, 'kid_J_shapedir')
    return p


def forward64(md, R, t, pose_rotvecs, shape_betas, trans, kid_factor, post_translate):
    """(root rotation matrix (B, 3, 3), new_trans (B, 3)) in float64 of rows-first inputs (R (B, 3, 3) or (3, 3), t
    (B, 3), (3,) or None, shape_betas (B, n) or (n,), kid_factor (B), a scalar or None)."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    pose, trans, R = f(pose_rotvecs), f(trans), f(R)
    B = pose.shape[0]
    R = np.broadcast_to(R, (B, 3, 3))
    t = np.zeros((B, 3)) if t is None else np.broadcast_to(f(t), (B, 3))
    betas = np.broadcast_to(f(shape_betas), (B, np.shape(shape_betas)[-1]))
    kid = None if kid_factor is None else np.broadcast_to(f(kid_factor).reshape(-1), (B,))
    root = R @ rotvec2mat64(pose[:, :3])
    p = pelvis64(md, betas, kid)
    rp = np.einsum('bij,bj->bi', R, p) - p
    if post_translate:
        return root, np.einsum('bij,bj->bi', R, trans) + t + rp
    return root, np.einsum('bij,bj->bi', R, trans - t) + rp


def _mat2rotvec_t(M):
    """Log map in torch (differentiable) as the function of the NINE matrix entries that sf::mat2rotvec (csrc/sf_math.h)
    and the reference evaluate — the four-way quaternion form, 2 atan2(|xyz|, w) / |xyz| xyz: the gradient with respect
    to an unconstrained R depends on how the map is continued off the rotations, so another formula of the same
    rotation vector will not do."""
    r = [[M[..., i, j] for j in range(3)] for i in range(3)]
    tr = r[0][0] + r[1][1] + r[2][2]
    q0 = (r[2][1] - r[1][2], r[0][2] - r[2][0], r[1][0] - r[0][1], 1 + tr)
    q1 = ((1 - r[2][2]) + (r[0][0] - r[1][1]), r[1][0] + r[0][1], r[0][2] + r[2][0], r[2][1] - r[1][2])
    q2 = (r[1][0] + r[0][1], (1 - r[2][2]) - (r[0][0] - r[1][1]), r[2][1] + r[1][2], r[0][2] - r[2][0])
    q3 = (r[0][2] + r[2][0], r[2][1] + r[1][2], (1 + r[2][2]) - (r[0][0] + r[1][1]), r[1][0] - r[0][1])
    b0, b1, b2 = tr > 0, (r[0][0] > r[1][1]) & (r[0][0] > r[2][2]), r[1][1] > r[2][2]
    q = [torch.where(b0, a, torch.where(b1, b, torch.where(b2, c, d))) for a, b, c, d in zip(q0, q1, q2, q3)]
    xyz = torch.stack(q[:3], -1)
    n = torch.sqrt((xyz * xyz).sum(-1))
    return xyz * (2 * torch.atan2(n, q[3]) / n)[..., None]


def grads64(md, x, cot_pose, cot_trans, post_translate):
    """fp64 autograd gradients of <cot_pose, new_pose> + <cot_trans, new_trans> w.r.t. every input of ``x`` (name ->
    rows-first array; R, t, shape_betas and kid_factor always per row here), as numpy: name -> (B, ...)."""
    ts = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in x.items()}
    pose, R = ts['pose_rotvecs'], ts['R']
    B = pose.shape[0]
    t = ts['t'] if 't' in ts else torch.zeros((B, 3), dtype=torch.float64)
    root = _mat2rotvec_t(grad_util.mm(R, grad_util.rotvec2mat(pose[:, :3])))
    new_pose = torch.cat([root, pose[:, 3:]], 1)
    n = ts['shape_betas'].shape[1]
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    p = t64(_const64(md, 'J_template')) + ts['shape_betas'] @ t64(_const64(md, 'J_shapedirs'))[:, :n].T
    if 'kid_factor' in ts:
        p = p + ts['kid_factor'].reshape(B, 1) * t64(_const64(md, 'kid_J_shapedir'))
    xx = ts['trans'] if post_translate else ts['trans'] - t
    new_trans = grad_util.mv(R, xx) + grad_util.mv(R, p) - p + (t if post_translate else 0)
    loss = (new_pose * t64(cot_pose)).sum() + (new_trans * t64(cot_trans)).sum()
    names = list(ts)
    gs = torch.autograd.grad(loss, [ts[k] for k in names], allow_unused=True)
    return {k: (np.zeros(ts[k].shape) if g is None else g.numpy()) for k, g in zip(names, gs)}


def root_error(new_pose, root64):
    """max |rotvec2mat(new_pose[:, :3]) - root64|: the root compared as a rotation matrix."""
    return float(np.abs(rotvec2mat64(np.asarray(new_pose)[:, :3]) - root64).max())


def trans_error(new_trans, trans64):
    """max over rows of |new_trans - trans64|_inf / max(1, |trans64|_inf)."""
    d = np.abs(np.asarray(new_trans, np.float64) - trans64).max(-1)
    return float((d / np.maximum(1.0, np.abs(trans64).max(-1))).max())


def grad_error(g, g64):
    """max |g - g64| / max |g64| (0 where both vanish)."""
    d, m = float(np.abs(np.asarray(g, np.float64) - g64).max()), float(np.abs(g64).max())
    return d / m if m > 0 else d


# ---- host emulation ----------------------------------------------------------------------------
def hostemu_lib():
    deps = [SRC] + [osp.join(CSRC, f) for f in ('sf_math.h', 'sf_stages.h', 'sf_rigid.h')]
    if not osp.exists(SO) or any(osp.getmtime(d) > osp.getmtime(SO) for d in deps):
        os.makedirs(osp.dirname(SO), exist_ok=True)
        tmp = SO + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', SRC, '-o', tmp], check=True)
        os.replace(tmp, SO)
    return C.CDLL(SO)


def _j_ext(md, kid):
    """Joint 0's rows of JointTabs::j_ext: (3, S + 1), [J_template | J_shapedirs (| kid_J_shapedir)]."""
    cols = [np.asarray(md.J_template, np.float32)[0][:, None], np.asarray(md.J_shapedirs, np.float32)[0]]
    if kid:
        cols.append(np.asarray(md.kid_J_shapedir, np.float32)[0][:, None])
    j = np.ascontiguousarray(np.concatenate(cols, 1), np.float32)
    return j, j.shape[1] - 1


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _rows_first(x):
    """(R, R_stride, t, t_stride, pose, betas, nb, kid, trans) as contiguous float32 for the emulation's pointers."""
    R, t = _f32(x['R']), _f32(x.get('t'))
    pose, betas, trans, kid = _f32(x['pose_rotvecs']), _f32(x['shape_betas']), _f32(x['trans']), _f32(x.get('kid_factor'))
    return R, (9 if R.ndim == 3 else 0), t, (3 if t is not None and t.ndim == 2 else 0), pose, betas, betas.shape[1], kid, trans


def hostemu_forward(md, x, post_translate):
    """(new_pose (B, 3J), new_trans (B, 3)) of the emulation; ``x``: name -> rows-first arrays (R / t may be shared)."""
    lib = hostemu_lib()
    R, rs, t, tstr, pose, betas, nb, kid, trans = _rows_first(x)
    j_ext, S = _j_ext(md, kid is not None)
    B, J3 = pose.shape
    new_pose, new_trans = np.empty_like(pose), np.empty_like(trans)
    lib.hostemu_rototranslate(_p(j_ext), S, J3, B, _p(R), rs, _p(t), tstr, _p(pose), _p(betas) if nb else None, nb,
                              _p(kid), _p(trans), int(post_translate), _p(new_pose), _p(new_trans))
    return new_pose, new_trans


def hostemu_backward(md, x, cot_pose, cot_trans, post_translate):
    """Per-row gradients of the emulation: name -> (B, ...) for R, t, pose_rotvecs, shape_betas, trans, kid_factor."""
    lib = hostemu_lib()
    R, rs, t, tstr, pose, betas, nb, kid, trans = _rows_first(x)
    j_ext, S = _j_ext(md, kid is not None)
    B, J3 = pose.shape
    gp, gt_in = _f32(cot_pose), _f32(cot_trans)
    out = dict(R=np.empty((B, 3, 3), np.float32), t=np.empty((B, 3), np.float32), pose_rotvecs=np.empty_like(pose),
               shape_betas=np.empty((B, nb), np.float32), trans=np.empty((B, 3), np.float32),
               kid_factor=np.empty((B,), np.float32))
    lib.hostemu_rototranslate_backward(
        _p(j_ext), S, J3, B, _p(R), rs, _p(t), tstr, _p(pose), _p(betas) if nb else None, nb, _p(kid), _p(trans),
        int(post_translate), _p(gp), _p(gt_in), _p(out['R']), _p(out['t']), _p(out['pose_rotvecs']),
        _p(out['shape_betas']) if nb else None, _p(out['trans']), _p(out['kid_factor']) if kid is not None else None)
    if kid is None:
        del out['kid_factor']
    return out
