"""Cases, seeded cotangents and the fp64 arbiter of the ``BodyConverter`` gradient tests (tests/test_convert_grad_host.py,
tests/test_gpu_convert_grad.py, tests/golden/make_golden_convert_grad.py).

The arbiter is a composition of the arbiters the other gradient tests already use, run in fp64 on the CPU: the input
model's forward (``grad_util.Model64`` / ``grad_util.forward``), the synthetic transfer matrix (``util.load_transfer_csr``)
as an fp64 sparse product, then the fit of the branch — ``TorchFit(enable_kid=True, dtype=float64).fit`` (beta ridge 0,
no final adjustment, kid ridge 1e9, or 0 when ``kid_factor`` is given), ``TorchFit.fit_with_known_shape``, or
``known_pose_grad_util.solve64``.  ``torch.autograd.grad`` gives the gradients.

The reference's own fp32 gradients (golden_convert_grad.npz) against this arbiter, relative to max |fp64| per tensor, as
tests/golden/make_golden_convert_grad.py prints them (largest over the two directions):

    case      pose_rotvecs  shape_betas  trans     known-output input
    it1       3.1e-4        4.9e-5       2.0e-5
    it2       1.3e-4        4.1e-5       2.4e-5
    kid.it1   2.7e-4        4.2e-5       4.7e-5
    kshape    3.0e-4        4.4e-5       2.3e-5    5.8e-5
    kpose     8.1e-6        1.3e-6       1.8e-6    5.1e-6

All are far below REF_REL_CAP, the condition under which the second term of the gradient gate (twice the reference's own
error) cannot make the gate vacuous.
"""

import numpy as np
import torch

import fit_grad_util
import grad_util
import known_pose_grad_util
import util

B = 2  # instances of the fixture
DIRS = util.CONVERT_DIRS  # tag -> (input golden-set name, output golden-set name)
# the cases of golden_convert_grad.npz: the branch of ``convert``, its options, the tensor inputs that require grad
CASES = {
    'it1': dict(branch='default', num_iter=1),
    'it2': dict(branch='default', num_iter=2),
    'kid.it1': dict(branch='default', num_iter=1, kid=True),
    'kshape': dict(branch='kshape', num_iter=2),
    'kpose': dict(branch='kpose'),
}
INPUTS = ('pose_rotvecs', 'shape_betas', 'trans')
KNOWN = dict(kshape='known_output_shape_betas', kpose='known_output_pose_rotvecs')
REF_REL_CAP = 1e-2  # the generator's condition on every reference-versus-arbiter figure
# the largest reference-versus-arbiter figure the generator printed, per tensor (the docstring's table)
REF_REL_LARGEST = dict(pose_rotvecs=3.1e-4, shape_betas=4.9e-5, trans=4.7e-5, known_output_shape_betas=5.8e-5,
                       known_output_pose_rotvecs=5.1e-6)
# largest |reference fp32 result - arbiter fp64 result| the generator printed, per result
REF_OUT_LARGEST = dict(pose_rotvecs=1.3e-4, shape_betas=1.2e-5, trans=1.7e-6, kid_factor=4.2e-6)


def grad_names(case):
    """The tensor inputs of a case that require grad, in the order the fixture stores their gradients."""
    branch = CASES[case]['branch']
    return INPUTS + ((KNOWN[branch],) if branch in KNOWN else ())


def output_names(case):
    """The results of a case = the tensors the cotangents are on."""
    cfg = CASES[case]
    names = dict(default=('pose_rotvecs', 'shape_betas', 'trans'), kshape=('pose_rotvecs', 'trans'),
                 kpose=('shape_betas', 'trans'))[cfg['branch']]
    return names + (('kid_factor',) if cfg.get('kid') else ())


def make_inputs(tag, j_in, j_out, nb=10):
    """Seeded inputs of one direction (numpy fp32), shared by its cases: the input model's parameters, a kid factor and
    the two known-output tensors."""
    rs = np.random.RandomState(dict(s2x=177, x2s=178)[tag])
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return dict(pose_rotvecs=f(rs.randn(B, 3 * j_in) * 0.1), shape_betas=f(rs.randn(B, nb) * 0.5), trans=f(rs.randn(B, 3)),
                kid_factor=f(rs.randn(B) * 0.3), known_output_shape_betas=f(rs.randn(B, nb) * 0.3),
                known_output_pose_rotvecs=f(rs.randn(B, 3 * j_out) * 0.05))


def fixture_inputs(gcg, tag):
    """The inputs of direction ``tag`` as golden_convert_grad.npz stores them."""
    pre = f'{tag}.in.'
    return {k[len(pre):]: v for k, v in gcg.items() if k.startswith(pre)}


def convert_kwargs(case, x):
    """Keyword arguments of ``BodyConverter.convert`` for a case, from the inputs ``x`` (arrays or tensors)."""
    cfg = CASES[case]
    kw = {k: x[k] for k in INPUTS}
    if cfg.get('kid'):
        kw['kid_factor'] = x['kid_factor']
    if cfg['branch'] in KNOWN:
        kw[KNOWN[cfg['branch']]] = x[KNOWN[cfg['branch']]]
    if 'num_iter' in cfg:
        kw['num_iter'] = cfg['num_iter']
    return kw


def cotangents(seed, case, n_joints_out, nb=10, batch=B):
    """Seeded cotangents of the results of a case (not stored in the fixture)."""
    rs = np.random.RandomState(seed)
    shapes = dict(pose_rotvecs=(batch, 3 * n_joints_out), shape_betas=(batch, nb), trans=(batch, 3), kid_factor=(batch,))
    return {k: rs.randn(*shapes[k]).astype(np.float32) for k in output_names(case)}


def case_seed(tag, case):
    return 1000 * (1 + list(DIRS).index(tag)) + list(CASES).index(case) + 1


_cache = {}


def _models(model_root, data_root, tag):
    if tag not in _cache:
        a, b = DIRS[tag]
        m_in = grad_util.Model64(util.load_md(model_root, a)[1])
        m_out = grad_util.Model64(util.load_md(model_root, b)[1])
        csr = util.load_transfer_csr(data_root, tag).tocoo()
        mat = torch.sparse_coo_tensor(np.stack([csr.row, csr.col]), csr.data.astype(np.float64), csr.shape).coalesce()
        _cache[tag] = m_in, m_out, fit_grad_util.torchfit64(model_root, b, {}, True), mat
    return _cache[tag]


def transfer64(mat, vertices):
    """(B, V_in, 3) -> (B, V_out, 3) with the sparse fp64 matrix, differentiable in the vertices."""
    n = vertices.shape[0]
    flat = vertices.permute(1, 0, 2).reshape(mat.shape[1], n * 3)
    return torch.sparse.mm(mat, flat).reshape(mat.shape[0], n, 3).permute(1, 0, 2)


def convert64(model_root, data_root, tag, case, ts):
    """``convert`` of a case on fp64 torch tensors ``ts`` (differentiable): the results the reference returns."""
    cfg = CASES[case]
    m_in, m_out, tf, mat = _models(model_root, data_root, tag)
    # as in the reference (pt/bodyconverter.py:86), the input mesh is evaluated without kid_factor
    mesh = grad_util.forward(m_in, pose_rotvecs=ts['pose_rotvecs'], shape_betas=ts['shape_betas'], trans=ts['trans'])
    target = transfer64(mat, mesh['vertices'])
    kid_reg = 0.0 if cfg.get('kid') else 1e9
    if cfg['branch'] == 'default':
        r = tf.fit(target, num_iter=cfg['num_iter'], beta_regularizer=0.0, kid_regularizer=kid_reg, final_adjust_rots=False)
    elif cfg['branch'] == 'kshape':
        r = tf.fit_with_known_shape(ts['known_output_shape_betas'], target, num_iter=cfg['num_iter'],
                                    final_adjust_rots=False)
    else:
        r = known_pose_grad_util.solve64(m_out, dict(pose_rotvecs=ts['known_output_pose_rotvecs'], target_vertices=target),
                                         dict(beta_regularizer=0.0, kid_regularizer=kid_reg), kid=True)
    return {k: r[k] for k in output_names(case)}


def arbiter(model_root, data_root, tag, case, x, cot):
    """fp64 results and gradients of sum(cot . results) w.r.t. ``grad_names(case)`` (numpy in, numpy out)."""
    torch.set_num_threads(8)
    ts = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=k in grad_names(case)) for k, v in x.items()}
    out = convert64(model_root, data_root, tag, case, ts)
    loss = sum((out[k] * torch.as_tensor(np.asarray(c, np.float64))).sum() for k, c in cot.items())
    names = grad_names(case)
    gs = torch.autograd.grad(loss, [ts[k] for k in names], allow_unused=True)
    grads = {k: (np.zeros(ts[k].shape) if g is None else g.numpy()) for k, g in zip(names, gs)}
    return {k: v.detach().numpy() for k, v in out.items()}, grads


def gate(ours, g64, g32):
    """The gradient gate of DESIGN.md §17 / §18 for one tensor: (error, bound) with
    bound = max(2e-4 max |fp64|, 2 max |reference fp32 - fp64|)."""
    g64 = np.asarray(g64, np.float64)
    err = float(np.abs(np.asarray(ours, np.float64) - g64).max())
    return err, max(2e-4 * float(np.abs(g64).max()), 2 * float(np.abs(np.asarray(g32, np.float64) - g64).max()))
