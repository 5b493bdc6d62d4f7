"""Host checks of BodyModel.rototranslate (no GPU): the per-instance bodies the kernels call (csrc/sf_rigid.h, built
with g++: tests/hostemu/hostemu_rototranslate.cpp) against the fp64 restatement under gates of 5 x the reference's own
fp32 floors recorded in tests/golden/golden_rototranslate.npz, their backward against fp64 autograd of the restatement,
the root gradient at a root of exactly 0 against a central fp64 finite difference, the new C-ABI symbols, and the
Python method's refusals."""

import os.path as osp
import sys

import numpy as np
import pytest
import torch

import rototranslate_util as U

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, osp.join(HERE, '..', 'oracle'))
import smplfit_oracle as O  # noqa: E402

_md = {}


@pytest.fixture(scope='module')
def gold():
    return np.load(U.GOLDEN)


def _model(tag):
    if tag not in _md:
        _md[tag] = U.load_md(tag)
    return _md[tag]


def test_fixture_shape(gold):
    """The fixture is the one tests/golden/make_golden_rototranslate.py describes: the two loaders agree to the bit on
    the pelvis constants, the row kinds are there, and the reference copies pose[3:] (the generator asserts it)."""
    for tag in U.MODELS:
        assert float(gold[f'{tag}.loader']) == 0.0
        x, _ = U.case_inputs(gold, tag, 'post_kid')
        assert x['pose_rotvecs'].shape[0] == U.ROWS
        assert np.array_equal(x['R'][1], np.eye(3, dtype=np.float32)) and not x['pose_rotvecs'][4, :3].any()
        ang = [np.linalg.norm(O.mat2rotvec(x['R'][i].astype(np.float64) @ O.rotvec2mat(x['pose_rotvecs'][i, :3].astype(np.float64))))
               for i in (2, 7, 12)]
        assert all(np.pi - 1.1e-3 < a <= np.pi for a in ang), ang
        assert np.abs(x['trans'][3]).max() > 10
    assert gold['smpl.in.shape_betas'].shape[1] == 10 and gold['smpl_b300.in.shape_betas'].shape[1] == 300


@pytest.mark.parametrize('tag', list(U.MODELS))
def test_hostemu_forward(gold, tag):
    md = _model(tag)
    for case in U.cases_of(tag):
        x, post = U.case_inputs(gold, tag, case)
        new_pose, new_trans = U.hostemu_forward(md, x, post)
        root64, trans64 = U.forward64(md, x['R'], x.get('t'), x['pose_rotvecs'], x['shape_betas'], x['trans'],
                                      x.get('kid_factor'), post)
        e_root, e_trans = U.root_error(new_pose, root64), U.trans_error(new_trans, trans64)
        f_root, f_trans = float(gold[f'{tag}.{case}.floor.root']), float(gold[f'{tag}.{case}.floor.trans'])
        print(f'{tag} {case}: root {e_root:.2e} (floor {f_root:.2e})  trans {e_trans:.2e} (floor {f_trans:.2e})')
        assert e_root <= U.FLOOR_MARGIN * f_root, (tag, case)
        assert e_trans <= U.FLOOR_MARGIN * f_trans, (tag, case)
        assert np.array_equal(new_pose[:, 3:].view(np.uint32), x['pose_rotvecs'][:, 3:].view(np.uint32))
        # the recorded floors are the reference's own results against this same restatement
        assert U.root_error(gold[f'{tag}.{case}.ref.new_root'], root64) == pytest.approx(f_root, rel=1e-3)
        assert U.trans_error(gold[f'{tag}.{case}.ref.new_trans'], trans64) == pytest.approx(f_trans, rel=1e-3)


def test_hostemu_shared_R_t(gold):
    """One R (3, 3) and t (3,) for the batch: the bits of the same values given per row."""
    md = _model('smpl')
    x, post = U.case_inputs(gold, 'smpl', 'pre_kid')
    B = x['pose_rotvecs'].shape[0]
    shared = dict(x, R=x['R'][0], t=x['t'][0])
    per = dict(x, R=np.tile(x['R'][:1], (B, 1, 1)), t=np.tile(x['t'][:1], (B, 1)))
    for a, b in zip(U.hostemu_forward(md, shared, post), U.hostemu_forward(md, per, post)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('case', list(U.GRAD_CASES))
@pytest.mark.parametrize('tag', list(U.MODELS))
def test_hostemu_backward(gold, tag, case):
    md = _model(tag)
    x, post = U.case_inputs(gold, tag, case, grad=True)
    cp, ct = gold[f'{tag}.grad.cot.pose'], gold[f'{tag}.grad.cot.trans']
    g = U.hostemu_backward(md, x, cp, ct, post)
    g64 = U.grads64(md, x, cp, ct, post)
    assert set(g64) == set(x)
    for k in g64:
        e, floor = U.grad_error(g[k], g64[k]), float(gold[f'{tag}.grad.{case}.gfloor.{k}'])
        print(f'{tag} {case} {k}: {e:.2e} (floor {floor:.2e})')
        assert e <= U.FLOOR_MARGIN * floor, (tag, case, k)
        # the recorded floor is the reference's fp32 gradient against this same restatement
        assert U.grad_error(gold[f'{tag}.grad.{case}.g32.{k}'], g64[k]) == pytest.approx(floor, rel=1e-3, abs=1e-12)
    assert np.array_equal(g['pose_rotvecs'][:, 3:], cp[:, 3:])  # the pose cotangent passes through untouched


@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_zero_root_gradient_is_the_true_derivative(gold, tag):
    """Row 4 (root rotation vector exactly 0, R != I): the root gradient against a central fp64 finite difference of
    <cot, mat2rotvec(R rotvec2mat(root))> — the reference's autograd returns 0 there.  Gate: 5 x the
    reference's recorded fp32 floor of the pose gradient of this model (the finite difference itself is good to 1e-9:
    step 1e-5, fp64)."""
    md = _model(tag)
    x, post = U.case_inputs(gold, tag, 'post_kid')
    x = {k: v[4:5] for k, v in x.items()}
    assert not x['pose_rotvecs'][0, :3].any() and not np.array_equal(x['R'][0], np.eye(3))
    rs = np.random.RandomState(3)
    cp = np.zeros_like(x['pose_rotvecs'])
    cp[0, :3] = rs.randn(3)
    g = U.hostemu_backward(md, x, cp, np.zeros((1, 3), np.float32), post)['pose_rotvecs'][0, :3]
    R, c, h = x['R'][0].astype(np.float64), cp[0, :3].astype(np.float64), 1e-5
    f = lambda r: float(c @ O.mat2rotvec(R @ O.rotvec2mat(r)))  # noqa: E731
    fd = np.array([(f(h * e) - f(-h * e)) / (2 * h) for e in np.eye(3)])
    assert np.abs(fd).max() > 0.1  # (not the reference's 0)
    e, floor = U.grad_error(g, fd), float(gold[f'{tag}.grad.post_kid.gfloor.pose_rotvecs'])
    print(f'{tag}: {e:.2e} (floor {floor:.2e})')
    assert e <= U.FLOOR_MARGIN * floor


def test_abi_symbols():
    from smplfitter_amd import _lib as L
    from smplfitter_amd import build

    assert L.SMPLFIT_ABI_VERSION == 7
    hdr = open(osp.join(HERE, '..', 'include', 'smplfit.h')).read()
    assert '#define SMPLFIT_ABI_VERSION 7' in hdr
    build.build(verbose=False)
    lib = L.load()
    for s in ('smplfit_rototranslate_f32', 'smplfit_rototranslate_backward_f32'):
        assert s in L.EXPORTED_SYMBOLS and f'int {s}(' in hdr
        assert getattr(lib, s).argtypes is not None  # exported and bound
    assert 'smplfit_rototranslate_args' in hdr and 'smplfit_rototranslate_backward_args' in hdr
    assert lib.smplfit_abi_version() == 7
    # the structs of the binding have the header's fields in the header's order
    import re

    for name, cls in (('smplfit_rototranslate_args', L.RototranslateArgs),
                      ('smplfit_rototranslate_backward_args', L.RototranslateBackwardArgs)):
        body = re.search(r'typedef struct ' + name + r' \{(.*?)\} ' + name + ';', hdr, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = [re.findall(r'(\w+);', line)[0] for line in body.splitlines() if ';' in line]
        assert fields == [f[0] for f in cls._fields_], name


def test_refusals_on_the_host():
    """The reference's message for missing inputs; no CPU path for CPU tensors."""
    from smplfitter_amd import synth
    from smplfitter_amd.pt import BodyModel

    root = synth.ensure_model_root(kinds=('smpl',), seed=0)
    m = BodyModel('smpl', 'neutral', model_root=f'{root}/smpl', num_betas=10)
    assert callable(m.rototranslate)
    eye, pose, betas, trans = torch.eye(3), torch.zeros(72), torch.zeros(10), torch.zeros(3)
    for kw in (dict(), dict(pose_rotvecs=pose, shape_betas=betas), dict(pose_rotvecs=pose, trans=trans),
               dict(shape_betas=betas, trans=trans)):
        with pytest.raises(ValueError, match='pose_rotvecs, shape_betas, and trans are required.'):
            m.rototranslate(eye, **kw)
    with pytest.raises(RuntimeError, match='There is no CPU path'):
        m.rototranslate(eye, None, pose, betas, trans)
