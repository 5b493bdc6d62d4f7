"""BodyFlipperOpt without a GPU: the two C-ABI symbols of the mesh-distance objective and the size of its argument struct,
the per-vertex arithmetic of csrc/sf_stages.h built with g++ (tests/hostemu/hostemu_objective.cpp) against fp64 autograd of
torch.linalg.norm, the class's signature and learning-rate schedule against the reference's fixture
(tests/golden/make_golden_flip_opt.py), and the fixture's own consistency under the fp64 oracle."""

import ctypes as C
import inspect
import os
import os.path as osp
import subprocess

import numpy as np
import pytest
import torch

import flip_opt_util
import flip_util
import util

HERE = osp.dirname(osp.abspath(__file__))
SRC = osp.join(HERE, 'hostemu', 'hostemu_objective.cpp')
SO = osp.join(HERE, 'hostemu', '_build', 'libhostemu_objective.so')
CSRC = osp.join(HERE, '..', 'smplfitter_amd', 'csrc')
HEADER = osp.join(HERE, '..', 'include', 'smplfit.h')


@pytest.fixture(scope='module')
def gfo(golden):
    return golden('flip_opt')


@pytest.fixture(scope='module')
def emu():
    deps = [SRC, HEADER, osp.join(CSRC, 'sf_math.h'), osp.join(CSRC, 'sf_stages.h')]
    if not osp.exists(SO) or any(osp.getmtime(d) > osp.getmtime(SO) for d in deps):
        os.makedirs(osp.dirname(SO), exist_ok=True)
        tmp = SO + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', SRC, '-o', tmp], check=True)
        os.replace(tmp, SO)
    return C.CDLL(SO)


def test_symbols_and_abi(emu):
    from smplfitter_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    assert _lib.SMPLFIT_ABI_VERSION == 7 and lib.smplfit_abi_version() == 7
    for s in ('smplfit_mesh_objective_workspace_bytes', 'smplfit_mesh_objective_f32'):
        assert s in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, s) is not None
    assert C.sizeof(_lib.MeshObjectiveArgs) == emu.hostemu_sizeof_mesh_objective_args()
    assert lib.smplfit_mesh_objective_workspace_bytes(None, 8) == 0


def test_null_arguments_refused():
    from smplfitter_amd import _lib

    lib = _lib.load()
    assert lib.smplfit_mesh_objective_f32(None, None) == _lib.SMPLFIT_ERR_BAD_ARG
    args = _lib.MeshObjectiveArgs(batch=1)
    assert lib.smplfit_mesh_objective_f32(None, C.byref(args)) == _lib.SMPLFIT_ERR_BAD_ARG


def _vertex(emu, v, t, sw):
    n = len(sw)
    g, term = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    emu.hostemu_mesh_objective_vertex(p(v), p(t), p(sw), n, p(g), p(term))
    return g, term


def test_vertex_objective_against_fp64(emu):
    """sf::mesh_objective_vertex on 1000 random (v, t, w) triples, centimetre residuals, scale = 1 / (8 * 6890): the
    cotangent within 4 fp32 ulps of scale * w (one subtraction, one rsqrt-class operation and two multiplies; |r| / |r|
    <= 1), the loss term within 4 ulps of itself."""
    rs = np.random.RandomState(0)
    n = 1000
    v = rs.randn(n, 3).astype(np.float32)
    t = (v + 0.03 * rs.randn(n, 3)).astype(np.float32)
    w = rs.uniform(0, 2, n).astype(np.float32)
    sw = (np.float32(1.0 / (8 * 6890)) * w).astype(np.float32)
    g, term = _vertex(emu, v, t, sw)
    v64 = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    d64 = torch.linalg.norm(v64 - torch.tensor(t, dtype=torch.float64), dim=-1)
    terms64 = torch.tensor(sw, dtype=torch.float64) * d64
    g64, = torch.autograd.grad(terms64.sum(), v64)
    ulp = np.spacing(sw).astype(np.float64)
    err = np.abs(g - g64.numpy()).max(1) / ulp
    print(f'[objective] cotangent: worst {err.max():.2f} ulp of scale * w')
    assert err.max() <= 4.0
    terr = np.abs(term - terms64.detach().numpy()) / np.spacing(term).astype(np.float64)
    print(f'[objective] loss term: worst {terr.max():.2f} ulp')
    assert terr.max() <= 4.0


def test_vertex_objective_zero_residual_and_weight(emu):
    rs = np.random.RandomState(1)
    v = rs.randn(8, 3).astype(np.float32)
    sw = rs.uniform(0.5, 2, 8).astype(np.float32)
    g, term = _vertex(emu, v, v.copy(), sw)  # residual exactly 0: what torch.linalg.norm's backward gives
    assert np.all(g == 0) and np.all(term == 0)
    t = (v + 0.03 * rs.randn(8, 3)).astype(np.float32)
    g, term = _vertex(emu, v, t, np.zeros(8, np.float32))  # weight 0
    assert np.all(g == 0) and np.all(term == 0)


def test_class_signature_matches_reference(gfo):
    import smplfitter_amd.pt as pt
    from smplfitter_amd.pt import BodyFlipperOpt

    assert 'BodyFlipperOpt' in pt.__all__
    params = list(inspect.signature(BodyFlipperOpt.flip).parameters.values())[1:]
    assert [p.name for p in params] == [str(n) for n in gfo['sig.names']]
    assert ['<required>' if p.default is p.empty else repr(p.default) for p in params] == \
        [str(d) for d in gfo['sig.defaults']]
    assert sorted(str(k) for k in gfo['keys']) == sorted(flip_util.FLIP_KEYS)
    ctor = inspect.signature(BodyFlipperOpt.__init__).parameters
    assert list(ctor)[1] == 'body_model' and ctor['fused_objective'].default is True


def test_learning_rates_match_reference(gfo):
    from smplfitter_amd.pt.bodyflipper_opt import refine_lr_at

    for tag in flip_util.FLIP_MODELS:
        for case in flip_opt_util.CASES:
            ref = gfo[f'{tag}.{case}.lr']
            assert ref.shape == (flip_opt_util.STEPS,)
            ours = np.array([refine_lr_at(s, flip_opt_util.STEPS, 0.03, 0.1) for s in range(flip_opt_util.STEPS)])
            assert np.abs(ours - ref).max() <= 1e-12 * np.abs(ref).max()
    # int(5 * 0.1) == 0: no warm-up steps, no division by zero; the half cosine starts at the full rate
    five = [refine_lr_at(s, 5, 0.03, 0.1) for s in range(5)]
    assert five[0] == 0.03 and all(a > b for a, b in zip(five, five[1:])) and five[-1] > 0
    assert five == [0.03 * 0.5 * (1.0 + np.cos(np.pi * s / 5)) for s in range(5)]
    assert refine_lr_at(0, 1, 0.03, 0.1) == 0.03


def test_grad_inputs_raise_on_host(model_root, gfo, data_root_fat, monkeypatch):
    from smplfitter_amd.pt import BodyFlipperOpt, BodyModel

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    m = BodyModel('smpl', 'neutral', model_root=f'{model_root}/{util.model_dir("smpl")}', num_betas=10)
    fl = BodyFlipperOpt(m)
    pose, betas, trans = (torch.from_numpy(gfo[f'smpl.{k}']) for k in ('pose', 'betas', 'trans'))
    with pytest.raises(NotImplementedError):
        fl.flip(pose, betas.clone().requires_grad_(), trans, refine_steps=3)


@pytest.mark.parametrize('tag', ['smpl', 'smplx'])
def test_fixture_consistency(tag, model_root, gfo, data_root_fat, monkeypatch):
    """fp64 oracle forwards of the stored results reproduce obj0 / obj100, and the reference's refinement improved on
    its closed-form flip."""
    from smplfitter_amd.pt.bodyflipper import mirror_csr_for

    monkeypatch.setenv('DATA_ROOT', data_root_fat)
    kind = 'smplx' if tag == 'smplx' else 'smpl'
    _, md = util.load_md(model_root, flip_util.FLIP_MODELS[tag])
    om64 = util.O.OracleModel(md, np.float64, kind)
    mirror = mirror_csr_for(md.num_vertices)
    for case in flip_opt_util.CASES:
        _, with_kid = flip_util.case_args(case)
        target = flip_opt_util.target64(om64, mirror, gfo[f'{tag}.pose'], gfo[f'{tag}.betas'], gfo[f'{tag}.trans'],
                                        gfo[f'{tag}.kid'] if with_kid else None)
        obj = {}
        for steps in (0, flip_opt_util.STEPS):
            res = {k: gfo[f'{tag}.{case}.s{steps}.{k}'] for k in flip_util.FLIP_KEYS}
            obj[steps] = flip_opt_util.objective64(om64, res, target)
            assert abs(obj[steps] - float(gfo[f'{tag}.{case}.obj{steps}'])) <= 1e-9 * obj[steps], (tag, case, steps)
        assert obj[flip_opt_util.STEPS] < obj[0]
