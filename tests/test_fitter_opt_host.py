"""BodyFitterOpt without a GPU: the two C-ABI symbols of the fit objective (the mesh-distance objective with a joint
term) and the size of its argument struct (tests/hostemu/hostemu_fit_objective.cpp), refused NULL arguments, the class's
export, signature and learning-rate schedule against the reference's fixture (tests/golden/make_golden_fitter_opt.py),
and the fixture's own consistency under the fp64 oracle."""

import ctypes as C
import inspect
import os
import os.path as osp
import subprocess

import numpy as np
import pytest

import fitter_opt_util as U
import util

HERE = osp.dirname(osp.abspath(__file__))
SRC = osp.join(HERE, 'hostemu', 'hostemu_fit_objective.cpp')
SO = osp.join(HERE, 'hostemu', '_build', 'libhostemu_fit_objective.so')
HEADER = osp.join(HERE, '..', 'include', 'smplfit.h')


@pytest.fixture(scope='module')
def gfo(golden):
    return golden('fitter_opt')


@pytest.fixture(scope='module')
def emu():
    deps = [SRC, HEADER]
    if not osp.exists(SO) or any(osp.getmtime(d) > osp.getmtime(SO) for d in deps):
        os.makedirs(osp.dirname(SO), exist_ok=True)
        tmp = SO + f'.tmp{os.getpid()}'
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', SRC, '-o', tmp], check=True)
        os.replace(tmp, SO)
    return C.CDLL(SO)


def test_symbols_and_struct_size(emu):
    from smplfitter_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    for s in ('smplfit_fit_objective_workspace_bytes', 'smplfit_fit_objective_f32'):
        assert s in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, s) is not None
    assert C.sizeof(_lib.FitObjectiveArgs) == emu.hostemu_sizeof_fit_objective_args()
    # the fields of smplfit_mesh_objective_args, plus target_joints, joint_weights and joint_scale
    mesh = [n for n, _ in _lib.MeshObjectiveArgs._fields_]
    fit = [n for n, _ in _lib.FitObjectiveArgs._fields_]
    assert [n for n in fit if n in mesh] == mesh
    assert [n for n in fit if n not in mesh] == ['target_joints', 'joint_weights', 'joint_scale']
    assert lib.smplfit_fit_objective_workspace_bytes(None, 8) == 0


def test_null_arguments_refused():
    from smplfitter_amd import _lib

    lib = _lib.load()
    assert lib.smplfit_fit_objective_f32(None, None) == _lib.SMPLFIT_ERR_BAD_ARG
    args = _lib.FitObjectiveArgs(batch=1)
    assert lib.smplfit_fit_objective_f32(None, C.byref(args)) == _lib.SMPLFIT_ERR_BAD_ARG


def test_class_signature_matches_reference(gfo):
    import smplfitter_amd.pt as pt
    from smplfitter_amd.pt import BodyFitterOpt

    assert 'BodyFitterOpt' in pt.__all__
    rep = lambda params: ['<required>' if p.default is p.empty else repr(p.default) for p in params]  # noqa: E731
    params = list(inspect.signature(BodyFitterOpt.fit).parameters.values())[1:]
    assert [p.name for p in params] == [str(n) for n in gfo['sig.names']]
    assert rep(params) == [str(d) for d in gfo['sig.defaults']]
    ctor = list(inspect.signature(BodyFitterOpt.__init__).parameters.values())[1:]
    n = len(gfo['init.names'])
    assert n == 2 and [p.name for p in ctor[:n]] == [str(x) for x in gfo['init.names']]
    assert rep(ctor[:n]) == [str(d) for d in gfo['init.defaults']]
    assert [p.name for p in ctor[n:]] == ['fused_objective'] and ctor[n].default is True
    for case in U.CASES:
        keys = {'pose_rotvecs', 'shape_betas', 'trans'} | ({'kid_factor'} if U.case_args(case)[1] else set())
        assert {str(k) for k in gfo[f'{case}.keys']} == keys


def test_learning_rates_match_reference(gfo):
    from smplfitter_amd.pt.bodyflipper_opt import refine_lr_at

    warmup = float(dict(zip(gfo['sig.names'], gfo['sig.defaults']))['warmup_ratio'])
    lr = float(dict(zip(gfo['sig.names'], gfo['sig.defaults']))['refine_lr'])
    for case in U.CASES:
        ref = gfo[f'{case}.lr']
        assert ref.shape == (U.STEPS,)
        ours = np.array([refine_lr_at(s, U.STEPS, lr, warmup) for s in range(U.STEPS)])
        assert np.abs(ours - ref).max() <= 1e-12 * np.abs(ref).max()


def test_fixture_consistency(model_root, gfo):
    """fp64 oracle forwards of the stored results reproduce obj0 / obj100 on the targets rebuilt from the stored
    parameters, and the reference's refinement improved on its closed-form fit."""
    _, md = util.load_md(model_root, 'smpl')
    om64 = util.O.OracleModel(md, np.float64, 'smpl')
    tv, tj = U.targets(om64, gfo)
    for case in U.CASES:
        joints, kid = U.case_args(case)
        obj = {}
        for steps in (0, U.STEPS):
            res = {str(k): gfo[f'{case}.s{steps}.{k}'] for k in gfo[f'{case}.keys']}
            assert ('kid_factor' in res) == kid
            obj[steps] = U.objective64(om64, res, tv, tj if joints else None, gfo['joint_weights'] if joints else None)
            assert abs(obj[steps] - float(gfo[f'{case}.obj{steps}'])) <= 1e-9 * obj[steps], (case, steps)
        assert obj[U.STEPS] < obj[0]
