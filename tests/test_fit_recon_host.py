"""Host checks (no GPU) of the mesh-error step: the C-ABI of the new entry points on a host-only handle,
and the argument errors and the dispatch of ``BodyFitter`` / ``BodyModel.mesh_error`` with CPU tensors."""

import ctypes as C
import os.path as osp
import re

import pytest
import torch

import hostemu_util as H
import util
from smplfitter_amd import _lib, build

SYMBOLS = ('smplfit_mesh_error_workspace_bytes', 'smplfit_mesh_error_f32', 'smplfit_fit_recon_workspace_bytes',
           'smplfit_fit_recon_f32')
RECON = ['vertices', 'joints', 'vertex_error', 'joint_error']


@pytest.fixture(scope='module')
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def cpu_fitter(model_root):
    from smplfitter_amd.pt import BodyFitter, BodyModel

    m = BodyModel('smpl', 'neutral', model_root=f'{model_root}/{util.model_dir("smpl")}', num_betas=10)
    return m, BodyFitter(m)


def test_symbols_and_abi(lib):
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.smplfit_abi_version() == 7 == _lib.SMPLFIT_ABI_VERSION
    assert _lib.RECON_KEYS == tuple(RECON)
    # the structs of the binding have the header's fields in the header's order
    hdr = open(osp.join(osp.dirname(osp.abspath(__file__)), '..', 'include', 'smplfit.h')).read()
    assert '#define SMPLFIT_ABI_VERSION 7' in hdr
    for name, cls in (('smplfit_mesh_error_args', _lib.MeshErrorArgs), ('smplfit_fit_recon_args', _lib.FitReconArgs)):
        body = re.search(r'typedef struct ' + name + r' \{(.*?)\} ' + name + ';', hdr, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = [re.findall(r'(\w+);', line)[0] for line in body.splitlines() if ';' in line]
        assert fields == [f[0] for f in cls._fields_], name


@pytest.mark.parametrize('kid', [False, True])
def test_workspace_queries(lib, kid, model_root, golden):
    """The step alone takes a fit workspace; the fit with reconstruction puts the fit's global rotations (B, J, 9) and
    kid factors (B), each 256-byte aligned, in front of the fit's own workspace — with a plan of segments that call's;
    0 for a null handle, a batch <= 0 and a batch that is not the plan's."""
    kind, md = util.load_md(model_root, 'smpl', golden('smpl'))
    desc, keep = H.desc_from_md(md, kind, enable_kid=kid)
    h = _lib.Handle(desc, host_only=True)
    r = lambda n: (n + 255) // 256 * 256  # noqa: E731
    J = h.info.num_joints
    for B in (1, 64, 65, 129, 1795):
        assert h.mesh_error_workspace_bytes(B) == h.workspace_bytes(B) > 0
        assert h.fit_recon_workspace_bytes(B) == r(36 * B * J) + r(4 * B) + h.workspace_bytes(B)
    plan = _lib.ShareSegments([3, 5], host_only=True)
    assert h.fit_recon_workspace_bytes(8, plan) == r(36 * 8 * J) + r(4 * 8) + plan.workspace_bytes(h)
    assert h.fit_recon_workspace_bytes(9, plan) == 0
    assert h.fit_recon_workspace_bytes(0) == 0 and h.mesh_error_workspace_bytes(-1) == 0
    assert lib.smplfit_fit_recon_workspace_bytes(None, 8, None) == 0
    h.close()


def test_native_refusals_without_device(lib, model_root, golden):
    """Null arguments and a host-only handle are refused by both entries with an error, not a crash."""
    kind, md = util.load_md(model_root, 'smpl', golden('smpl'))
    desc, keep = H.desc_from_md(md, kind)
    h = _lib.Handle(desc, host_only=True)
    assert lib.smplfit_mesh_error_f32(h.ptr, None) == _lib.SMPLFIT_ERR_BAD_ARG
    assert lib.smplfit_fit_recon_f32(h.ptr, None, None, C.byref(_lib.FitReconArgs())) == _lib.SMPLFIT_ERR_BAD_ARG
    assert lib.smplfit_fit_recon_f32(h.ptr, None, None, None) == _lib.SMPLFIT_ERR_BAD_ARG  # the segments call's refusal
    a = _lib.MeshErrorArgs(batch=4)
    assert lib.smplfit_mesh_error_f32(h.ptr, C.byref(a)) == _lib.SMPLFIT_ERR_HIP
    assert b'host-only' in lib.smplfit_last_error()
    f = _lib.FitArgs(batch=4)
    assert lib.smplfit_fit_recon_f32(h.ptr, C.byref(f), None, C.byref(_lib.FitReconArgs())) == _lib.SMPLFIT_ERR_HIP
    h.close()


def test_python_argument_errors(cpu_fitter):
    """Checked before the device is touched: CPU tensors get the argument errors, not the no-CPU-path error."""
    m, f = cpu_fitter
    B, J, V = 4, m.num_joints, m.num_vertices
    tv, tj = torch.zeros(B, V, 3), torch.zeros(B, J, 3)
    pose, betas = torch.zeros(B, 3 * J), torch.zeros(B, 10)
    with pytest.raises(ValueError, match='joint_error'):
        f.fit(tv, requested_keys=['joint_error'])
    with pytest.raises(ValueError, match='joint_error'):
        f.fit_with_known_pose(pose, tv, requested_keys=['pose_rotvecs', 'joint_error'])
    with pytest.raises(ValueError, match='joint_error'):
        f.fit_with_known_shape(betas, tv, requested_keys=['joint_error'])
    for key in RECON:
        for opt in ('scale_target', 'scale_fit'):
            with pytest.raises(NotImplementedError, match=opt):
                f.fit(tv, tj, requested_keys=[key], **{opt: True})
            with pytest.raises(NotImplementedError, match=opt):
                f.fit_with_known_pose(pose, tv, tj, requested_keys=[key], **{opt: True})
        with pytest.raises(NotImplementedError, match='scale_fit'):
            f.fit_with_known_shape(betas, tv, tj, requested_keys=[key], scale_fit=True)
    # without the keys the scale options reach the device check as before
    with pytest.raises(RuntimeError, match='MI355X'):
        f.fit(tv, tj, scale_target=True)
    # mesh_error: forward's checks plus the target shapes
    with pytest.raises(ValueError, match='Only one rotation input'):
        m.mesh_error(tv, pose_rotvecs=pose, glob_rotmats=torch.zeros(B, J, 3, 3))
    with pytest.raises(ValueError, match='target_vertices must have shape'):
        m.mesh_error(tv[:, :-1], pose_rotvecs=pose)
    with pytest.raises(ValueError, match='target_joints must have shape'):
        m.mesh_error(tv, tj[:, :-1], pose_rotvecs=pose)
    with pytest.raises(ValueError, match='rows'):
        m.mesh_error(tv, pose_rotvecs=pose[:3])
    with pytest.raises(ValueError, match='Expected batched input'):
        m.mesh_error(tv, pose_rotvecs=pose[0])
    with pytest.raises(TypeError, match='numpy'):
        m.mesh_error(tv.numpy(), pose_rotvecs=pose)
    with pytest.raises(RuntimeError, match='MI355X'):  # valid arguments: no CPU path
        m.mesh_error(tv, tj, pose_rotvecs=pose, shape_betas=betas)
    empty = m.mesh_error(tv[:0], tj[:0], pose_rotvecs=pose[:0], return_mesh=True)
    assert {k: tuple(v.shape) for k, v in empty.items()} == dict(
        vertex_error=(0, V), joint_error=(0, J), vertices=(0, V, 3), joints=(0, J, 3))


def test_dispatch(cpu_fitter, monkeypatch):
    """``requested_keys`` without the new names takes the old call (no recon keys reach ``_fit_direct``, which then calls
    ``smplfit_fit_segments_f32``); with them, exactly the requested ones in the library's order."""
    m, f = cpu_fitter
    B = 2
    tv, tj = torch.zeros(B, m.num_vertices, 3), torch.zeros(B, m.num_joints, 3)
    seen = []

    def spy(*args):
        seen.append(args[-1])
        return dict(pose_rotvecs=None, shape_betas=None, trans=None, orientations=None, relative_orientations=None)

    monkeypatch.setattr(f, '_fit_direct', spy)
    f.fit(tv, tj)
    f.fit(tv, tj, requested_keys=['pose_rotvecs', 'relative_orientations', 'something_else'])
    f.fit(tv, tj, requested_keys=['joint_error', 'pose_rotvecs', 'vertices'])
    f.fit(tv, requested_keys=['vertex_error'])
    assert seen == [(), (), ('vertices', 'joint_error'), ('vertex_error',)]
