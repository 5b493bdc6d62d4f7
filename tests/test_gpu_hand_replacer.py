"""-m gpu: HandReplacer on the HIP kernels.  The fused replace_hand (smplfit_replace_hands_f32: weighted fit with the (V)
weights read as one row, hand joints overwritten in the relative rotation matrices, forward, blend in the pass that writes
the result) against the reference's fixture (tests/golden/make_golden_hand_replacer.py), against the composition of the
public fit / forward / PyTorch blend, exact identity where the mix weight is 0, the returned parameters, the fallback
routes and the error paths.

Gate (hand_util.GATE, the flip tests' 1e-4 m max vertex L2); the fixture's own fp32-vs-fp64 floor is 1.7e-5 m."""

import ctypes as C
import os
import os.path as osp
import re

import numpy as np
import pytest
import torch

import hand_util

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gh(golden):
    return golden('hand_replacer')


_cache = {}


def get_replacer(gh, dev, num_betas=None):
    from smplfitter_amd.pt import HandReplacer

    if num_betas not in _cache:
        root = hand_util.data_root()
        _cache[num_betas] = HandReplacer(torch.from_numpy(gh['hand_pose_source']), model_root=f'{root}/body_models/smplh16',
                                         data_root=root, device=dev, num_betas=num_betas)
    return _cache[num_betas]


def fused(hr, dev, smplfit_env):
    smplfit_env('SMPLFIT_BM', None)
    assert hr._plan(dev) is not None
    return hr


def meshes(hr, B, seed, dev):
    """B noisy posed SMPL-H meshes on the device."""
    bm = hr.smplh_bm
    rs = np.random.RandomState(seed)
    pose = rs.randn(B, bm.num_joints, 3) * 0.1
    pose[:, 22:] *= 2.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    v = bm(t(pose.reshape(B, -1)), t(rs.randn(B, bm.num_betas) * 0.5), t(rs.randn(B, 3)))['vertices']
    return v + t(rs.randn(B, bm.num_vertices, 3) * 0.002)


def two_chunk_batch():
    """Just above the smallest batch a call with two chunks is cut at: every chunk is a multiple of 128 instances above
    the fine tables' largest batch (chunk_plan_n, SMPLFIT_FINE_MAX_B)."""
    src = open(osp.join(ROOT, 'smplfitter_amd', 'csrc', 'sf_tables.h')).read()
    fine = int(re.search(r'#define SMPLFIT_FINE_MAX_B (\d+)', src).group(1))
    return 2 * (fine // 128 + 1) * 128 + 3


def l2(a, b):
    return float((a.double() - b.double()).norm(dim=-1).max())


def test_replace_hand_golden(gh, dev, smplfit_env):
    """The fused replace_hand at B = 8 against the reference's vertices, on all stored vertices (every vertex with
    0 < mix < 1, a quarter of the hand vertices, every 53rd vertex).  Observed on an MI355X: max vertex L2 1.45e-5 m (the
    fixture's own fp32-vs-fp64 floor: 1.68e-5 m; gate 1e-4 m)."""
    hr = fused(get_replacer(gh, dev), dev, smplfit_env)
    hand_util.check_floor(gh['fp32_vs_fp64'])
    assert hr.smplh_bm.num_betas == 16 and hr.smplh_bm.kernel_path() == 'batch-major'
    verts = torch.from_numpy(gh['verts']).to(dev)
    out = hr.replace_hand(verts)
    assert out.shape == verts.shape and out.dtype == torch.float32
    err = hand_util.vertex_l2(out[:, torch.from_numpy(gh['out_idx']).to(dev)].cpu().numpy(), gh['out_vertices_sub'])
    print(f'[hand] fused vs reference: max vertex L2 {err:.2e} m (floor {float(gh["fp32_vs_fp64"]):.2e}, gate {hand_util.GATE:.0e})')
    assert err <= hand_util.GATE, err
    zero = torch.from_numpy(gh['hand_mix_weight'] == 0).to(dev)
    assert torch.equal(out[:, zero], verts[:, zero])


@pytest.mark.parametrize('B', [1, 3, 129])
def test_fused_matches_unfused(B, gh, dev, smplfit_env):
    """The fused call against fit + forward + PyTorch blend of the public entry points (the same fit kernels fed the (V)
    weights instead of a (B, V) tensor; the forward from rotation matrices instead of rotation vectors), and the
    returned parameters against the composition's."""
    _fused_vs_unfused(fused(get_replacer(gh, dev), dev, smplfit_env), B, dev)


@pytest.mark.usefixtures('two_chunks')
def test_fused_matches_unfused_two_chunks(gh, dev, smplfit_env):
    """The same just above the smallest batch that is cut into two chunks (the second one partial), with the chunk count
    pinned to two; the fit's chunks are joined before the forward runs over the whole batch."""
    hr = fused(get_replacer(gh, dev), dev, smplfit_env)
    B = two_chunk_batch()
    _fused_vs_unfused(hr, B, dev)


def _fused_vs_unfused(hr, B, dev):
    verts = meshes(hr, B, 7 + B, dev)
    a = hr._replace_fused(verts)
    assert a is not None
    b = hr._replace_unfused(verts)
    assert all(bool(torch.isfinite(x).all()) for x in a.values())
    err = l2(a['vertices'], b['vertices'])
    print(f'[hand] B = {B}: fused vs unfused max vertex L2 {err:.2e} m')
    assert err <= hand_util.GATE, err
    assert float((a['trans'] - b['trans']).abs().max()) <= 2e-5
    assert torch.equal(a['pose_rotvecs'][:, 66:], b['pose_rotvecs'][:, 66:])  # the replacement values themselves


def test_ten_betas_batch_major_fit(gh, dev, smplfit_env):
    """num_betas = 10: the weighted fit itself takes the batch-major kernels (the shared-row weight layout pass)."""
    hr = fused(get_replacer(gh, dev, num_betas=10), dev, smplfit_env)
    verts = meshes(hr, 70, 3, dev)
    a, b = hr._replace_fused(verts), hr._replace_unfused(verts)
    assert l2(a['vertices'], b['vertices']) <= hand_util.GATE
    zero = (hr.hand_mix_weight == 0).to(dev)
    assert torch.equal(a['vertices'][:, zero], verts[:, zero])


def test_identity_where_mix_is_zero(gh, dev, smplfit_env):
    """Bit-for-bit the input where mix == 0 — also when a few of those coordinates are very large but finite —, and the
    input tensor is left as it was."""
    hr = fused(get_replacer(gh, dev), dev, smplfit_env)
    zero = (hr.hand_mix_weight == 0).to(dev)
    verts = meshes(hr, 67, 21, dev)
    out = hr.replace_hand(verts)
    assert torch.equal(out[:, zero], verts[:, zero]) and not torch.equal(out[:, ~zero], verts[:, ~zero])
    big = verts.clone()
    idx = torch.nonzero(zero)[:, 0]
    big[0, idx[0], 0] = 3e30
    big[5, idx[17], 2] = -1e25
    big[66, idx[-1], 1] = 7e18
    keep = big.clone()
    out = hr.replace_hand(big)
    assert torch.equal(big, keep)
    assert torch.equal(out[:, zero], big[:, zero])
    clean = [b for b in range(67) if b not in (0, 5, 66)]
    assert bool(torch.isfinite(out[clean]).all())


def test_returned_parameters_reproduce_vertices(gh, dev, smplfit_env):
    hr = fused(get_replacer(gh, dev), dev, smplfit_env)
    verts = meshes(hr, 33, 5, dev)
    r = hr.replace_hand_with_params(verts)
    assert set(r) == {'vertices', 'pose_rotvecs', 'shape_betas', 'trans'}
    assert r['pose_rotvecs'].shape == (33, 156) and r['shape_betas'].shape == (33, 16) and r['trans'].shape == (33, 3)
    repl = torch.from_numpy(hand_util.replacement(gh['hand_pose_source'])).to(dev)
    assert torch.equal(r['pose_rotvecs'][:, 66:], repl.expand(33, -1))
    new = hr.smplh_bm(r['pose_rotvecs'], r['shape_betas'], r['trans'])['vertices']
    back = verts + (new - verts) * hr.hand_mix_weight.to(dev)[:, None]
    assert l2(back, r['vertices']) <= hand_util.GATE
    assert torch.equal(hr.replace_hand(verts), r['vertices'])  # deterministic, and the same call


def test_in_place(gh, dev, smplfit_env):
    """smplfit_replace_hands_f32 with out_vertices = vertices gives the bits of the out-of-place call."""
    from smplfitter_amd import _lib

    hr = fused(get_replacer(gh, dev), dev, smplfit_env)
    verts = meshes(hr, 70, 31, dev)
    ref = hr.replace_hand(verts)
    buf = verts.clone()
    plan = hr._plan(dev)
    ws = torch.empty(plan.workspace_bytes(70), dtype=torch.uint8, device=dev)
    args = _lib.ReplaceHandsArgs(vertices=buf.data_ptr(), batch=70, num_iter=3, out_vertices=buf.data_ptr(),
                                 workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                                 hip_stream=torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().smplfit_replace_hands_f32(plan.ptr, C.byref(args)))
    torch.cuda.synchronize()
    assert torch.equal(buf, ref) and not torch.equal(buf, verts)


def test_fallback_under_compile(gh, dev, smplfit_env):
    hr = fused(get_replacer(gh, dev), dev, smplfit_env)
    verts = meshes(hr, 5, 9, dev)
    eager = hr.replace_hand(verts)
    compiled = torch.compile(hr.replace_hand, backend='aot_eager', fullgraph=True)(verts)
    assert l2(eager, compiled) <= hand_util.GATE
    assert torch.equal(compiled, hr._replace_unfused(verts)['vertices'])


def test_fallback_after_options_reload(gh, dev, smplfit_env):
    """A plan made while the batch-major kernels applied, then SMPLFIT_BM=0: smplfit_replace_hands_f32 reports
    unsupported and that call takes fit + forward + blend."""
    hr = fused(get_replacer(gh, dev), dev, smplfit_env)
    verts = meshes(hr, 40, 13, dev)
    a = hr.replace_hand(verts)
    smplfit_env('SMPLFIT_BM', '0')
    assert hr._replace_fused(verts) is None
    late = hr.replace_hand(verts)
    assert torch.equal(late, hr._replace_unfused(verts)['vertices'])
    assert l2(a, late) <= hand_util.GATE
    zero = (hr.hand_mix_weight == 0).to(dev)
    assert torch.equal(late[:, zero], verts[:, zero])


def test_errors(gh, dev, smplfit_env):
    from smplfitter_amd import _lib

    hr = fused(get_replacer(gh, dev), dev, smplfit_env)
    verts = meshes(hr, 4, 2, dev)
    with pytest.raises(NotImplementedError):
        hr.replace_hand(verts.clone().requires_grad_())
    with pytest.raises(ValueError):
        hr.replace_hand(verts[:, :100])
    empty = hr.replace_hand_with_params(verts[:0])
    assert empty['vertices'].shape == (0, 6890, 3) and empty['pose_rotvecs'].shape == (0, 156)
    # a workspace one byte short is refused before anything is enqueued; so are null meshes
    plan = hr._plan(dev)
    ws = torch.empty(plan.workspace_bytes(4), dtype=torch.uint8, device=dev)
    out = torch.full_like(verts, float('nan'))
    args = _lib.ReplaceHandsArgs(vertices=verts.data_ptr(), batch=4, num_iter=3, out_vertices=out.data_ptr(),
                                 workspace=ws.data_ptr(), workspace_bytes=ws.numel() - 1,
                                 hip_stream=torch.cuda.current_stream(dev).cuda_stream)
    lib = _lib.load()
    assert lib.smplfit_replace_hands_f32(plan.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_WORKSPACE
    args.workspace_bytes = ws.numel()
    args.vertices = None
    assert lib.smplfit_replace_hands_f32(plan.ptr, C.byref(args)) == _lib.SMPLFIT_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the parameter outputs are optional
    args.vertices = verts.data_ptr()
    _lib.check(lib.smplfit_replace_hands_f32(plan.ptr, C.byref(args)))
    torch.cuda.synchronize()
    assert torch.equal(out, hr.replace_hand(verts))


def test_replace_hands_guards(gh, dev, smplfit_env):
    """smplfit_replace_hands_f32 at B = 65 with the parameter outputs NULL (the regions at the front of the workspace
    take the fit's results), out_vertices and a workspace of exactly the queried size each between two 1 MB guard
    regions, the output pre-filled with NaN, the workspace once zeroed and once filled with a NaN pattern: every guard
    byte survives, every output element is written and finite, the two fills give the same bits.  A workspace one byte
    short is refused before anything is enqueued."""
    from smplfitter_amd import _lib
    from test_gpu_flipper import _guarded, _intact

    hr = fused(get_replacer(gh, dev), dev, smplfit_env)
    B = 65
    verts = meshes(hr, B, 41, dev)
    plan, lib = hr._plan(dev), _lib.load()
    nws = plan.workspace_bytes(B)
    mk = lambda out, ws, n: _lib.ReplaceHandsArgs(  # noqa: E731
        vertices=verts.data_ptr(), batch=B, num_iter=3, beta_regularizer=1.0, final_adjust_rots=1,
        out_vertices=out.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=n,
        hip_stream=torch.cuda.current_stream(dev).cuda_stream)
    res = {}
    for fill in ('zero', 'nan'):
        obuf, out = _guarded(4 * verts.numel(), dev)
        out.view(torch.float32).fill_(float('nan'))
        wbuf, ws = _guarded(nws, dev)
        assert ws.data_ptr() % 256 == 0
        if fill == 'zero':
            ws.zero_()
        else:
            ws.view(torch.int32)[: nws // 4].fill_(0x7FC00000 | 0x1234)
        _lib.check(lib.smplfit_replace_hands_f32(plan.ptr, C.byref(mk(out, ws, nws))))
        torch.cuda.synchronize()
        assert _intact(wbuf, nws), 'workspace guard written'
        assert _intact(obuf, out.numel()), 'guard region of out_vertices written'
        assert bool(torch.isfinite(out.view(torch.float32)).all()), 'out_vertices: an element was not written'
        res[fill] = out.clone()
        del obuf, out, wbuf, ws
    assert torch.equal(res['zero'], res['nan'])
    assert not torch.equal(res['zero'].view(torch.float32).view_as(verts), verts)  # (the hands were replaced)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    out = torch.full_like(verts, float('nan'))
    assert lib.smplfit_replace_hands_f32(plan.ptr, C.byref(mk(out, ws, nws - 1))) == _lib.SMPLFIT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())  # nothing was enqueued
