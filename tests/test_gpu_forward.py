"""-m gpu: BodyModel.forward (smplfit_forward_ex_f32) against the fp64 oracle on every vertex route, model kind and batch
edge, with the input forms and values where the arithmetic branches; batch independence and determinism over every row;
guard regions around the outputs and the workspace.

Every fit test at scale builds its targets with this forward, and the fp64 oracle is then given those same targets: a
forward wrong on some instances of a large or ragged batch would pass them all.  Forward is a pure per-instance
function, so it is compared here directly: ``util.forward64`` (checked against the reference's goldens by
tests/test_forward_reference.py) on the inputs of ``util.forward_inputs``; every row up to 300 instances, about 64 rows
above (``util.forward_rows``: both ends, both sides of the 64 / 128 / 256 boundaries near the tail, a seeded scatter).

Gates (fp64 reference): vertices and joints |ours - ref| <= GATE_M[model] + 4 ulp_fp32(|ref|) (the ulp term only
matters for the instance translated by ~1000 m), orientations <= 1e-6 (5e-7 for rel_rotmats).  GATE_M is
util.FWD_GATE_M = 2e-6 m, tightened to about twice the largest error observed on one MI355X where that is lower (the
far instance left out; every case prints its batches as ``[fwd]`` lines).  Observed maxima over all batches of a case
(vertices and joints in metres), vertices / joints / orientations:

    smpl         batch-major       split-bf16 GEMM 1.2e-6 / 4.0e-7 / 6.6e-7   fp32-MFMA GEMM 1.0e-6 / 4.0e-7 / 6.6e-7
                 wave-per-instance split-bf16 GEMM 8.9e-7 / 4.0e-7 / 6.6e-7   fp32-MFMA GEMM 7.7e-7 / 4.0e-7 / 6.6e-7
    smplx        batch-major       tiled split-bf16 1.3e-6 / 5.8e-7 / 7.4e-7  fp32-MFMA GEMM 1.7e-6 / 5.8e-7 / 7.4e-7
                 wave-per-instance (fp32-MFMA GEMM) 1.6e-6 / 5.8e-7 / 7.4e-7
    smplxfat     batch-major 1.3e-6 / 4.5e-7 / 7.4e-7       wave-per-instance 1.9e-6 / 4.5e-7 / 7.4e-7
    smpl1024     batch-major 8.2e-7 / 5.4e-7 / 6.4e-7       wave-per-instance 8.7e-7 / 5.4e-7 / 6.4e-7
    smpl_w6      batch-major 1.2e-6 / 4.2e-7 / 6.8e-7       wave-per-instance 7.5e-7 / 4.2e-7 / 6.8e-7
    smplx_w6     batch-major 1.3e-6 / 5.8e-7 / 7.4e-7       wave-per-instance 1.6e-6 / 5.8e-7 / 7.4e-7
    smpl_rnd     batch-major 9.3e-7 / 4.2e-7 / 6.8e-7       wave-per-instance 7.4e-7 / 4.2e-7 / 6.8e-7
    smpl_b16     batch-major 8.5e-7 / 4.2e-7 / 6.8e-7       wave-per-instance 1.1e-6 / 4.2e-7 / 6.8e-7
    smpl_w6_b16  batch-major 9.0e-7 / 4.2e-7 / 6.8e-7       wave-per-instance 8.7e-7 / 4.2e-7 / 6.8e-7
    smpl_b32     general 1.5e-6 / 6.8e-7 / 5.9e-7
    smpl_w12     general 1.0e-6 / 4.6e-7 / 5.9e-7
    smpl_b300    general 2.0e-6 / 5.0e-7 / 6.5e-7
    input forms  smpl 8.7e-7 / 4.6e-7 / 4.7e-7, smplx 1.8e-6 / 4.6e-7 / 6.5e-7, smpl_b16 1.1e-6 / 3.5e-7 / 4.7e-7;
                 rel_rotmats orientations 2.4e-7

smpl_b300 sits at its fp32 floor: its 300 shape terms summed in fp32 (even at the 0.15 x betas util.forward_inputs gives
models of more than 32 betas; +-5 on every column is a 36 m lever, 8.4e-6 m observed, as a plain sequential fp32 sum)
round to 2.4e-6 m on these inputs, so its gate is twice the observed 2.0e-6.
"""

import ctypes as C

import numpy as np
import pytest
import torch

import util
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


# name -> (directory under the model root, num_betas, the kernel family kernel_path() must report); the golden kinds are
# built by test_gpu_parity.get_model (vertex subset of smpl1024), the others directly
MODELS = {
    'smpl': (None, 10, 'batch-major'), 'smplx': (None, 10, 'batch-major'), 'smplxfat': (None, 10, 'batch-major'),
    'smpl1024': (None, 10, 'batch-major'),
    'smpl_w6': (None, 10, 'batch-major'), 'smplx_w6': (None, 10, 'batch-major'), 'smpl_rnd': (None, 10, 'batch-major'),
    'smpl_b16': ('smpl_b16', 16, 'batch-major'), 'smpl_w6_b16': ('smpl_w6_b16', 16, 'batch-major'),
    'smpl_b32': ('smpl_b32', 32, 'general'), 'smpl_w12': ('smpl_w12', 10, 'general'),
    'smpl_b300': ('smpl_b300', None, 'general'),
}
BATCHES = {
    'smpl': [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 767, 768, 769, 1000, 4097, 32768],
    **{n: [1, 255, 256, 257, 300, 769, 2049] for n in ('smplx', 'smplxfat', 'smplx_w6')},
    **{n: [1, 65, 257, 769, 4097] for n in ('smpl_w6', 'smpl_rnd', 'smpl_b16', 'smpl_w6_b16')},
    'smpl1024': [1, 65, 257, 769, 16384],
    'smpl_b32': [1, 65, 257, 769, 2049], 'smpl_w12': [1, 65, 257, 769, 2049],
    'smpl_b300': [1, 65, 96],  # (the general path's per-call workspace holds an S x S fp64 system per instance)
}
# vertex / joint gate per model (m, + 4 ulp): util.FWD_GATE_M, tightened to about twice the largest observed error where
# that is below it, smpl_b300 at twice its fp32 floor (module docstring); orientations: GATE_O, GATE_O_REL for
# rel_rotmats (observed 2.4e-7: the reference composes the same rounded factors in fp64)
GATE_M = {n: util.FWD_GATE_M for n in MODELS}
GATE_M.update(smpl1024=1.7e-6, smpl_rnd=1.8e-6, smpl_w6_b16=1.8e-6, smpl_b300=4e-6)
GATE_O, GATE_O_REL = 1e-6, 5e-7

_models, _refs = {}, {}


def _model(name, model_root, golden, dev):
    """(BodyModel, fp64 OracleModel) of a kind, cached for the module."""
    if name not in _models:
        from smplfitter_amd import modelio
        from smplfitter_amd.pt import BodyModel

        d, nb, _ = MODELS[name]
        if d is None:
            g = golden(name)
            m, _ = get_model(model_root, name, g, dev)
            kind, md = util.load_md(model_root, name, g)
        else:
            m = BodyModel('smpl', 'neutral', model_root=f'{model_root}/{d}', num_betas=nb, device=dev)
            kind, md = 'smpl', modelio.load_model('smpl', 'neutral', model_root=f'{model_root}/{d}', num_betas=nb)
        _models[name] = (m, util.O.OracleModel(md, np.float64, kind))
    return _models[name]


def _ref(name, om, B, form='pose', seed=0):
    """The fp64 reference of one input form over B instances (util.Ref64; its inputs on the device as .dev)."""
    key = (name, B, form, seed)
    if key not in _refs:
        x = util.forward_inputs(B, om.J, om.S, seed=seed)
        glob32, rel32 = util.rotation_forms(x['pose_rotvecs'], om.parents)
        p, b, tr, k = x['pose_rotvecs'], x['shape_betas'], x['trans'], x['kid_factor']
        forms = dict(
            pose=dict(pose_rotvecs=p, shape_betas=b, trans=tr),
            glob=dict(glob_rotmats=glob32, shape_betas=b, trans=tr),
            rel=dict(rel_rotmats=rel32, shape_betas=b, trans=tr),
            norot=dict(shape_betas=b, trans=tr),
            nobetas=dict(pose_rotvecs=p, trans=tr),
            betas4=dict(pose_rotvecs=p, shape_betas=np.ascontiguousarray(b[:, :4]), trans=tr),
            betas10=dict(pose_rotvecs=p, shape_betas=np.ascontiguousarray(b[:, :10]), trans=tr),
            notrans=dict(pose_rotvecs=p, shape_betas=b),
            trans13=dict(pose_rotvecs=p, shape_betas=b, trans=np.ascontiguousarray(tr[:1])),
            kid=dict(pose_rotvecs=p, shape_betas=b, trans=tr, kid_factor=k),
            kidscalar=dict(pose_rotvecs=p, shape_betas=b, trans=tr, kid_factor=np.ascontiguousarray(k[:1])),
        )
        r = util.Ref64(om, **forms[form])
        r.dev = {a: torch.from_numpy(v).to('cuda:0') for a, v in forms[form].items()}
        _refs[key] = r
    return _refs[key]


def _slice(dev_inputs, B):
    """The first B instances of the device inputs; a (1, 3) translation and a one-element kid factor stay as they are."""
    return {k: (v if v.shape[0] == 1 and k in ('trans', 'kid_factor') else v[:B]) for k, v in dev_inputs.items()}


def _errors(fw, rows, ref, dev):
    """Errors of the forward result at ``rows``: gated (util.forward_errors) and raw maxima without the far instance."""
    ti = torch.from_numpy(rows).to(dev)
    ours = {k: v[ti].cpu().numpy() for k, v in fw.items()}
    r = ref.rows(rows)
    ev, ej, eo = util.forward_errors(ours, r)
    near = rows != util.FWD_FAR
    raw = [float(np.abs(ours[k][near].astype(np.float64) - r[k][near]).max()) if k in ours and near.any() else 0.0
           for k in ('vertices', 'joints')]
    return dict(v=ev, j=ej, o=eo, v_raw=raw[0], j_raw=raw[1])


def _set_route(route, gemm, smplfit_env):
    smplfit_env('SMPLFIT_BM_FORWARD', '0' if route == 'wave' else None)
    smplfit_env('SMPLFIT_GEMM', 'f32' if gemm == 'f32' else None)


def _route_cases():
    for name, (_, _, path) in MODELS.items():
        routes = ['bm', 'wave'] if path == 'batch-major' else ['wave' if path == 'wave-per-instance' else 'general']
        for route in routes:
            for gemm in (['bf16x3', 'f32'] if name in ('smpl', 'smplx') else ['default']):
                yield pytest.param(name, route, gemm, id=f'{name}-{route}-{gemm}')


def _check_route(m, name, route, gemm, dev):
    """The kernels a case claims: the model's kernel family (kernel_path), and on the SMPL / SMPL-X default cases the
    split-bf16 GEMM (gemm_vgprs >= 256: k_posedirs_gemm_bf16x3 for SMPL on both routes, k_split_features +
    k_posedirs_gemm_bf16x3_tiled for SMPL-X on the batch-major route — its wave route runs k_posedirs_gemm<false>, the
    fp32 MFMA, whatever SMPLFIT_GEMM says).  SMPLFIT_GEMM=f32: k_posedirs_gemm_as<104, *> (SMPL) / k_posedirs_gemm (SMPL-X).
    Returns the line the case prints."""
    path = m.kernel_path()
    assert path == MODELS[name][2], (name, path)
    vgprs = m._native(dev).info.gemm_vgprs
    if gemm == 'bf16x3':
        assert vgprs >= 256, f'{name}: the split-bf16 GEMM does not run (gemm_vgprs {vgprs}): the case would test a fallback'
    return f'{path}{" + SMPLFIT_BM_FORWARD=0" if route == "wave" and path == "batch-major" else ""}, gemm {gemm} (vgprs {vgprs})'


def _gate(errs, name, rel=False):
    """The failed gates of one result (empty: passed)."""
    g, go = GATE_M[name], GATE_O_REL if rel else GATE_O
    bad = [k for k, lim in (('v', g), ('j', g), ('o', go)) if not errs[k] <= lim]  # (nan for vertices: not returned)
    return [b for b in bad if not (b == 'v' and np.isnan(errs['v']))]


def _line(tag, e):
    return (f'[fwd] {tag}: vertices {e["v_raw"]:.2e} (excess {e["v"]:.2e}) joints {e["j_raw"]:.2e} (excess {e["j"]:.2e}) '
            f'orientations {e["o"]:.2e}')


@pytest.mark.parametrize('name,route,gemm', list(_route_cases()))
def test_forward_vs_fp64(name, route, gemm, model_root, golden, dev, smplfit_env):
    """Route x model x batch: every batch of BATCHES[name] on the route the case names against the fp64 oracle; the
    batches are prefixes of one input set (util.forward_inputs: zero, tiny, large and near-pi rotations mixed per joint,
    betas up to +-5, one instance ~1000 m away).  The batch-major forward runs k_fill_shape, the transposed GEMM,
    k_transpose_targets, the forward-only LBS pass on the kShareLbsAll table (fine up to 768 instances, coarse above)
    and k_unlayout_vertices; route 'wave' (SMPLFIT_BM_FORWARD=0) the wave-per-instance LBS kernel behind the
    instance-major GEMM; 'general' the general path's kernels."""
    m, om = _model(name, model_root, golden, dev)
    _set_route(route, gemm, smplfit_env)
    desc = _check_route(m, name, route, gemm, dev)
    ref = _ref(name, om, max(BATCHES[name]))
    x = ref.dev
    bad = []
    for B in BATCHES[name]:
        fw = m(x['pose_rotvecs'][:B], x['shape_betas'][:B], x['trans'][:B])
        e = _errors(fw, util.forward_rows(B), ref, dev)
        del fw
        print(_line(f'{name:11s} {route:7s} {gemm:7s} B={B:5d} [{desc}]', e))
        if _gate(e, name):
            bad.append((B, e))
    assert not bad, bad


def _form_cases():
    for name in ('smpl', 'smplx', 'smpl_b16'):
        for route in ('bm', 'wave'):
            yield pytest.param(name, route, id=f'{name}-{route}')


@pytest.mark.parametrize('name,route', list(_form_cases()))
def test_forward_input_forms(name, route, model_root, golden, dev, smplfit_env):
    """The input forms of BodyModel.forward at a ragged coarse batch (769) and at B = 1: pose rotation vectors, global
    rotations (composed in fp64, rounded once), relative rotations (the chain inside k_forward_joint; reference: the
    oracle fed their fp64 composition), no rotation input, no betas, 4 betas, 10 of 16 betas, no translation, a (1, 3)
    translation, a per-instance and a one-element kid factor (the kid handle).  return_vertices=False gives joints and
    orientations bit for bit equal to the call that returns vertices."""
    m, om = _model(name, model_root, golden, dev)
    _set_route(route, 'default', smplfit_env)
    assert m.kernel_path() == 'batch-major' and m.kernel_path(enable_kid=True) == 'batch-major'
    forms = ['pose', 'glob', 'rel', 'norot', 'nobetas', 'betas4'] + (['betas10'] if om.S == 16 else []) + \
            ['notrans', 'trans13', 'kid', 'kidscalar']
    bad = []
    for form in forms:
        ref = _ref(name, om, 769, form)
        for B in (769, 1):
            x = _slice(ref.dev, B)
            fw = m(**x)
            e = _errors(fw, util.forward_rows(B), ref, dev)
            j = m(**x, return_vertices=False)
            assert 'vertices' not in j
            for k in ('joints', 'orientations'):
                assert torch.equal(j[k], fw[k]), (form, B, k)
            del fw, j
            print(_line(f'{name:9s} {route:4s} {form:9s} B={B:4d}', e))
            if _gate(e, name, rel=form == 'rel'):
                bad.append((form, B, e))
    assert not bad, bad


# slices of a batch that cross the 64 / 128 / 256 boundaries and the fine / coarse limit (768), and single instances
_SLICES = [(0, 1), (64, 65), (60, 70), (120, 140), (250, 262), (700, 800), (767, 769), (0, 769), (0, 768), (1000, 1300)]


@pytest.mark.parametrize('name,B', [('smpl', 4097), ('smplx', 2049)])
def test_forward_batch_independence(name, B, model_root, golden, dev):
    """On the default route an instance's forward output does not depend on the batch it sits in: forward(X)[s] is bit
    for bit forward(X[s]) for slices across every block, tile and table boundary, and two calls on the same inputs are
    bit for bit equal.  The GEMM and the forward LBS pass do no reduction whose order depends on an instance's
    position; the fine and coarse cell tables (slices of <= 768 instances against the whole batch) compute every vertex
    with the same arithmetic.  Covers the rows test_forward_vs_fp64 does not sample."""
    m, om = _model(name, model_root, golden, dev)
    x = _ref(name, om, max(BATCHES[name])).dev
    x = {k: v[:B] for k, v in x.items()}
    a = m(x['pose_rotvecs'], x['shape_betas'], x['trans'])
    b = m(x['pose_rotvecs'], x['shape_betas'], x['trans'])
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for s0, s1 in _SLICES + [(B - 1, B), (B - 70, B), (B - 300, B - 1)]:
        c = m(x['pose_rotvecs'][s0:s1], x['shape_betas'][s0:s1], x['trans'][s0:s1])
        for k in a:
            assert torch.equal(a[k][s0:s1], c[k]), (s0, s1, k)


GUARD = 1 << 20


def _guarded(nbytes, dev):
    buf = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=dev)
    buf.fill_(0xA5)
    return buf, buf[GUARD:GUARD + nbytes]


def _intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


@pytest.mark.parametrize('name,B', [('smpl', 1), ('smpl', 65), ('smpl', 769), ('smpl', 4097), ('smplx', 257), ('smplx', 769)])
@pytest.mark.parametrize('route', ['bm', 'wave'])
def test_forward_guards(name, B, route, model_root, golden, dev, smplfit_env):
    """smplfit_forward_ex_f32 called directly with vertices, joints, orientations and the workspace each between two
    1 MB guard regions: outputs pre-filled with NaN, the workspace once zeroed and once filled with a NaN pattern.
    Every guard byte survives, every output element is written and finite, and the two workspace fills give the same
    bits — no kernel writes outside the rows it owns or reads a workspace cell nobody wrote."""
    from smplfitter_amd import _lib

    m, om = _model(name, model_root, golden, dev)
    _set_route(route, 'default', smplfit_env)
    x = {k: v[:B].contiguous() for k, v in _ref(name, om, max(BATCHES[name])).dev.items()}
    h = m._native(dev)
    J, V = m.num_joints, m.num_vertices
    out = {}
    for fill in ('zero', 'nan'):
        bufs = {k: _guarded(4 * n, dev) for k, n in (('v', B * V * 3), ('j', B * J * 3), ('o', B * J * 9))}
        for _, o in bufs.values():
            o.view(torch.float32).fill_(float('nan'))
        nws = h.workspace_bytes(B)
        wbuf, ws = _guarded(nws, dev)
        assert ws.data_ptr() % 256 == 0
        if fill == 'zero':
            ws.zero_()
        else:
            ws.view(torch.int32)[: nws // 4].fill_(0x7FC00000 | 0x1234)
        args = _lib.ForwardArgs(
            pose_rotvecs=x['pose_rotvecs'].data_ptr(), shape_betas=x['shape_betas'].data_ptr(), num_betas_given=10,
            trans=x['trans'].data_ptr(), batch=B, vertices=bufs['v'][1].data_ptr(), joints=bufs['j'][1].data_ptr(),
            orientations=bufs['o'][1].data_ptr(), workspace=ws.data_ptr(), workspace_bytes=nws,
            hip_stream=torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().smplfit_forward_ex_f32(h.ptr, C.byref(args)))
        torch.cuda.synchronize()
        assert _intact(wbuf, nws), 'workspace guard written'
        for k, (buf, o) in bufs.items():
            assert _intact(buf, o.numel()), f'guard region of output {k} written'
            assert bool(torch.isfinite(o.view(torch.float32)).all()), f'output {k}: an element was not written'
        out[fill] = {k: o.clone() for k, (_, o) in bufs.items()}
        del bufs, wbuf, ws
    for k in out['zero']:
        assert torch.equal(out['zero'][k], out['nan'][k]), k
