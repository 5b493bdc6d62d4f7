"""Hard inputs and exclusion-free criteria for the rotation primitives of sf_math.h, shared by the host build
(tests/test_hostemu.py) and the device build (tests/test_gpu_primitives.py): plain numpy, seeded, no GPU.

A *runner* is ``run(op, a, b, out_shape) -> float32 array`` with the operation numbers of smplfit_primitives_f32:
0 proj_so3 (a: n x 3 x 3), 1 rotvec2mat (a: n x 3), 2 mat2rotvec (a: n x 3 x 3), 3 align_unit_vectors (a, b: n x 3),
4 swing_twist (a: reference bone n x 3, b: n x 12 = target bone | centred cross-covariance, row-major).

Every ``check_*`` prints the figures it measured, asserts the gates, and returns the figures."""

import numpy as np

import util

O = util.O
DECADES = tuple(range(0, -13, -1))  # 10^0 .. 10^-12
PER_DECADE = 64
SCALES = (0, 60, -60)  # every proj_so3 family again as A * 2^60 and A * 2^-60 (exact in fp32)

# ---- gates (what they rest on is stated next to each check) --------------------------------------------------------------
PROPER_TOL = 1e-5       # |R R^T - I|, |det R - 1|: the gate of test_device_primitives
PROJ_OPT_TOL = 5e-7     # (s1 + s2 + d s3 - tr(R^T A)) / s1  (host 8.9e-8, device 8.9e-8 observed)
PROJ_DIST_TOL = 5e-7    # max|R - R_svd| * min(gap, 1)       (host 3.0e-8, device 3.0e-8 observed)
M2R_FLOOR = 1e-6        # |exp64(mat2rotvec(R)) - R|         (host 6.5e-7, device 5.7e-7, fp32 oracle 6.9e-7 observed)
M2R_ORACLE_TOL = 1e-5   # element-wise against the fp32 oracle: the gate of test_device_primitives
R2M_TOL = 5e-7          # * (1 + theta): rotvec2mat against fp64 Rodrigues, and its orthogonality (fp32 oracle 0.41, host 0.39, device 0.44 of it observed)
ALIGN_FLOOR = 1e-6      # |R a - b|
SWING_FLOOR = 5e-6      # swing_twist against the fp64 restatement (the gate of test_device_primitives; 7.9e-7 / 5.8e-7 observed)
ANTIPARALLEL_MIN = 1e-3  # align: the formula is ill-posed closer than this to pi, in the reference too


def _rot(rs, n):
    """n random proper rotations (fp64)."""
    Q, _ = np.linalg.qr(rs.randn(n, 3, 3))
    Q[:, :, 2] *= np.sign(np.linalg.det(Q))[:, None]
    return Q


def _perm(rs, n):
    """n random signed permutation matrices of determinant +1."""
    P = np.eye(3)[np.argsort(rs.rand(n, 3), axis=1)] * rs.choice([-1.0, 1.0], (n, 1, 3))
    P[:, :, 2] *= np.sign(np.linalg.det(P))[:, None]
    return P


def _unit(rs, n):
    v = rs.randn(n, 3)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perp(rs, a):
    p = np.cross(a, rs.randn(*a.shape))
    return p / np.linalg.norm(p, axis=-1, keepdims=True)


def exp64(rv):
    """Rodrigues in fp64."""
    return O.rotvec2mat(np.asarray(rv, np.float64))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


# ---- proj_so3 ---------------------------------------------------------------------------------------------------------
def proj_families(seed=0, per_decade=PER_DECADE):
    """name -> (A float32 (n, 3, 3), decade (n,)): U diag(s) V^T built in fp64 and rounded to fp32.

    refl_gap   det < 0 and s2 - s3 = 10^e s1: the double top eigenvalue of Horn's matrix under a reflection
    rank1      s2, s3 ~ 10^e s1, either sign of the determinant
    small_s3   s3 = +-10^e s1 beside a separated s2
    near_rot   a rotation plus 10^e of noise (what a fit feeds the projection)
    axis_sweep inputs of the Jacobi sweeps (s3 = -s2, or rank 1) whose U and V are signed permutations turned by 10^e: the
               off-diagonal entries of A^T A fall to 10^e of its diagonal differences, of either sign (the root choice of
               the Jacobi angle, the 'already diagonal' exits)
    Each again scaled by 2^60 and 2^-60 (suffixes _up / _down), and 'degenerate': exactly rank 1, rank 0, diag(1, 1, -1),
    -I, each at the three scales."""
    rs = np.random.RandomState(seed)
    n = per_decade
    fam = {k: [] for k in ('refl_gap', 'rank1', 'small_s3', 'near_rot', 'axis_sweep')}
    dec = []
    for e in DECADES:
        g = 10.0 ** e
        dec.append(np.full(n, e))
        U, V = _rot(rs, n), _rot(rs, n)
        sv = lambda s: U @ (s[:, :, None] * np.swapaxes(V, -1, -2))  # noqa: E731
        s1 = rs.uniform(1, 2, n)
        s2 = s1 * (g + (1 - g) * rs.uniform(0, 1, n))
        fam['refl_gap'].append(sv(np.stack([s1, s2, -(s2 - g * s1)], 1)))
        sign = rs.choice([-1.0, 1.0], n)
        fam['rank1'].append(sv(np.stack([s1, g * s1 * rs.uniform(0.5, 1, n), sign * g * s1 * rs.uniform(0, 0.5, n)], 1)))
        fam['small_s3'].append(sv(np.stack([s1, s1 * rs.uniform(0.3, 0.9, n), sign * g * s1], 1)))
        fam['near_rot'].append(U + g * rs.randn(n, 3, 3))
        U, V = _perm(rs, n) @ exp64(g * rs.randn(n, 3)), _perm(rs, n) @ exp64(g * rs.randn(n, 3))
        s2 = np.where(np.arange(n) % 2 == 0, s1 * rs.uniform(0.3, 0.9, n), 1e-10 * s1)
        fam['axis_sweep'].append(sv(np.stack([s1, s2, -s2], 1)))
    dec = np.concatenate(dec)
    out = {}
    for k, v in fam.items():
        A = _f32(np.concatenate(v))
        for sc, tag in zip(SCALES, ('', '_up', '_down')):
            out[k + tag] = (_f32(A * np.float32(2.0 ** sc)), dec)
    deg = np.stack([np.outer([1.0, 2, 3], [3.0, -1, 2]), np.zeros((3, 3)), np.diag([1.0, 1, -1]), -np.eye(3)])
    deg = np.concatenate([deg * 2.0 ** sc for sc in SCALES])
    out['degenerate'] = (_f32(deg), np.zeros(len(deg), int))
    return out


def proj_figures(A, R):
    """(orthogonality, determinant, optimality deficit, conditioned distance) per matrix, in fp64 on the fp32 input."""
    A64, R64 = np.asarray(A, np.float64), np.asarray(R, np.float64)
    U, s, Vt = np.linalg.svd(A64)
    d = np.sign(np.linalg.det(U @ Vt))
    U = U.copy()
    U[:, :, 2] *= d[:, None]
    Rsvd = U @ Vt
    s1 = np.where(s[:, 0] > 0, s[:, 0], 1.0)
    deficit = (s[:, 0] + s[:, 1] + d * s[:, 2] - np.einsum('nij,nij->n', R64, A64)) / s1
    gap = (s[:, 1] + d * s[:, 2]) / s1
    dist = np.abs(R64 - Rsvd).max((1, 2)) * np.minimum(gap, 1.0)
    orth = np.abs(R64 @ np.swapaxes(R64, -1, -2) - np.eye(3)).max((1, 2))
    det = np.abs(np.linalg.det(R64) - 1)
    return orth, det, deficit, dist


def check_proj_so3(run, label):
    fams = proj_families()
    names = list(fams)
    A = np.concatenate([fams[k][0] for k in names])
    R = run(0, A, None, A.shape)
    assert R.shape == A.shape and np.isfinite(R).all(), label
    orth, det, deficit, dist = proj_figures(A, R)
    fig, pos = {}, 0
    for k in names:
        sl = slice(pos, pos + len(fams[k][0]))
        pos = sl.stop
        fig[k] = dict(orth=float(orth[sl].max()), det=float(det[sl].max()), deficit=float(deficit[sl].max()),
                      dist=float(dist[sl].max()))
        print(f'[proj_so3 {label}] {k:15s} orth {fig[k]["orth"]:.1e} det {fig[k]["det"]:.1e} '
              f'deficit {fig[k]["deficit"]:.2e} dist*gap {fig[k]["dist"]:.2e}')
    for k, f in fig.items():
        assert f['orth'] < PROPER_TOL and f['det'] < PROPER_TOL, (label, k, f)
        assert f['deficit'] <= PROJ_OPT_TOL, (label, k, f)
        assert f['dist'] <= PROJ_DIST_TOL, (label, k, f)
    zero = np.abs(A).max((1, 2)) == 0
    assert zero.sum() == 3 and (R[zero] == np.eye(3, dtype=np.float32)).all()  # rank 0 -> identity, exactly
    return fig


def proj_nonfinite(seed=1):
    """(clean, poisoned, bad_rows): 81 well-conditioned matrices; in ``poisoned`` every third row has a NaN (the first
    nine of them), a +Inf (the next nine) or a -Inf (the last nine) in one of the nine positions, every position covered."""
    rs = np.random.RandomState(seed)
    clean = _f32(_rot(rs, 81) + 0.05 * rs.randn(81, 3, 3))
    bad = clean.copy()
    rows = np.arange(27) * 3 + 1
    for i, r in enumerate(rows):
        bad[r].reshape(9)[i % 9] = (np.nan, np.inf, -np.inf)[i // 9]
    return clean, bad, rows


def check_proj_nonfinite(run, label):
    clean, bad, rows = proj_nonfinite()
    Rc, Rb = run(0, clean, None, clean.shape), run(0, bad, None, bad.shape)
    good = np.setdiff1d(np.arange(len(clean)), rows)
    assert np.isfinite(Rc).all(), label
    assert np.array_equal(Rc[good], Rb[good]), label  # the neighbours of a poisoned row are untouched, bit for bit
    assert np.isnan(Rb[rows]).all(), (label, rows[~np.isnan(Rb[rows]).all((1, 2))])  # never a silent rotation


# ---- the angle grid of mat2rotvec / rotvec2mat ---------------------------------------------------------------------------
def theta_grid():
    """name -> angles (fp64): zero, tiny (10^-30 .. 10^-3), 2 pi / 3 +- k fp32 ulp (the trace of the fp32 matrix crosses
    0 there: branch 0 against the three diagonal branches), pi - 10^-k for k = 1 .. 7, and pi."""
    t0 = np.float32(2 * np.pi / 3)
    ulp = np.spacing(t0)
    ks = np.array([0, 1, 2, 3, 4, 8, 16, 64, 256])
    return dict(
        zero=np.array([0.0]),
        tiny=10.0 ** np.array([-30, -25, -22, -20, -19, -16, -12, -10, -8, -7, -6, -5, -4, -3], float),
        trace0=np.concatenate([t0 + ks * ulp, t0 - ks[1:] * ulp]).astype(np.float64),
        near_pi=np.pi - 10.0 ** -np.arange(1, 8, dtype=float),
        pi=np.array([np.pi]),
    )


def axes(seed=2, n_generic=12):
    """Unit axes: generic; the coordinate axes (exact half turns diag(1, -1, -1), ...); axes whose two largest components
    tie (the r00 > r11 and r11 > r22 comparisons of the log map's branch), all three equal included."""
    rs = np.random.RandomState(seed)
    coord = np.concatenate([np.eye(3), -np.eye(3)])
    ties = np.array([[1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 0.3], [1, 0.3, 1], [0.3, 1, 1], [1, 1, 1], [1, -1, 0.5],
                     [-1, 1, -0.5], [0.5, 1, -1], [-1, -1, -1], [1, -1, 1]], float)
    ties /= np.linalg.norm(ties, axis=-1, keepdims=True)
    return np.concatenate([_unit(rs, n_generic), coord, ties])


def rotvec_grid():
    """name -> rotation vectors (fp64, (n, 3)): every angle class of theta_grid on every axis."""
    ax = axes()
    return {k: (th[:, None, None] * ax[None]).reshape(-1, 3) for k, th in theta_grid().items()}


def _rot_err(rv_out, R):
    return np.abs(exp64(rv_out) - np.asarray(R, np.float64)).max((1, 2))


def check_mat2rotvec(run, label):
    """|exp64(out) - R| <= max(2 x the fp32 oracle's, 1e-6) per angle class, and element-wise agreement with the fp32
    oracle (the same fp32 inputs take the same branch).  |out| <= pi is NOT asserted: the reference's negative-w
    behaviour is reproduced on purpose."""
    fig = {}
    for k, rv in rotvec_grid().items():
        R = _f32(exp64(rv))
        out = run(2, R, None, (len(R), 3))
        ref32 = O.mat2rotvec(R)
        assert np.isfinite(out).all(), (label, k)
        ours, orc = float(_rot_err(out, R).max()), float(_rot_err(ref32, R).max())
        vs = float(np.abs(out - ref32).max())
        fig[k] = dict(ours=ours, oracle32=orc, vs_oracle32=vs)
        print(f'[mat2rotvec {label}] {k:8s} n {len(R):4d} |exp(out) - R| {ours:.2e} (fp32 oracle {orc:.2e}) vs oracle {vs:.2e}')
    for k, f in fig.items():
        assert f['ours'] <= max(2 * f['oracle32'], M2R_FLOOR), (label, k, f)
        assert f['vs_oracle32'] < M2R_ORACLE_TOL, (label, k, f)
    return fig


def rotvec2mat_inputs(seed=3):
    """name -> rotation vectors (float32): the grid of mat2rotvec, angles up to 100 pi, denormal components (alone and
    beside normal ones)."""
    rs = np.random.RandomState(seed)
    out = {k: _f32(v) for k, v in rotvec_grid().items()}
    ax = axes()
    big = np.concatenate([np.pi * np.array([1.5, 2, 3, 7, 10, 31.5, 64, 99.5, 100]), rs.uniform(np.pi, 100 * np.pi, 16)])
    out['large'] = _f32((big[:, None, None] * ax[None]).reshape(-1, 3))
    den = np.array([1e-45, 1e-42, 1e-40, 5e-39])  # below the smallest normal fp32 (1.18e-38)
    d = [s * ax for s in den]
    d += [np.stack([s * ax[:, 0], ax[:, 1] * 1e-20, ax[:, 2]], 1) for s in den]
    d += [np.stack([ax[:, 0] * 1e-3, s * ax[:, 1], s * ax[:, 2]], 1) for s in den]
    out['denormal'] = _f32(np.concatenate(d))
    return out


def check_rotvec2mat(run, label, oracle_only=False):
    """Against fp64 Rodrigues of the fp32 input, and orthogonality: <= 5e-7 (1 + theta) (the rounding of the fp32 angle
    dominates: 6e-8 theta, times the few operations behind it).  The reference arithmetic (O.rotvec2mat in fp32) stays
    under the bound on every class (worst ratio to it: 0.41), so it is not widened anywhere."""
    fig = {}
    for k, rv in rotvec2mat_inputs().items():
        M = O.rotvec2mat(rv) if oracle_only else run(1, rv, None, (len(rv), 3, 3))
        assert np.isfinite(M).all(), (label, k)
        M64 = M.astype(np.float64)
        bound = R2M_TOL * (1 + np.linalg.norm(rv.astype(np.float64), axis=-1))
        err = np.abs(M64 - exp64(rv)).max((1, 2)) / bound
        orth = np.abs(M64 @ np.swapaxes(M64, -1, -2) - np.eye(3)).max((1, 2)) / bound
        fig[k] = dict(err=float(err.max()), orth=float(orth.max()))
        print(f'[rotvec2mat {label}] {k:8s} n {len(rv):4d} err / bound {fig[k]["err"]:.3f} orth / bound {fig[k]["orth"]:.3f}')
    for k, f in fig.items():
        assert f['err'] <= 1 and f['orth'] <= 1, (label, k, f)
    return fig


# ---- align_unit_vectors / swing_twist ----------------------------------------------------------------------------------
def unit_pairs(seed=4, per_decade=PER_DECADE):
    """name -> (a, b) float32 unit vectors at angle 10^-k ('par_k') and pi - 10^-k ('anti_k'), k = 1 .. 7, built in fp64
    and rounded; plus 'same' (identical pairs) and 'opposite' (exactly opposite ones)."""
    rs = np.random.RandomState(seed)
    out = {}
    for k in range(1, 8):
        for tag, ang in (('par', 10.0 ** -k), ('anti', np.pi - 10.0 ** -k)):
            a = _unit(rs, per_decade)
            b = np.cos(ang) * a + np.sin(ang) * _perp(rs, a)
            out[f'{tag}_{k}'] = (_f32(a), _f32(b))
    a = _f32(np.concatenate([_unit(rs, 8), np.eye(3)]))
    out['same'], out['opposite'] = (a, a.copy()), (a, -a)
    return out


def _proper(R):
    R64 = np.asarray(R, np.float64)
    return max(float(np.abs(R64 @ np.swapaxes(R64, -1, -2) - np.eye(3)).max()), float(np.abs(np.linalg.det(R64) - 1).max()))


def check_align(run, label):
    """Finite proper rotations everywhere; |R a - b| <= max(2 x fp32 oracle, 1e-6) per decade for angles no closer than
    1e-3 to pi.  Closer than that the formula is ill-posed in the reference too (the axis is the normalised cross product
    of two nearly opposite fp32 vectors: rounding noise), so the four decades anti_4 .. anti_7 — 4 of the 14 decades — and the
    exactly opposite pairs are held to 'finite proper rotation' only."""
    fig = {}
    for k, (a, b) in unit_pairs().items():
        R = run(3, a, b, (len(a), 3, 3))
        assert np.isfinite(R).all(), (label, k)
        res = lambda M: float(np.abs(np.einsum('nij,nj->ni', M.astype(np.float64), a.astype(np.float64)) - b).max())  # noqa: E731
        fig[k] = dict(proper=_proper(R), ours=res(R), oracle32=res(O.align_unit_vectors(a, b)))
        print(f'[align {label}] {k:7s} proper {fig[k]["proper"]:.1e} |R a - b| {fig[k]["ours"]:.2e} (fp32 oracle {fig[k]["oracle32"]:.2e})')
    gated = 0
    for k, f in fig.items():
        assert f['proper'] < PROPER_TOL, (label, k, f)
        tag, _, dec = k.partition('_')
        if tag in ('par', 'same') or (tag == 'anti' and 10.0 ** -int(dec) >= ANTIPARALLEL_MIN):
            gated += 1
            assert f['ours'] <= max(2 * f['oracle32'], ALIGN_FLOOR), (label, k, f)
    assert gated == 11  # 'same', 7 parallel decades, anti_1 .. anti_3; excluded: exactly anti_4 .. anti_7 and 'opposite'
    return fig


def swing_twist_ref(bref, btgt, A, dtype):
    """The oracle's restatement of the bone part (pt/bodyfitter.py:1389-1412) in ``dtype``."""
    bref, btgt, A = (np.asarray(x, dtype) for x in (bref, btgt, A))
    br = O.divide_no_nan(bref, np.linalg.norm(bref, axis=-1, keepdims=True)).astype(dtype)
    bt = O.divide_no_nan(btgt, np.linalg.norm(btgt, axis=-1, keepdims=True)).astype(dtype)
    Rsw = O.align_unit_vectors(br, bt)
    Hm = Rsw @ np.swapaxes(A, -1, -2)
    trH = Hm[:, 0, 0] + Hm[:, 1, 1] + Hm[:, 2, 2]
    bHb = np.einsum('br,brc,bc->b', bt, Hm, bt)
    vee = np.stack([Hm[:, 1, 2] - Hm[:, 2, 1], Hm[:, 2, 0] - Hm[:, 0, 2], Hm[:, 0, 1] - Hm[:, 1, 0]], -1)
    ang = np.arctan2((bt * vee).sum(-1), trH - bHb)
    return (O.rotvec2mat((bt * ang[:, None]).astype(dtype)) @ Rsw).astype(dtype), ang


def swing_twist_inputs(seed=5):
    """name -> (bref, btgt, A) float32.  The unit pairs above as bones of random length with a generic covariance;
    'twist_k': the covariance of a part turned by +-(pi - 10^-k) about the target bone behind the swing (the twist's
    atan2 at its branch cut); 'zero_ref', 'zero_tgt', 'zero_cov': the divide_no_nan and atan2(0, 0) paths."""
    rs = np.random.RandomState(seed)
    out = {}
    for k, (a, b) in unit_pairs().items():
        n = len(a)
        cov = rs.randn(n, 3, 3) + 2 * np.eye(3)
        out[k] = (_f32(a * rs.uniform(0.05, 0.5, (n, 1))), _f32(b * rs.uniform(0.05, 0.5, (n, 1))), _f32(cov))
    n = PER_DECADE
    for k in range(1, 8):
        a, b = _unit(rs, n), _unit(rs, n)
        Rsw = O.align_unit_vectors(a, b)
        phi = rs.choice([-1.0, 1.0], n) * (np.pi - 10.0 ** -k)
        cov = exp64(b * phi[:, None]) @ Rsw * rs.uniform(0.5, 2, (n, 1, 1))
        out[f'twist_{k}'] = (_f32(a * 0.3), _f32(b * 0.3), _f32(cov))
    a, b, cov = _f32(_unit(rs, n) * 0.3), _f32(_unit(rs, n) * 0.3), _f32(rs.randn(n, 3, 3) + 2 * np.eye(3))
    out['zero_ref'] = (0 * a, b, cov)
    out['zero_tgt'] = (a, 0 * b, cov)
    out['zero_cov'] = (a, b, 0 * cov)
    return out


def check_swing_twist(run, label):
    """Rotation matrices (continuous across twist = +-pi) against the fp64 restatement: <= max(2 x the fp32 restatement's
    distance, 5e-6) per class, no class excluded (near antiparallel bones the fp32 restatement's own distance is large
    and sets the gate)."""
    fig = {}
    for k, (br, bt, A) in swing_twist_inputs().items():
        R = run(4, br, np.concatenate([bt, A.reshape(-1, 9)], 1), (len(br), 3, 3))
        assert np.isfinite(R).all(), (label, k)
        ref64, _ = swing_twist_ref(br, bt, A, np.float64)
        ref32, _ = swing_twist_ref(br, bt, A, np.float32)
        fig[k] = dict(proper=_proper(R), ours=float(np.abs(R - ref64).max()), oracle32=float(np.abs(ref32 - ref64).max()))
        print(f'[swing_twist {label}] {k:8s} proper {fig[k]["proper"]:.1e} |R - R64| {fig[k]["ours"]:.2e} (fp32 restatement {fig[k]["oracle32"]:.2e})')
    for k, f in fig.items():
        assert f['proper'] < PROPER_TOL, (label, k, f)
        assert f['ours'] <= max(2 * f['oracle32'], SWING_FLOOR), (label, k, f)
    return fig
