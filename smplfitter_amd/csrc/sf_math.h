// Small fixed-size math shared by the HIP kernels (device) and the host unit-test build:
// 3x3 helpers, the SO(3) projection, swing / Rodrigues / log map, with the reference's branch
// structure (reference src/smplfitter/pt/rotation.py).  All matrices are row-major float[9].
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SF_HD __host__ __device__ __forceinline__
// partial unrolling of loops with run-time trip counts whose bodies are LDS / table reads: the reads of
// several iterations are then issued together instead of one memory latency per iteration (the
// accumulation order is unchanged)
#define SF_UNROLL(n) _Pragma(SF_STR_(unroll n))
#define SF_UNROLL_FULL _Pragma("unroll")
#define SF_STR_(x) #x
#else
#define SF_HD inline
#define SF_UNROLL(n)
#define SF_UNROLL_FULL
#endif

// Scheduling fence for the device compiler: stops it from hoisting the LDS loads of later phases
// above earlier ones (which explodes register pressure in the per-vertex bodies). No-op on host.
#if defined(__HIP_DEVICE_COMPILE__)
#define SF_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define SF_SCHED_FENCE() ((void)0)
#endif

namespace sf {

// The sum of n doubles `stride` apart, in the one order every share_beta sum uses (k_share_partial / k_share_reduce and
// their host emulation): eight interleaved accumulators (eight loads in flight on the device), the first n / 8 * 8
// elements dealt to them in turn, the tail to the first n % 8, then a fixed tree over the eight.
SF_HD double sum_rows_f64(const double* __restrict__ p, int n, size_t stride) {
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    SF_UNROLL_FULL
    for (int u = 0; u < 8; ++u) a[u] += p[(size_t)(i + u) * stride];
  }
  for (int u = 0; i < n; ++i, ++u) a[u] += p[(size_t)i * stride];
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

#if defined(__HIPCC__)
// Error-free split of an fp32 into three bf16 terms x = h + m + l (3 x 8 mantissa bits), the operand form of the
// split-bf16 posedirs GEMMs.  Stated once: whoever produces feature planes (the GEMM's own front end,
// k_split_features, k_prologue_bm) gets the same bits.
struct Bf16x3 {
  __bf16 h, m, l;
};
SF_HD Bf16x3 split_bf16x3(float x) {
  const __bf16 h = (__bf16)x;
  const float r1 = x - (float)h;
  const __bf16 m = (__bf16)r1;
  const __bf16 l = (__bf16)(r1 - (float)m);
  return {h, m, l};
}
#endif

// a / b, 0 where b == 0 (rotation.py:8-11)
SF_HD float divide_no_nan(float a, float b) { return b == 0.f ? 0.f : a / b; }

SF_HD void m3_mul(const float* a, const float* b, float* o) {  // o = a b
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      o[r * 3 + c] = a[r * 3 + 0] * b[0 * 3 + c] + a[r * 3 + 1] * b[1 * 3 + c] +
                     a[r * 3 + 2] * b[2 * 3 + c];
}
SF_HD void m3_tmul(const float* a, const float* b, float* o) {  // o = a^T b
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      o[r * 3 + c] = a[0 * 3 + r] * b[0 * 3 + c] + a[1 * 3 + r] * b[1 * 3 + c] +
                     a[2 * 3 + r] * b[2 * 3 + c];
}
SF_HD void m3_mult(const float* a, const float* b, float* o) {  // o = a b^T
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      o[r * 3 + c] = a[r * 3 + 0] * b[c * 3 + 0] + a[r * 3 + 1] * b[c * 3 + 1] +
                     a[r * 3 + 2] * b[c * 3 + 2];
}
SF_HD void m3_vec(const float* a, const float* v, float* o) {  // o = a v
  for (int r = 0; r < 3; ++r) o[r] = a[r * 3] * v[0] + a[r * 3 + 1] * v[1] + a[r * 3 + 2] * v[2];
}
SF_HD void m3_identity(float* o) {
  for (int k = 0; k < 9; ++k) o[k] = (k % 4 == 0) ? 1.f : 0.f;
}

// Centered cross-covariance from uncentered part sums about centres (ct, ca):
//   raw - st ca^T - ct sa^T + sw (ct ca^T)          (bodyfitter.py:1354-1359, :1512-1518)
SF_HD void centered_cov(const float* raw, const float* st, const float* sa, float sw,
                        const float* ct, const float* ca, float* A) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      A[r * 3 + c] = raw[r * 3 + c] - st[r] * ca[c] - ct[r] * sa[c] + sw * (ct[r] * ca[c]);
}

// 1/sqrt(x) and 1/x in fp64 from the hardware seed + one Newton step on the device (the IEEE
// sqrt / divide sequences cost ~20 dependent fp64 instructions each and dominate the latency of the
// joint-level kernels); plain libm on the host.  Accurate to ~1e-14, far below the fp32 output.
SF_HD double fast_rsqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  double y = __builtin_amdgcn_rsq(x);
  y = y * (1.5 - 0.5 * x * y * y);
  return y * (1.5 - 0.5 * x * y * y);
#else
  return 1.0 / sqrt(x);
#endif
}
SF_HD double fast_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r = __builtin_amdgcn_rcp(x);
  r = r * (2.0 - x * r);
  return r * (2.0 - x * r);
#else
  return 1.0 / x;
#endif
}

// Nearest rotation in Frobenius norm: R = U diag(1,1,det(UV^T)) V^T of the SVD A = U S V^T
// (rotation.py:100-110 computes it with a library SVD + reflection fix; rotation.py:26-97 is the reference's own
// closed form).  Here, in fp64: the closed form through Horn's quaternion eigenproblem (below), and — for the inputs
// whose nearest rotation is not unique — cyclic Jacobi on the symmetric M = A^T A gives V and the singular-value order; U's first two
// columns are A v1, A v2 (Gram-Schmidt), and taking u3 = u1 x u2, v3 = v1 x v2 keeps both frames
// right-handed, which IS the reflection fix (R = u1 v1^T + u2 v2^T + u3 v3^T has det +1).
// Degenerate inputs: A ~ 0 -> identity; rank 1 -> an arbitrary completion (as any SVD would give).
SF_HD void proj_so3(const float* Af, float* R) {
  double a[9];
  double fro2 = 0.0;
  for (int k = 0; k < 9; ++k) {
    a[k] = (double)Af[k];
    fro2 += a[k] * a[k];
  }
  if (!(fro2 > 1e-60)) {  // also catches NaN
    if (fro2 == fro2) {
      m3_identity(R);
    } else {
      for (int k = 0; k < 9; ++k) R[k] = Af[k] * 0.f + (float)fro2;  // propagate NaN
    }
    return;
  }
  const double inv = fast_rsqrt(fro2);
  for (int k = 0; k < 9; ++k) a[k] *= inv;
  // M = A^T A (symmetric): m00 m01 m02 m11 m12 m22
  double m00 = a[0] * a[0] + a[3] * a[3] + a[6] * a[6];
  double m01 = a[0] * a[1] + a[3] * a[4] + a[6] * a[7];
  double m02 = a[0] * a[2] + a[3] * a[5] + a[6] * a[8];
  double m11 = a[1] * a[1] + a[4] * a[4] + a[7] * a[7];
  double m12 = a[1] * a[2] + a[4] * a[5] + a[7] * a[8];
  double m22 = a[2] * a[2] + a[5] * a[5] + a[8] * a[8];
#ifndef SMPLFIT_PROJ_JACOBI_ONLY
  // ---- closed form (round 6; the north star's "closed-form 3x3 SVD").  The nearest rotation is the rotation of the
  // unit quaternion q that maximises q^T N q, N = Horn's symmetric 4 x 4 matrix of A (Horn 1987; with A = sum t a^T,
  // rows = target, Horn's S is A^T).  Its eigenvalues are the signed sums of the singular values, largest
  // lambda = s1 + s2 + sgn(det A) s3 — the reflection case needs no fix-up: q always is a proper rotation — and the
  // characteristic polynomial of the trace-free N needs three invariants of the normalised A only:
  //   P(x) = x^4 - 2 |A|_F^2 x^2 - 8 det(A) x + (2 tr((A^T A)^2) - |A|_F^4),      |A|_F = 1 here.
  // lambda: Newton from the upper bound sqrt(3) (P is convex and increasing above its largest root: monotone
  // convergence, 4 steps for the near-rotations of a fit, <= 12 for ill-conditioned inputs); q: a column of
  // adj(N - lambda I) = P'(lambda) q q^T, the one with the largest diagonal entry.  ~330 fp64 operations without a
  // data-dependent sweep count, against ~600 for the Jacobi sweeps below, which stay for the inputs whose largest
  // eigenvalue is (nearly) double — rank 1, or s2 ~ s3 under a reflection: the nearest rotation is not unique there and
  // the cofactors vanish — detected by |tr adj| = |P'(lambda)| = the product of the gaps to the other eigenvalues.
  {
    const double trm2 = (m00 * m00 + m11 * m11 + m22 * m22) + 2.0 * (m01 * m01 + m02 * m02 + m12 * m12);
    const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
    const double c1 = -8.0 * det, c0 = 2.0 * trm2 - 1.0;
    double lam = 1.7320508075688772;
    bool conv = false;
    for (int it = 0; it < 12; ++it) {
      const double l2 = lam * lam;
      const double P = (l2 * l2 - 2.0 * l2) + (c1 * lam + c0), dP = 4.0 * (l2 * lam - lam) + c1;
      if (!(dP > 1e-6)) break;  // (a multiple root at the top: the sweeps below)
      const double d = P * fast_rcp(dP);
      lam -= d;
      if (fabs(d) <= 1e-11 * lam) {  // (quadratic convergence: the step after this one would be below 1e-16)
        conv = true;
        break;
      }
    }
    if (conv) {
      // K = N - lambda I (symmetric), S = A^T:  S_xy = a[3 y + x]
      const double sxx = a[0], sxy = a[3], sxz = a[6], syx = a[1], syy = a[4], syz = a[7], szx = a[2], szy = a[5], szz = a[8];
      const double k00 = (sxx + syy + szz) - lam, k01 = syz - szy, k02 = szx - sxz, k03 = sxy - syx;
      const double k11 = (sxx - syy - szz) - lam, k12 = sxy + syx, k13 = szx + sxz;
      const double k22 = (-sxx + syy - szz) - lam, k23 = syz + szy;
      const double k33 = (-sxx - syy + szz) - lam;
      // adjugate through the 2 x 2 minors of the row pairs (0, 1) and (2, 3)
      const double s0 = k00 * k11 - k01 * k01, s1 = k00 * k12 - k01 * k02, s2 = k00 * k13 - k01 * k03;
      const double s3 = k01 * k12 - k11 * k02, s4 = k01 * k13 - k11 * k03, s5 = k02 * k13 - k12 * k03;
      const double d5 = k22 * k33 - k23 * k23, d4 = k12 * k33 - k13 * k23, d3 = k12 * k23 - k13 * k22;
      const double d2 = k02 * k33 - k03 * k23, d1 = k02 * k23 - k03 * k22;
      const double a00 = k11 * d5 - k12 * d4 + k13 * d3, a01 = -k01 * d5 + k02 * d4 - k03 * d3;
      const double a02 = k13 * s5 - k23 * s4 + k33 * s3, a03 = -k12 * s5 + k22 * s4 - k23 * s3;
      const double a11 = k00 * d5 - k02 * d2 + k03 * d1, a12 = -k03 * s5 + k23 * s2 - k33 * s1;
      const double a13 = k02 * s5 - k22 * s2 + k23 * s1, a22 = k03 * s4 - k13 * s2 + k33 * s0;
      const double a23 = -k02 * s4 + k12 * s2 - k23 * s0, a33 = k02 * s3 - k12 * s1 + k22 * s0;
      // (the diagonal entries share the sign of P'(lambda); gaps: a well-separated largest eigenvalue)
      const double tra = fabs((a00 + a11) + (a22 + a33));
      if (tra > 1e-4) {
        double q0 = a00, q1 = a01, q2 = a02, q3 = a03, best = fabs(a00);
        if (fabs(a11) > best) { best = fabs(a11); q0 = a01; q1 = a11; q2 = a12; q3 = a13; }
        if (fabs(a22) > best) { best = fabs(a22); q0 = a02; q1 = a12; q2 = a22; q3 = a23; }
        if (fabs(a33) > best) { best = fabs(a33); q0 = a03; q1 = a13; q2 = a23; q3 = a33; }
        const double qn = fast_rsqrt((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
        const double w = q0 * qn, x = q1 * qn, y = q2 * qn, z = q3 * qn;
        R[0] = (float)(1.0 - 2.0 * (y * y + z * z));
        R[1] = (float)(2.0 * (x * y - w * z));
        R[2] = (float)(2.0 * (x * z + w * y));
        R[3] = (float)(2.0 * (x * y + w * z));
        R[4] = (float)(1.0 - 2.0 * (x * x + z * z));
        R[5] = (float)(2.0 * (y * z - w * x));
        R[6] = (float)(2.0 * (x * z - w * y));
        R[7] = (float)(2.0 * (y * z + w * x));
        R[8] = (float)(1.0 - 2.0 * (x * x + y * y));
        return;
      }
    }
  }
#endif
  // eigenvectors as columns of V (v[r][c])
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
#define SF_JACOBI(app, aqq, apq, arp, arq, vp0, vq0, vp1, vq1, vp2, vq2)                   \
  if (fabs(apq) > 1e-140) {                                                                \
    /* tan of the Jacobi angle: t = e / (d + sgn(d) sqrt(d^2 + e^2)), d = aqq-app, e = 2 apq */ \
    const double dd = aqq - app, ee = 2.0 * apq;                                           \
    const double hh = dd * dd + ee * ee;                                                   \
    const double rt = hh * fast_rsqrt(hh);                                                 \
    const double tt = ee * fast_rcp(dd >= 0.0 ? dd + rt : dd - rt);                        \
    const double cc = fast_rsqrt(tt * tt + 1.0), ss = tt * cc;                             \
    app -= tt * apq;                                                                       \
    aqq += tt * apq;                                                                       \
    apq = 0.0;                                                                             \
    const double rp = arp, rq = arq;                                                       \
    arp = cc * rp - ss * rq;                                                               \
    arq = ss * rp + cc * rq;                                                               \
    double x, y;                                                                           \
    x = vp0; y = vq0; vp0 = cc * x - ss * y; vq0 = ss * x + cc * y;                        \
    x = vp1; y = vq1; vp1 = cc * x - ss * y; vq1 = ss * x + cc * y;                        \
    x = vp2; y = vq2; vp2 = cc * x - ss * y; vq2 = ss * x + cc * y;                        \
  }
  for (int sweep = 0; sweep < 8; ++sweep) {
    const double off = m01 * m01 + m02 * m02 + m12 * m12;
    if (off < 1e-34) break;  // trace(M) == 1 after normalisation: relative threshold
    SF_JACOBI(m00, m11, m01, m02, m12, v00, v01, v10, v11, v20, v21)  // (p,q)=(0,1), r=2
    SF_JACOBI(m00, m22, m02, m01, m12, v00, v02, v10, v12, v20, v22)  // (0,2), r=1
    SF_JACOBI(m11, m22, m12, m01, m02, v01, v02, v11, v12, v21, v22)  // (1,2), r=0
  }
#undef SF_JACOBI
  // pick the two largest eigenvalues (order: e1 >= e2 >= e3)
  double e[3] = {m00, m11, m22};
  double vc[3][3] = {{v00, v10, v20}, {v01, v11, v21}, {v02, v12, v22}};  // vc[k] = k-th eigvec
  int i1 = 0, i3 = 0;
  for (int k = 1; k < 3; ++k) {
    if (e[k] > e[i1]) i1 = k;
    if (e[k] <= e[i3]) i3 = k;
  }
  if (i1 == i3) {  // all equal
    i1 = 0;
    i3 = 2;
  }
  const int i2 = 3 - i1 - i3;
  const double* v1 = vc[i1];
  const double* v2 = vc[i2];
  const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2],
                        v1[0] * v2[1] - v1[1] * v2[0]};
  double u1[3], u2[3], u3[3];
  for (int r = 0; r < 3; ++r) {
    u1[r] = a[r * 3] * v1[0] + a[r * 3 + 1] * v1[1] + a[r * 3 + 2] * v1[2];
    u2[r] = a[r * 3] * v2[0] + a[r * 3 + 1] * v2[1] + a[r * 3 + 2] * v2[2];
  }
  const double i1n = fast_rsqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);  // sigma1 >= 1/sqrt(3)
  for (int r = 0; r < 3; ++r) u1[r] *= i1n;
  const double d12 = u2[0] * u1[0] + u2[1] * u1[1] + u2[2] * u1[2];
  for (int r = 0; r < 3; ++r) u2[r] -= d12 * u1[r];
  double n2 = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];
  if (n2 > 1e-28) {
    const double i2n = fast_rsqrt(n2);
    for (int r = 0; r < 3; ++r) u2[r] *= i2n;
  } else {  // rank 1: any unit vector orthogonal to u1
    int k = 0;
    if (fabs(u1[1]) < fabs(u1[k])) k = 1;
    if (fabs(u1[2]) < fabs(u1[k])) k = 2;
    double ek[3] = {0, 0, 0};
    ek[k] = 1.0;
    u2[0] = u1[1] * ek[2] - u1[2] * ek[1];
    u2[1] = u1[2] * ek[0] - u1[0] * ek[2];
    u2[2] = u1[0] * ek[1] - u1[1] * ek[0];
    n2 = fast_rsqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    for (int r = 0; r < 3; ++r) u2[r] *= n2;
  }
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      R[r * 3 + c] = (float)(u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c]);
}

// Rodrigues with the reference's element arithmetic (rotation.py:236-258).
SF_HD void rotvec2mat(const float* rv, float* m) {
  const float angle = sqrtf(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
  const float ax = divide_no_nan(rv[0], angle), ay = divide_no_nan(rv[1], angle),
              az = divide_no_nan(rv[2], angle);
  const float sn = sinf(angle), cs = cosf(angle);
  const float sx = sn * ax, sy = sn * ay, sz = sn * az;
  const float c1 = 1.0f - cs;
  const float c1x = c1 * ax, c1y = c1 * ay, c1z = c1 * az;
  float tmp = c1x * ay;
  m[1] = tmp - sz;
  m[3] = tmp + sz;
  tmp = c1x * az;
  m[2] = tmp + sy;
  m[6] = tmp - sy;
  tmp = c1y * az;
  m[5] = tmp - sx;
  m[7] = tmp + sx;
  m[0] = c1x * ax + cs;
  m[4] = c1y * ay + cs;
  m[8] = c1z * az + cs;
}

// Rotation taking unit a to unit b; zero rotvec (identity) when parallel or exactly antiparallel
// (rotation.py:210-224).
SF_HD void align_unit_vectors(const float* a, const float* b, float* m) {
  const float cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2],
              cz = a[0] * b[1] - a[1] * b[0];
  const float dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const float sn = sqrtf(cx * cx + cy * cy + cz * cz);
  const float ang = atan2f(sn, dot);
  const float rv[3] = {divide_no_nan(cx * ang, sn), divide_no_nan(cy * ang, sn),
                       divide_no_nan(cz * ang, sn)};
  rotvec2mat(rv, m);
}

// Log map with the reference's 4-way quaternion branch; w may be negative (rotvec norm > pi),
// reproduced as is (rotation.py:261-289).
SF_HD void mat2rotvec(const float* r, float* rv) {
  const float r00 = r[0], r01 = r[1], r02 = r[2], r10 = r[3], r11 = r[4], r12 = r[5], r20 = r[6],
              r21 = r[7], r22 = r[8];
  const float trace = r00 + r11 + r22;
  float x, y, z, w;
  if (trace > 0.f) {
    x = r21 - r12; y = r02 - r20; z = r10 - r01; w = 1.0f + trace;
  } else if (r00 > r11 && r00 > r22) {
    x = (1.0f - r22) + (r00 - r11); y = r10 + r01; z = r02 + r20; w = r21 - r12;
  } else if (r11 > r22) {
    x = r10 + r01; y = (1.0f - r22) - (r00 - r11); z = r21 + r12; w = r02 - r20;
  } else {
    x = r02 + r20; y = r21 + r12; z = (1.0f + r22) - (r00 + r11); w = r10 - r01;
  }
  const float n = sqrtf(x * x + y * y + z * z);
  const float f = divide_no_nan(2.0f, n) * atan2f(n, w);
  rv[0] = f * x;
  rv[1] = f * y;
  rv[2] = f * z;
}

// Bone part: swing aligns the reference bone with the target bone, twist about the target bone is
// recovered in closed form from the part's centred cross-covariance A (bodyfitter.py:1389-1412).
SF_HD void swing_twist(const float* b_ref, const float* b_tgt, const float* A, float* R) {
  const float nr = sqrtf(b_ref[0] * b_ref[0] + b_ref[1] * b_ref[1] + b_ref[2] * b_ref[2]);
  const float nt = sqrtf(b_tgt[0] * b_tgt[0] + b_tgt[1] * b_tgt[1] + b_tgt[2] * b_tgt[2]);
  const float br[3] = {divide_no_nan(b_ref[0], nr), divide_no_nan(b_ref[1], nr),
                       divide_no_nan(b_ref[2], nr)};
  const float bt[3] = {divide_no_nan(b_tgt[0], nt), divide_no_nan(b_tgt[1], nt),
                       divide_no_nan(b_tgt[2], nt)};
  float Rsw[9], H[9];
  align_unit_vectors(br, bt, Rsw);
  m3_mult(Rsw, A, H);  // H = R_swing A^T
  const float trH = H[0] + H[4] + H[8];
  float Hb[3];
  m3_vec(H, bt, Hb);
  const float bHb = bt[0] * Hb[0] + bt[1] * Hb[1] + bt[2] * Hb[2];
  const float vee[3] = {H[5] - H[7], H[6] - H[2], H[1] - H[3]};
  const float ang = atan2f(bt[0] * vee[0] + bt[1] * vee[1] + bt[2] * vee[2], trH - bHb);
  const float rv[3] = {bt[0] * ang, bt[1] * ang, bt[2] * ang};
  float Rtw[9];
  rotvec2mat(rv, Rtw);
  m3_mul(Rtw, Rsw, R);
}

// ---------------------------------------------------------------------------------------------
// Adjoints of the rotation primitives above (smplfit_fit_backward_f32).  All 3x3 algebra in fp64, on
// the fp32 values the forward read; cotangents are row-major like their matrices.
// ---------------------------------------------------------------------------------------------
SF_HD void d3_mul(const double* a, const double* b, double* o) {  // o = a b
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r * 3] * b[c] + a[r * 3 + 1] * b[3 + c] + a[r * 3 + 2] * b[6 + c];
}
SF_HD void d3_tmul(const double* a, const double* b, double* o) {  // o = a^T b
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r] * b[c] + a[3 + r] * b[3 + c] + a[6 + r] * b[6 + c];
}
SF_HD void d3_mult(const double* a, const double* b, double* o) {  // o = a b^T
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r * 3] * b[c * 3] + a[r * 3 + 1] * b[c * 3 + 1] + a[r * 3 + 2] * b[c * 3 + 2];
}

// Adjoint of R = proj_so3(A): with S = R^T A (symmetric; indefinite in the reflection case) solve
// (tr(S) I - S) w = vee(R^T Rbar - Rbar^T R), vee(K) = (K21, K02, K10); Abar = R hat(w).  No SVD; singular exactly
// where the projection is (sigma2 + d sigma3 = 0): the division then gives inf / NaN for that matrix only.
SF_HD void proj_so3_adjoint(const double* A, const double* R, const double* Rbar, double* Abar) {
  double S[9], K[9];
  d3_tmul(R, A, S);
  d3_tmul(R, Rbar, K);
  const double v[3] = {K[7] - K[5], K[2] - K[6], K[3] - K[1]};
  // symmetrised: R is the fp32 rounding of the projection
  const double s01 = 0.5 * (S[1] + S[3]), s02 = 0.5 * (S[2] + S[6]), s12 = 0.5 * (S[5] + S[7]);
  const double tr = S[0] + S[4] + S[8];
  const double m00 = tr - S[0], m11 = tr - S[4], m22 = tr - S[8], m01 = -s01, m02 = -s02, m12 = -s12;
  // symmetric 3x3 solve by the adjugate
  const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
  const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
  const double det = m00 * c00 + m01 * c01 + m02 * c02;
  const double id = 1.0 / det;
  const double w0 = (c00 * v[0] + c01 * v[1] + c02 * v[2]) * id;
  const double w1 = (c01 * v[0] + c11 * v[1] + c12 * v[2]) * id;
  const double w2 = (c02 * v[0] + c12 * v[1] + c22 * v[2]) * id;
  const double H[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
  d3_mul(R, H, Abar);
}

// Adjoint of centered_cov.  The covariance is A = sum_i w_i (t_i - ct)(a_i - ca)^T, so with the cotangent Abar the
// cotangents of the part sums are Rawbar = Abar, stbar = -Abar ca, sabar = -Abar^T ct, swbar = ct^T Abar ca.  The vertex
// pass applies them in the factored form (partsum_vertex_adjoint), which does not cancel: the record it reads is
// [Abar 9 | ct 3 | ca 3 | 0] (part_cotangent).  The cotangents of the centres: -Abar (sa - sw ca), -Abar^T (st - sw ct).
SF_HD void part_cotangent(const double* Abar, const double* ct, const double* ca, float* rec) {
  for (int k = 0; k < 9; ++k) rec[k] = (float)Abar[k];
  for (int c = 0; c < 3; ++c) {
    rec[9 + c] = (float)ct[c];
    rec[12 + c] = (float)ca[c];
  }
  rec[15] = 0.f;
}
SF_HD void centered_cov_centres_adjoint(const double* Abar, const double* ps, const double* ct, const double* ca,
                                        double* ctbar, double* cabar) {
  const double sw = ps[15];
  for (int r = 0; r < 3; ++r) {
    ctbar[r] = cabar[r] = 0.0;
    for (int c = 0; c < 3; ++c) {
      ctbar[r] -= Abar[r * 3 + c] * (ps[12 + c] - sw * ca[c]);
      cabar[r] -= Abar[c * 3 + r] * (ps[9 + c] - sw * ct[c]);
    }
  }
}

// Rodrigues R = cos I + sin hat(a) + (1 - cos) a a^T of r = theta a, in fp64, and its vector-Jacobian product with the
// reference's convention at r = 0 (axis = 0 there: the gradient is 0, pt/_autograd.py _div0).
SF_HD void rodrigues_d(const double* r, double* R) {
  const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  const double a[3] = {th == 0.0 ? 0.0 : r[0] / th, th == 0.0 ? 0.0 : r[1] / th, th == 0.0 ? 0.0 : r[2] / th};
  const double sn = sin(th), cs = cos(th), c1 = 1.0 - cs;
  R[0] = c1 * a[0] * a[0] + cs; R[1] = c1 * a[0] * a[1] - sn * a[2]; R[2] = c1 * a[0] * a[2] + sn * a[1];
  R[3] = c1 * a[0] * a[1] + sn * a[2]; R[4] = c1 * a[1] * a[1] + cs; R[5] = c1 * a[1] * a[2] - sn * a[0];
  R[6] = c1 * a[0] * a[2] - sn * a[1]; R[7] = c1 * a[1] * a[2] + sn * a[0]; R[8] = c1 * a[2] * a[2] + cs;
}
SF_HD void rodrigues_vjp_d(const double* r, const double* Rb, double* rbar) {
  const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (th == 0.0) {
    rbar[0] = rbar[1] = rbar[2] = 0.0;
    return;
  }
  const double a[3] = {r[0] / th, r[1] / th, r[2] / th};
  const double sn = sin(th), cs = cos(th);
  const double vv[3] = {Rb[7] - Rb[5], Rb[2] - Rb[6], Rb[3] - Rb[1]};
  double Ra[3], Rta[3];
  for (int i = 0; i < 3; ++i) {
    Ra[i] = Rb[i * 3] * a[0] + Rb[i * 3 + 1] * a[1] + Rb[i * 3 + 2] * a[2];
    Rta[i] = Rb[i] * a[0] + Rb[3 + i] * a[1] + Rb[6 + i] * a[2];
  }
  const double aRa = a[0] * Ra[0] + a[1] * Ra[1] + a[2] * Ra[2], tr = Rb[0] + Rb[4] + Rb[8];
  const double avv = a[0] * vv[0] + a[1] * vv[1] + a[2] * vv[2];
  const double thbar = -sn * tr + cs * avv + sn * aRa;
  double abar[3], ad = 0.0;
  for (int i = 0; i < 3; ++i) {
    abar[i] = sn * vv[i] + (1.0 - cs) * (Ra[i] + Rta[i]);
    ad += a[i] * abar[i];
  }
  for (int i = 0; i < 3; ++i) rbar[i] = thbar * a[i] + (abar[i] - a[i] * ad) / th;
}

// Adjoint of the normalisation b = v / |v| (0 where |v| == 0, with a zero gradient there): vbar += ...
SF_HD void normalize_adjoint_add(const double* v, const double* bbar, double* vbar) {
  const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (n == 0.0) return;
  const double b[3] = {v[0] / n, v[1] / n, v[2] / n};
  const double d = b[0] * bbar[0] + b[1] * bbar[1] + b[2] * bbar[2];
  for (int c = 0; c < 3; ++c) vbar[c] += (bbar[c] - b[c] * d) / n;
}

// Adjoint of swing_twist: from the cotangent Rbar of the part rotation those of the centred covariance A and of the two
// (unnormalised) bones.  The forward is re-evaluated in fp64.
SF_HD void swing_twist_adjoint(const double* b_ref, const double* b_tgt, const double* A, const double* Rbar, double* Abar,
                               double* brefbar, double* btgtbar) {
  const double nr = sqrt(b_ref[0] * b_ref[0] + b_ref[1] * b_ref[1] + b_ref[2] * b_ref[2]);
  const double nt = sqrt(b_tgt[0] * b_tgt[0] + b_tgt[1] * b_tgt[1] + b_tgt[2] * b_tgt[2]);
  double br[3], bt[3];
  for (int c = 0; c < 3; ++c) {
    br[c] = nr == 0.0 ? 0.0 : b_ref[c] / nr;
    bt[c] = nt == 0.0 ? 0.0 : b_tgt[c] / nt;
  }
  // swing
  const double cr[3] = {br[1] * bt[2] - br[2] * bt[1], br[2] * bt[0] - br[0] * bt[2], br[0] * bt[1] - br[1] * bt[0]};
  const double dot = br[0] * bt[0] + br[1] * bt[1] + br[2] * bt[2];
  const double sn = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
  const double ang = atan2(sn, dot);
  const double f = sn == 0.0 ? 0.0 : ang / sn;
  const double rv[3] = {cr[0] * f, cr[1] * f, cr[2] * f};
  double Rsw[9], H[9];
  rodrigues_d(rv, Rsw);
  d3_mult(Rsw, A, H);  // H = R_swing A^T
  const double trH = H[0] + H[4] + H[8];
  double Hb[3], Htb[3];
  for (int i = 0; i < 3; ++i) {
    Hb[i] = H[i * 3] * bt[0] + H[i * 3 + 1] * bt[1] + H[i * 3 + 2] * bt[2];
    Htb[i] = H[i] * bt[0] + H[3 + i] * bt[1] + H[6 + i] * bt[2];
  }
  const double bHb = bt[0] * Hb[0] + bt[1] * Hb[1] + bt[2] * Hb[2];
  const double vee[3] = {H[5] - H[7], H[6] - H[2], H[1] - H[3]};
  const double y = bt[0] * vee[0] + bt[1] * vee[1] + bt[2] * vee[2], x = trH - bHb;
  const double ang2 = atan2(y, x);
  const double rv2[3] = {bt[0] * ang2, bt[1] * ang2, bt[2] * ang2};
  double Rtw[9];
  rodrigues_d(rv2, Rtw);
  // reverse: R = Rtw Rsw
  double Rtwbar[9], Rswbar[9], rv2bar[3];
  d3_mult(Rbar, Rsw, Rtwbar);
  d3_tmul(Rtw, Rbar, Rswbar);
  rodrigues_vjp_d(rv2, Rtwbar, rv2bar);
  double btbar[3], brbar[3] = {0.0, 0.0, 0.0};
  double ang2bar = 0.0;
  for (int c = 0; c < 3; ++c) {
    btbar[c] = rv2bar[c] * ang2;
    ang2bar += rv2bar[c] * bt[c];
  }
  const double q = x * x + y * y;
  const double ybar = q == 0.0 ? 0.0 : ang2bar * x / q, xbar = q == 0.0 ? 0.0 : -ang2bar * y / q;
  double Hbar[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Hbar[r * 3 + c] = (r == c ? xbar : 0.0) - xbar * bt[r] * bt[c];
  Hbar[5] += ybar * bt[0]; Hbar[7] -= ybar * bt[0];
  Hbar[6] += ybar * bt[1]; Hbar[2] -= ybar * bt[1];
  Hbar[1] += ybar * bt[2]; Hbar[3] -= ybar * bt[2];
  for (int c = 0; c < 3; ++c) btbar[c] += ybar * vee[c] - xbar * (Hb[c] + Htb[c]);
  // H = Rsw A^T
  double HA[9];
  d3_mul(Hbar, A, HA);
  for (int k = 0; k < 9; ++k) Rswbar[k] += HA[k];
  d3_tmul(Hbar, Rsw, Abar);  // Abar = Hbar^T Rsw
  // swing: Rsw = rodrigues(cr * ang / sn)
  if (sn != 0.0) {
    double rvbar[3], crbar[3];
    rodrigues_vjp_d(rv, Rswbar, rvbar);
    double fbar = 0.0;
    for (int c = 0; c < 3; ++c) {
      crbar[c] = rvbar[c] * f;
      fbar += rvbar[c] * cr[c];
    }
    const double angbar = fbar / sn;
    double snbar = -fbar * ang / (sn * sn);
    const double q2 = sn * sn + dot * dot;
    snbar += angbar * dot / q2;
    const double dotbar = -angbar * sn / q2;
    for (int c = 0; c < 3; ++c) crbar[c] += snbar * cr[c] / sn;
    // cr = br x bt
    brbar[0] += bt[1] * crbar[2] - bt[2] * crbar[1];
    brbar[1] += bt[2] * crbar[0] - bt[0] * crbar[2];
    brbar[2] += bt[0] * crbar[1] - bt[1] * crbar[0];
    btbar[0] += crbar[1] * br[2] - crbar[2] * br[1];
    btbar[1] += crbar[2] * br[0] - crbar[0] * br[2];
    btbar[2] += crbar[0] * br[1] - crbar[1] * br[0];
    for (int c = 0; c < 3; ++c) {
      brbar[c] += dotbar * bt[c];
      btbar[c] += dotbar * br[c];
    }
  }
  for (int c = 0; c < 3; ++c) brefbar[c] = btgtbar[c] = 0.0;
  normalize_adjoint_add(b_ref, brbar, brefbar);
  normalize_adjoint_add(b_tgt, btbar, btgtbar);
}

// Adjoint of mat2rotvec as evaluated above (the four-way quaternion branch, 2 atan2(|xyz|, w) / |xyz| xyz; gradient 0
// where |xyz| == 0, the _div0 convention): relbar += J^T rvbar.
SF_HD void mat2rotvec_adjoint_add(const float* r, const double* rvbar, double* relbar) {
  const double r00 = r[0], r01 = r[1], r02 = r[2], r10 = r[3], r11 = r[4], r12 = r[5], r20 = r[6], r21 = r[7], r22 = r[8];
  const float trace = r[0] + r[4] + r[8];
  double x, y, z, w;
  int br;
  if (trace > 0.f) {
    br = 0; x = r21 - r12; y = r02 - r20; z = r10 - r01; w = 1.0 + ((r00 + r11) + r22);
  } else if (r[0] > r[4] && r[0] > r[8]) {
    br = 1; x = (1.0 - r22) + (r00 - r11); y = r10 + r01; z = r02 + r20; w = r21 - r12;
  } else if (r[4] > r[8]) {
    br = 2; x = r10 + r01; y = (1.0 - r22) - (r00 - r11); z = r21 + r12; w = r02 - r20;
  } else {
    br = 3; x = r02 + r20; y = r21 + r12; z = (1.0 + r22) - (r00 + r11); w = r10 - r01;
  }
  const double n2 = x * x + y * y + z * z, n = sqrt(n2);
  if (n == 0.0) return;
  const double at = atan2(n, w), f = 2.0 * at / n, q = n2 + w * w;
  const double fbar = rvbar[0] * x + rvbar[1] * y + rvbar[2] * z;
  const double nbar = fbar * (2.0 * (w / q) / n - 2.0 * at / n2);
  const double wb = fbar * (-2.0 / q);
  const double xb = f * rvbar[0] + nbar * x / n, yb = f * rvbar[1] + nbar * y / n, zb = f * rvbar[2] + nbar * z / n;
  if (br == 0) {
    relbar[7] += xb; relbar[5] -= xb; relbar[2] += yb; relbar[6] -= yb; relbar[3] += zb; relbar[1] -= zb;
    relbar[0] += wb; relbar[4] += wb; relbar[8] += wb;
  } else if (br == 1) {
    relbar[8] -= xb; relbar[0] += xb; relbar[4] -= xb; relbar[3] += yb; relbar[1] += yb; relbar[2] += zb; relbar[6] += zb;
    relbar[7] += wb; relbar[5] -= wb;
  } else if (br == 2) {
    relbar[3] += xb; relbar[1] += xb; relbar[8] -= yb; relbar[0] -= yb; relbar[4] += yb; relbar[7] += zb; relbar[5] += zb;
    relbar[2] += wb; relbar[6] -= wb;
  } else {
    relbar[2] += xb; relbar[6] += xb; relbar[7] += yb; relbar[5] += yb; relbar[8] += zb; relbar[0] -= zb; relbar[4] -= zb;
    relbar[3] += wb; relbar[1] -= wb;
  }
}

// ---- robust reweighting (k_robust_reweight and its host emulation) ---------------------
// The per-element pieces: the key of an error, the digit of a selection pass, the scale from the median and the four
// weight functions of u = e / (tuning * scale).  All four are rational: +, *, / alone (IEEE division).
enum RobustLoss { kRobustHuber = 0, kRobustCauchy = 1, kRobustGemanMcClure = 2, kRobustTukey = 3, kRobustLossCount = 4 };
constexpr int kRobustPasses = 4;               // 8 bits a pass, most significant first
constexpr uint32_t kRobustInfKey = 0x7F800000u;  // keys >= this one: inf and NaN

// The magnitude's bit pattern: non-negative floats order as these unsigned integers (denormals and inf included), every
// NaN lies above inf.  (The sign bit is dropped, so -0 has the key of 0.)
SF_HD uint32_t robust_key(float e) {
  uint32_t k;
  __builtin_memcpy(&k, &e, 4);
  return k & 0x7FFFFFFFu;
}
SF_HD float robust_key_value(uint32_t k) {
  float e;
  __builtin_memcpy(&e, &k, 4);
  return e;
}
SF_HD uint32_t robust_digit(uint32_t key, int pass) { return (key >> (24 - 8 * pass)) & 0xFFu; }
// what the passes before `pass` have fixed of a key: the selection counts the keys that agree with it there
SF_HD uint32_t robust_prefix(uint32_t key, int pass) { return pass == 0 ? 0u : key >> (32 - 8 * pass); }
// sigma = max(1.4826 * median, floor): the MAD-style consistency factor of the normal distribution, one fp32 product
SF_HD float robust_scale(float median, float floor) {
  const float s = 1.4826f * median;
  return s > floor ? s : floor;
}
SF_HD float robust_huber(float u) { return u <= 1.f ? 1.f : 1.f / u; }
SF_HD float robust_cauchy(float u) { return 1.f / (1.f + u * u); }
SF_HD float robust_geman_mcclure(float u) {
  const float d = 1.f + u * u;
  return 1.f / (d * d);
}
SF_HD float robust_tukey(float u) {
  if (!(u < 1.f)) return 0.f;
  const float t = (1.f - u) * (1.f + u);  // 1 - u^2 without the cancellation next to u = 1
  return t * t;
}
SF_HD float robust_weight(int loss, float u) {
  return loss == kRobustHuber ? robust_huber(u) : loss == kRobustCauchy ? robust_cauchy(u)
       : loss == kRobustGemanMcClure ? robust_geman_mcclure(u) : robust_tukey(u);
}

}  // namespace sf
