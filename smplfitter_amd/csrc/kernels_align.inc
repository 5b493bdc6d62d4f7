// ================================================================================================
// Procrustes alignment of point sets and the aligned errors (smplfit_align_points_f32,
// smplfit_mesh_error_aligned_f32; DESIGN.md §24).  Row-major sets: x (B, n, 3) the model, y (B, n, 3) the target,
// w (B, n) or null (= 1).  Four kernels, no float atomics, every sum in a fixed order:
//   k_align_moments     grid (B, nslab), block 256: the sf::kAlignMoments sums of kAlignSlab points of a row, about
//                       the row's provisional origins (the first point of each set), in fp64 -> part (nslab, B, 17)
//   k_align_solve       lane = row, fp64: the slabs added in slab order, sf::align_solve, the transform as fp32 to the
//                       caller and the row's record (s R, c, ox, oy) for the apply kernel
//   k_align_apply       one thread per point: |s R (x - ox) + c - (y - oy)|, rounded at the size of the body
//   k_align_row_means   one wave per row: sum w e / sum w in fp64, lanes strided, then a fixed butterfly
// A weight that is negative or not finite enters the sums as NaN, so its row is NaN; a non-finite point makes the
// moments of its row non-finite, which align_solve turns into a NaN transform.  Every output element has one writer.
// ================================================================================================
constexpr int kAlignSlab = 2048;  // points of a row per moments workgroup (eight a thread)

__device__ __forceinline__ double align_weight(const float* __restrict__ w, size_t i) {
  if (!w) return 1.0;
  const float v = w[i];
  return (v >= 0.f && v < __builtin_inff()) ? (double)v : __builtin_nan("");
}

__device__ __forceinline__ double align_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_align_moments(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ w, int n, int B, double* __restrict__ part) {
  __shared__ double red[4 * sf::kAlignMoments];
  const int row = blockIdx.x, slab = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)row * n;
  const float *xr = x + base * 3, *yr = y + base * 3;
  const float ox0 = xr[0], ox1 = xr[1], ox2 = xr[2], oy0 = yr[0], oy1 = yr[1], oy2 = yr[2];
  double m[sf::kAlignMoments];
#pragma unroll
  for (int k = 0; k < sf::kAlignMoments; ++k) m[k] = 0.0;
  const int i1 = min(n, (slab + 1) * kAlignSlab);
  for (int i = slab * kAlignSlab + tid; i < i1; i += 256) {
    const double wi = align_weight(w, base + i);
    // (differences of fp32 values in fp64: exact)
    const double a0 = (double)xr[3 * i] - ox0, a1 = (double)xr[3 * i + 1] - ox1, a2 = (double)xr[3 * i + 2] - ox2;
    const double b0 = (double)yr[3 * i] - oy0, b1 = (double)yr[3 * i + 1] - oy1, b2 = (double)yr[3 * i + 2] - oy2;
    const double wa0 = wi * a0, wa1 = wi * a1, wa2 = wi * a2;
    m[0] += wi;
    m[1] += wa0;
    m[2] += wa1;
    m[3] += wa2;
    m[4] += wi * b0;
    m[5] += wi * b1;
    m[6] += wi * b2;
    m[7] += b0 * wa0;
    m[8] += b0 * wa1;
    m[9] += b0 * wa2;
    m[10] += b1 * wa0;
    m[11] += b1 * wa1;
    m[12] += b1 * wa2;
    m[13] += b2 * wa0;
    m[14] += b2 * wa1;
    m[15] += b2 * wa2;
    m[16] += wa0 * a0 + wa1 * a1 + wa2 * a2;
  }
#pragma unroll
  for (int k = 0; k < sf::kAlignMoments; ++k) {
    const double v = align_wave_sum(m[k]);
    if (lane == 0) red[wave * sf::kAlignMoments + k] = v;
  }
  __syncthreads();
  if (tid < sf::kAlignMoments)
    part[((size_t)slab * B + row) * sf::kAlignMoments + tid] =
        (red[tid] + red[sf::kAlignMoments + tid]) + (red[2 * sf::kAlignMoments + tid] + red[3 * sf::kAlignMoments + tid]);
}

struct AlignSolveArgs {
  const double* part;   // (nslab, B, 17); with kAlignRoot: the moments of the joints, read for the row's validity alone
  const float *x, *y;   // the sets the moments were taken of (their first points are the origins); kAlignRoot: the joints
  int n, nslab, B, mode;
  float* rec;                   // (B, kAlignRecord)
  float *scale, *rot, *trans;   // out (B), (B, 9), (B, 3); each may be null
};

__global__ __launch_bounds__(64) void k_align_solve(AlignSolveArgs a) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= a.B) return;
  double m[sf::kAlignMoments];
#pragma unroll
  for (int k = 0; k < sf::kAlignMoments; ++k) m[k] = 0.0;
  for (int sl = 0; sl < a.nslab; ++sl) {
    const double* p = a.part + ((size_t)sl * a.B + row) * sf::kAlignMoments;
#pragma unroll
    for (int k = 0; k < sf::kAlignMoments; ++k) m[k] += p[k];
  }
  const float *xr = a.x + (size_t)row * a.n * 3, *yr = a.y + (size_t)row * a.n * 3;
  const double ox[3] = {xr[0], xr[1], xr[2]}, oy[3] = {yr[0], yr[1], yr[2]};
  double s, R[9], t[3], c[3];
  if (a.mode == sf::kAlignRoot) {  // joint 0 onto joint 0: the origins are the two roots, the centred offset is 0
    double chk = m[0] - m[0];
#pragma unroll
    for (int k = 1; k < sf::kAlignMoments; ++k) chk += m[k] - m[k];
    const bool ok = m[0] > 0.0 && chk == 0.0;
    const double nan = __builtin_nan("");
    s = ok ? 1.0 : nan;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = !ok ? nan : k % 4 == 0 ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t[k] = ok ? oy[k] - ox[k] : nan;
      c[k] = ok ? 0.0 : nan;
    }
  } else {
    sf::align_solve(a.mode, m, ox, oy, &s, R, t, c);
  }
  float* rec = a.rec + (size_t)row * sf::kAlignRecord;
#pragma unroll
  for (int k = 0; k < 9; ++k) rec[k] = (float)(s * R[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    rec[9 + k] = (float)c[k];
    rec[12 + k] = xr[k];
    rec[15 + k] = yr[k];
  }
  if (a.scale) a.scale[row] = (float)s;
  if (a.rot) {
#pragma unroll
    for (int k = 0; k < 9; ++k) a.rot[(size_t)row * 9 + k] = (float)R[k];
  }
  if (a.trans) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.trans[(size_t)row * 3 + k] = (float)t[k];
  }
}

// err[i] = |M (x_i - ox) + c - (y_i - oy)| over the B n points of two (B, n, 3) arrays, (M, c, ox, oy) the record of
// the point's row; one thread per point.  The two differences are taken first: what is multiplied and added is of the
// size of the body.
__global__ __launch_bounds__(256) void k_align_apply(const float* __restrict__ x, const float* __restrict__ y,
                                                     const float* __restrict__ rec, float* __restrict__ err, int n, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float* r = rec + (i / (size_t)n) * sf::kAlignRecord;
  const float *px = x + i * 3, *py = y + i * 3;
  const float a0 = __fsub_rn(px[0], r[12]), a1 = __fsub_rn(px[1], r[13]), a2 = __fsub_rn(px[2], r[14]);
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float moved = __fmaf_rn(r[3 * k + 2], a2, __fmaf_rn(r[3 * k + 1], a1, __fmaf_rn(r[3 * k], a0, r[9 + k])));
    d[k] = __fsub_rn(moved, __fsub_rn(py[k], r[15 + k]));
  }
  err[i] = point_distance(d[0], d[1], d[2]);
}

// mean[row] = sum_i w_i e_i / sum_i w_i over the n errors of a row (w null: 1), one wave per row, four rows a workgroup
__global__ __launch_bounds__(256) void k_align_row_means(const float* __restrict__ err, const float* __restrict__ w, int n, int B,
                                                         float* __restrict__ mean) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;  // (whole waves leave together)
  const size_t base = (size_t)row * n;
  double swe = 0.0, sw = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double wi = align_weight(w, base + i);
    swe += wi * (double)err[base + i];
    sw += wi;
  }
  swe = align_wave_sum(swe);
  sw = align_wave_sum(sw);
  if (lane == 0) mean[row] = (float)(swe / sw);
}
