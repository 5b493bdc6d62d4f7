// Adjoint of the shape solve (smplfit_shape_solve_backward_f32): the gradients of a fit_with_known_pose.
// Included by smplfit_hip.hip (same anonymous namespace).  DESIGN.md §16.
//
//   k_forward_joint + k_adj_zero_bias + posedirs GEMM   recompute: the pose blend shapes WITHOUT the template
//                 (instance-major ws.vposed); nothing is kept from the forward
//   k_adj_gram    grid B, block 256: per instance the FK Jacobian of the joints in LDS, then tiles of 64 sorted slots:
//                 three waves build the 192 Jacobian rows of a tile in LDS (wave = coordinate, lane = vertex), then every
//                 thread owns ONE entry of [sum w A^T A | sum w A | W] and adds the tile's rows in row order (fp32), the
//                 tile totals in tile order (fp64); the target joints are one more tile.  The same workgroup assembles
//                 and solves the system in fp64 (sf::shape_adjoint_solve) and writes (lambda_x, lambda_t) and the
//                 gradients of the ridge references.  It accumulates its own normal matrix: no dependence on the route
//                 the forward's solve took.
//   k_adj_apply   grid B, block 256: second vertex pass: p_n, res_n and delta_n in registers; the gradients of the targets
//                 and weights and, when the rotations want a gradient, the two cotangent streams; the joints likewise
//   3 x smplfit_forward_backward_f32 + k_adj_combine   the gradient of the global rotations (DESIGN.md §16)
// No float atomics: every sum has a fixed order, the results are bitwise run-to-run deterministic.

constexpr int kAdjTile = 64;  // vertices (or joints) per LDS tile of k_adj_gram: 192 rows

struct AdjWorkspace {
  float* lam;   // (B, S + 3) lambda_x | lambda_t
  float* lamb;  // (B, nb) lambda of the caller's betas, lamk (B) of the kid unknown: the second backward call's inputs
  float* lamk;
  float *c1, *c2;    // (B, V, 3) -w delta, w res
  float *c1j, *c2j;  // (B, J, 3)
  float *g1, *g2, *g3;  // (B, J, 9) the three vector-Jacobian products
};

struct AdjArgs {
  const float *glob, *tv, *tj;
  const float *vw, *jw;  // the weights the rule reads (bodyfitter.py:1018-1028), else NULL (= 1)
  float beta_reg, beta_reg2, kid_reg;
  int nb, nref;
  const float *betas, *trans, *kid;        // the forward's solution
  const float *g_betas, *g_trans, *g_kid;  // cotangents or NULL
  float *o_tv, *o_tj, *o_vw, *o_jw, *o_bref, *o_kref;
  int want_glob;
};

__host__ __device__ inline int adj_row_pitch(int S) { return S | 1; }  // odd: lanes writing their rows hit distinct LDS banks
inline size_t adj_gram_lds_bytes(const DevModel& d) {
  const size_t S = d.S, J = d.J;
  return (sf::adj_sums(d.S) + S * S + 2 * S) * 8 +
         (J * 9 + 2 * J * 3 * (S + 1) + 3 * kAdjTile * adj_row_pitch(d.S) + kAdjTile + 2 * S + 6) * 4;
}
inline size_t adj_apply_lds_bytes(const DevModel& d) {
  const size_t S = d.S, J = d.J;
  return (J * 9 + 2 * J * 3 * (S + 1) + 6 * J + 2 * S + 6) * 4;
}

// the tile's rows (LDS) added to the thread's entry: kind 0 = (ei, ej) of the triangle, 1 = sum w A[ei][ej], 2 = W
__device__ __forceinline__ float adj_tile_entry(const float* rows, const float* wrow, int RS, int n, int kind, int ei, int ej) {
  float part = 0.f;
  if (kind == 0) {
    for (int c = 0; c < 3; ++c)
      for (int v = 0; v < n; ++v) {
        const float* r = rows + (c * kAdjTile + v) * RS;
        part += (wrow[v] * r[ei]) * r[ej];
      }
  } else if (kind == 1) {
    for (int v = 0; v < n; ++v) part += wrow[v] * rows[(ei * kAdjTile + v) * RS + ej];
  } else if (kind == 2) {
    for (int v = 0; v < n; ++v) part += wrow[v];
  }
  return part;
}

// grid B, block 256
__global__ __launch_bounds__(256) void k_adj_gram(DevModel m, AdjArgs a, AdjWorkspace aw, int B) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = m.S, S1 = S + 1, J = m.J, V = m.V, RS = adj_row_pitch(S), NG = sf::ne_ng(S), NS = sf::adj_sums(S);
  const size_t Vp = m.Vp;
  const int b = blockIdx.x, tid = threadIdx.x;
  double* sum = reinterpret_cast<double*>(smem);  // [NS]
  double* M = sum + NS;                           // [S][S]
  double* x = M + S * S;                          // [S]
  double* rd = x + S;                             // [S]
  float* sG = reinterpret_cast<float*>(rd + S);   // [J][9]
  float* Pe = sG + J * 9;                         // [J][3][S1]
  float* Te = Pe + J * 3 * S1;                    // [J][3][S1]
  float* rows = Te + J * 3 * S1;                  // [3][kAdjTile][RS]
  float* wrow = rows + 3 * kAdjTile * RS;         // [kAdjTile]
  float* gx = wrow + kAdjTile;                    // [S]
  float* gt = gx + S;                             // [3]
  float* lam = gt + 3;                            // [S + 3]
  for (int k = tid; k < J * 9; k += 256) sG[k] = a.glob[(size_t)b * J * 9 + k];
  for (int s = tid; s < S; s += 256) {
    float v = (a.g_betas && s < a.nb) ? a.g_betas[(size_t)b * a.nb + s] : 0.f;
    if (a.g_kid && m.jt.n_kid && s == S - 1) v = a.g_kid[b];
    gx[s] = v;
  }
  if (tid < 3) gt[tid] = a.g_trans ? a.g_trans[(size_t)b * 3 + tid] : 0.f;
  __syncthreads();
  DevCtx cx{tid, 256};
  sf::shape_adjoint_fk(cx, m.jt, sG, Pe, Te);
  // the entry this thread owns
  int kind = 3, ei = 0, ej = 0;
  if (tid < NG) {
    int i = 0, r = tid;
    while (r >= S - i) {
      r -= S - i;
      ++i;
    }
    kind = 0, ei = i, ej = i + r;
  } else if (tid < NG + 3 * S) {
    kind = 1, ei = (tid - NG) / S, ej = (tid - NG) % S;
  } else if (tid == NG + 3 * S) {
    kind = 2;
  }
  double acc = 0.0;
  const int c = tid >> 6, v = tid & 63;
  for (int t0 = 0; t0 < V; t0 += kAdjTile) {
    if (c < 3) {
      const int i = t0 + v;
      float* row = rows + (c * kAdjTile + v) * RS;
      if (i < V) {
        sf::shape_adjoint_vertex_row(S, m.KW, Vp, sG, Te, m.sd, m.widx, m.wval, (size_t)i, c, row);
      } else {
        for (int s = 0; s < S; ++s) row[s] = 0.f;
      }
      if (c == 0) wrow[v] = i < V ? (a.vw ? a.vw[(size_t)b * V + m.perm[i]] : 1.f) : 0.f;
    }
    __syncthreads();
    acc += (double)adj_tile_entry(rows, wrow, RS, min(kAdjTile, V - t0), kind, ei, ej);
    __syncthreads();
  }
  if (a.tj)
    for (int j0 = 0; j0 < J; j0 += kAdjTile) {
      if (c < 3) {
        const int j = j0 + v;
        float* row = rows + (c * kAdjTile + v) * RS;
        for (int s = 0; s < S; ++s) row[s] = j < J ? Pe[(j * 3 + c) * S1 + 1 + s] : 0.f;
        if (c == 0) wrow[v] = j < J ? (a.jw ? a.jw[(size_t)b * J + j] : 1.f) : 0.f;
      }
      __syncthreads();
      acc += (double)adj_tile_entry(rows, wrow, RS, min(kAdjTile, J - j0), kind, ei, ej);
      __syncthreads();
    }
  if (kind < 3) sum[tid] = acc;
  __syncthreads();
  sf::shape_adjoint_solve(cx, m.jt, sum, a.beta_reg, a.beta_reg2, a.kid_reg, gx, gt, M, x, rd, lam);
  for (int k = tid; k < S + 3; k += 256) aw.lam[(size_t)b * (S + 3) + k] = lam[k];
  for (int s = tid; s < a.nb; s += 256) aw.lamb[(size_t)b * a.nb + s] = lam[s];
  if (tid == 0) aw.lamk[b] = m.jt.n_kid ? lam[S - 1] : 0.f;
  if (a.o_bref)
    for (int s = tid; s < a.nref; s += 256)
      a.o_bref[(size_t)b * a.nref + s] = (float)sf::ridge_weight(m.jt, s, a.beta_reg, a.beta_reg2, a.kid_reg) * lam[s];
  if (a.o_kref && tid == 0) a.o_kref[b] = a.kid_reg * lam[S - 1];
}

// grid B, block 256.  vertex_pass: a vertex-sized output (or cotangent stream) is wanted.
__global__ __launch_bounds__(256) void k_adj_apply(DevModel m, Workspace ws, AdjArgs a, AdjWorkspace aw, int B, int vertex_pass) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = m.S, S1 = S + 1, J = m.J, V = m.V;
  const size_t Vp = m.Vp;
  const int b = blockIdx.x, tid = threadIdx.x;
  float* sG = smem;               // [J][9]
  float* Pe = sG + J * 9;         // [J][3][S1]
  float* Te = Pe + J * 3 * S1;    // [J][3][S1]
  float* jx = Te + J * 3 * S1;    // [J][3] Te [1 | x]
  float* jl = jx + J * 3;         // [J][3] Te [0 | lambda_x]
  float* sx = jl + J * 3;         // [S]
  float* slam = sx + S;           // [S + 3]
  float* str = slam + S + 3;      // [3]
  for (int k = tid; k < J * 9; k += 256) sG[k] = a.glob[(size_t)b * J * 9 + k];
  for (int s = tid; s < S; s += 256) {
    float v = s < a.nb ? a.betas[(size_t)b * a.nb + s] : 0.f;
    if (a.kid && m.jt.n_kid && s == S - 1) v = a.kid[b];
    sx[s] = v;
  }
  for (int k = tid; k < S + 3; k += 256) slam[k] = aw.lam[(size_t)b * (S + 3) + k];
  if (tid < 3) str[tid] = a.trans[(size_t)b * 3 + tid];
  __syncthreads();
  DevCtx cx{tid, 256};
  sf::shape_adjoint_fk(cx, m.jt, sG, Pe, Te);
  for (int k = tid; k < J * 3; k += 256) {
    float px = Te[k * S1], pl = 0.f;
    for (int s = 0; s < S; ++s) {
      px += Te[k * S1 + 1 + s] * sx[s];
      pl += Te[k * S1 + 1 + s] * slam[s];
    }
    jx[k] = px;
    jl[k] = pl;
  }
  __syncthreads();
  if (vertex_pass) {
    const float* vps = ws.vposed + (size_t)b * 3 * Vp;
    for (int i = tid; i < V; i += 256) {
      const size_t o = (size_t)b * V + m.perm[i];
      // (the posedirs product arrives WITHOUT the template, see k_adj_zero_bias: one rounding at the template's magnitude)
      const float vp[3] = {m.vt[i] + vps[i], m.vt[Vp + i] + vps[Vp + i], m.vt[2 * Vp + i] + vps[2 * Vp + i]};
      float pos[3], al[3], y[3], gy[3], wres[3];
      sf::shape_adjoint_vertex_dots(S, m.KW, Vp, sG, jx, jl, m.sd, m.widx, m.wval, (size_t)i, vp, sx, slam, pos, al);
      for (int c = 0; c < 3; ++c) y[c] = a.tv[o * 3 + c];
      const float dot = sf::shape_adjoint_point(pos, al, str, slam + S, y, a.vw ? a.vw[o] : 1.f, gy, wres);
      if (a.o_tv)
        for (int c = 0; c < 3; ++c) a.o_tv[o * 3 + c] = gy[c];
      if (a.o_vw) a.o_vw[o] = a.vw ? dot : 0.f;
      if (a.want_glob)
        for (int c = 0; c < 3; ++c) {
          aw.c1[o * 3 + c] = -gy[c];
          aw.c2[o * 3 + c] = wres[c];
        }
    }
  }
  if (a.tj)
    for (int j = tid; j < J; j += 256) {
      const size_t o = (size_t)b * J + j;
      float pos[3], al[3], y[3], gy[3], wres[3];
      for (int c = 0; c < 3; ++c) {
        const float* pe = Pe + (j * 3 + c) * S1;
        float px = pe[0], pl = 0.f;
        for (int s = 0; s < S; ++s) {
          px += pe[1 + s] * sx[s];
          pl += pe[1 + s] * slam[s];
        }
        pos[c] = px, al[c] = pl, y[c] = a.tj[o * 3 + c];
      }
      const float dot = sf::shape_adjoint_point(pos, al, str, slam + S, y, a.jw ? a.jw[o] : 1.f, gy, wres);
      if (a.o_tj)
        for (int c = 0; c < 3; ++c) a.o_tj[o * 3 + c] = gy[c];
      if (a.o_jw) a.o_jw[o] = a.jw ? dot : 0.f;
      if (a.want_glob)
        for (int c = 0; c < 3; ++c) {
          aw.c1j[o * 3 + c] = -gy[c];
          aw.c2j[o * 3 + c] = wres[c];
        }
    }
}

// grid ceil(B / 256): the bias feature of the posedirs GEMM (the 1 that multiplies the template row) set to 0, so that the
// product holds the pose blend shapes alone.  They are of order 1e-2 m: summed into an accumulator that carries the
// template (order 1 m) every one of the P additions rounds at the template's magnitude (~2e-7 m in all, 1e-5 of the
// residual the weight gradients are made of); k_adj_apply adds the template itself, once.
__global__ __launch_bounds__(256) void k_adj_zero_bias(float* __restrict__ rp, int B, int Kp, int pos) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) rp[(size_t)b * Kp + pos] = 0.f;
}

// grad G = VJP(x; -w delta) + (VJP(lambda; w res) - VJP(0; w res))
__global__ __launch_bounds__(256) void k_adj_combine(const float* __restrict__ g1, const float* __restrict__ g2,
                                                     const float* __restrict__ g3, float* __restrict__ out, size_t n) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) out[e] = g1[e] + (g2[e] - g3[e]);
}

// ================================================================================================
// Adjoint of the whole fit (smplfit_fit_backward_f32, DESIGN.md §17).  The per-instance arithmetic is sf::fit_rot_* /
// sf::fit_tail_adjoint (sf_stages.h), ONE lane per instance like k_bwd_joint; the vertex passes are one workgroup per
// instance, one wave per part, every vertex with a single writer.  Vertex arrays here are (B, V, 3) in the caller's
// vertex order; the part of a vertex comes from the part-aligned segments of the sorted slots.
//   k_fa_center      centred copies of the targets (the mean over V (+ J) points, fp64 sums in a fixed order)
//   k_fa_regress     joints regressed from a mesh (the centred targets, a fitted mesh, or the default mesh)
//   k_fa_partsums    fp64 part sums of (targets, reference mesh): the backward's own, see sf::fit_part_cov
//   k_fa_rot_fwd     one rotation pass                         k_fa_rot_adj   its adjoint
//   k_fa_tail        output stage + refinement, forward and adjoint
//   k_fa_vertex      the part-sum adjoint (a gather) and the regressor's transpose
//   k_fa_uncenter    the centring step, into the caller's outputs
//   k_fa_add         dst += src
//   k_fa_align       the alignment of a known-shape fit (§18): t, and the mesh and joints moved by it
//   k_fa_align_adj   its adjoint: the complete tbar, then the targets', the mesh's and the weights' share of it
// ================================================================================================
__device__ __forceinline__ double fa_wave_sum(double v) {  // fixed tree: the total in every lane's view of lane 0
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// grid B, block 256
__global__ __launch_bounds__(256) void k_fa_center(DevModel m, const float* __restrict__ tv, const float* __restrict__ tj,
                                                   float* __restrict__ ctv, float* __restrict__ ctj) {
  __shared__ double red[256 * 3];
  __shared__ double mean[3];
  const int b = blockIdx.x, tid = threadIdx.x, V = m.V, J = m.J;
  const float* t = tv + (size_t)b * V * 3;
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < V; i += 256)
    for (int c = 0; c < 3; ++c) s[c] += (double)t[(size_t)i * 3 + c];
  if (tj)
    for (int j = tid; j < J; j += 256)
      for (int c = 0; c < 3; ++c) s[c] += (double)tj[((size_t)b * J + j) * 3 + c];
  for (int c = 0; c < 3; ++c) red[tid * 3 + c] = s[c];
  __syncthreads();
  if (tid < 3) {
    double a = 0.0;
    for (int k = 0; k < 256; ++k) a += red[k * 3 + tid];
    mean[tid] = a / (double)(V + (tj ? J : 0));
  }
  __syncthreads();
  for (int k = tid; k < V * 3; k += 256) ctv[(size_t)b * V * 3 + k] = (float)((double)t[k] - mean[k % 3]);
  if (tj)
    for (int k = tid; k < J * 3; k += 256)
      ctj[(size_t)b * J * 3 + k] = (float)((double)tj[(size_t)b * J * 3 + k] - mean[k % 3]);
}

// grid B (1 for a shared mesh), block 64.  src (B, V, 3), or null: the default mesh.
__global__ __launch_bounds__(64) void k_fa_regress(DevModel m, const float* __restrict__ src, float* __restrict__ out) {
  const int b = blockIdx.x, V = m.V;
  for (int j = threadIdx.x; j < m.J; j += 64) {
    float a[3] = {0.f, 0.f, 0.f};
    for (int k = m.reg_start[j]; k < m.reg_start[j + 1]; ++k) {
      const int i = m.reg_slot[k];
      const float r = m.reg_val[k];
      for (int c = 0; c < 3; ++c) a[c] += r * (src ? src[((size_t)b * V + m.perm[i]) * 3 + c] : m.dm[(size_t)c * m.Vp + i]);
    }
    for (int c = 0; c < 3; ++c) out[((size_t)b * m.J + j) * 3 + c] = a[c];
  }
}

// grid B, block 256.  ref (B, V, 3), or null: the default mesh.  psum (B, J, kPsum) doubles.
__global__ __launch_bounds__(256) void k_fa_partsums(DevModel m, const float* __restrict__ ctv, const float* __restrict__ ref,
                                                     const float* __restrict__ vw, double* __restrict__ psum) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, V = m.V;
  for (int p = wave; p < m.J; p += 4) {
    double acc[sf::kPsum];
    for (int k = 0; k < sf::kPsum; ++k) acc[k] = 0.0;
    for (int s = m.part_seg_start[p]; s < m.part_seg_start[p + 1]; ++s) {
      const int start = m.segments[s * 3], count = m.segments[s * 3 + 1];
      if (lane >= count) continue;
      const int i = start + lane, o = m.perm[i];
      const size_t e = (size_t)b * V + o;
      const float t[3] = {ctv[e * 3], ctv[e * 3 + 1], ctv[e * 3 + 2]};
      float a[3];
      for (int c = 0; c < 3; ++c) a[c] = ref ? ref[e * 3 + c] : m.dm[(size_t)c * m.Vp + i];
      sf::partsum_vertex_d(t, a, vw ? vw[e] : 1.f, acc);
    }
    for (int k = 0; k < sf::kPsum; ++k) {
      const double r = fa_wave_sum(acc[k]);
      if (lane == 0) psum[((size_t)b * m.J + p) * sf::kPsum + k] = r;
    }
  }
}

// the joints an instance's rotation stage reads: (B, J, 3), or one (J, 3) row for every instance
struct FaJoints {
  const float *tj, *rj;
  int rj_shared;
  const float* jw;  // (B, J) or null
};

// grid ceil(B / 64), block 64
__global__ __launch_bounds__(64) void k_fa_rot_fwd(DevModel m, const double* __restrict__ psum, FaJoints jn,
                                                   const float* __restrict__ Gprev, float* __restrict__ Gout, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x, J = m.J;
  if (b >= B) return;
  sf::fit_rot_forward(m.jt, psum + (size_t)b * J * sf::kPsum, jn.tj + (size_t)b * J * 3,
                      jn.rj + (jn.rj_shared ? 0 : (size_t)b * J * 3), jn.jw ? jn.jw + (size_t)b * J : nullptr,
                      Gprev ? Gprev + (size_t)b * J * 9 : nullptr, Gout + (size_t)b * J * 9);
}

// the cotangents a joint-level adjoint leaves for k_fa_vertex: the part records and the joints' / joint weights'
struct FaJointCot {
  float* pbar;   // (B, J, kPsum) records [Abar | ct | ca]
  float* tjbar;  // (B, J, 3) target joints
  float* rjtbar; // (B, J, 3) reference joints of the joint term (regressed without target joints)
  float* rjbar;  // (B, J, 3) joints of the solve
  float* jwbar;  // (B, J)
};

// grid ceil(B / 64), block 64.  Gbar: the cotangent of the pass's output; Gprev_bar: written when Gprev is given.
__global__ __launch_bounds__(64) void k_fa_rot_adj(DevModel m, const double* __restrict__ psum, FaJoints jn,
                                                   const float* __restrict__ Gprev, const float* __restrict__ Gbar,
                                                   float* __restrict__ Gprev_bar, double* __restrict__ scr, FaJointCot o, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x, J = m.J;
  if (b >= B) return;
  double* sc = scr + (size_t)b * sf::fit_tail_adjoint_scratch(J);
  sf::fit_rot_adjoint(m.jt, psum + (size_t)b * J * sf::kPsum, jn.tj + (size_t)b * J * 3,
                      jn.rj + (jn.rj_shared ? 0 : (size_t)b * J * 3), jn.jw ? jn.jw + (size_t)b * J : nullptr,
                      Gprev ? Gprev + (size_t)b * J * 9 : nullptr, Gbar + (size_t)b * J * 9, o.pbar + (size_t)b * J * sf::kPsum,
                      Gprev ? Gprev_bar + (size_t)b * J * 9 : nullptr, sc);
  for (int k = 0; k < J * 3; ++k) {
    o.tjbar[(size_t)b * J * 3 + k] = (float)sc[k];
    o.rjtbar[(size_t)b * J * 3 + k] = (float)sc[J * 3 + k];
    o.rjbar[(size_t)b * J * 3 + k] = 0.f;
  }
  for (int k = 0; k < J; ++k) o.jwbar[(size_t)b * J + k] = (float)sc[J * 6 + k];
}

struct FaTailArgs {
  const float *G, *betas, *kid, *trans;  // the last iteration's rotations and solution (centred frame)
  const float* rj_true;                  // (B, J, 3) joints of that solve (refinement only)
  int final_adjust, nb;
  const float *g_pose, *g_orient, *g_rel, *g_betas, *g_kid, *g_trans;  // the caller's cotangents or null
  float *Gbar, *xb, *kb, *tb;  // out: the cotangents of the rotations (B,J,9), betas (B,nb), kid (B), trans (B,3)
};

// grid ceil(B / 64), block 64
__global__ __launch_bounds__(64) void k_fa_tail(DevModel m, const double* __restrict__ psum, FaJoints jn, FaTailArgs a,
                                                double* __restrict__ scr, FaJointCot o, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x, J = m.J, S = m.S;
  if (b >= B) return;
  float x[sf::kAdjMaxUnknowns], xbar[sf::kAdjMaxUnknowns], tbar[3];
  for (int s = 0; s < S; ++s) x[s] = s < a.nb ? a.betas[(size_t)b * a.nb + s] : 0.f;
  if (m.jt.n_kid) x[S - 1] = a.kid ? a.kid[b] : 0.f;
  double* sc = scr + (size_t)b * sf::fit_tail_adjoint_scratch(J);
  const bool fa = a.final_adjust != 0;
  sf::fit_tail_adjoint(m.jt, a.G + (size_t)b * J * 9, x, a.trans + (size_t)b * 3, psum + (size_t)b * J * sf::kPsum,
                       fa ? jn.tj + (size_t)b * J * 3 : nullptr, fa ? jn.rj + (size_t)b * J * 3 : nullptr,
                       fa ? a.rj_true + (size_t)b * J * 3 : nullptr, jn.jw ? jn.jw + (size_t)b * J : nullptr, fa,
                       a.g_pose ? a.g_pose + (size_t)b * J * 3 : nullptr, a.g_orient ? a.g_orient + (size_t)b * J * 9 : nullptr,
                       a.g_rel ? a.g_rel + (size_t)b * J * 9 : nullptr, sc, a.Gbar + (size_t)b * J * 9, xbar, tbar,
                       o.pbar + (size_t)b * J * sf::kPsum);
  for (int s = 0; s < a.nb; ++s) a.xb[(size_t)b * a.nb + s] = xbar[s] + (a.g_betas ? a.g_betas[(size_t)b * a.nb + s] : 0.f);
  a.kb[b] = m.jt.n_kid ? xbar[S - 1] + (a.g_kid ? a.g_kid[b] : 0.f) : 0.f;
  for (int c = 0; c < 3; ++c) a.tb[(size_t)b * 3 + c] = tbar[c] + (a.g_trans ? a.g_trans[(size_t)b * 3 + c] : 0.f);
  for (int k = 0; k < J * 3; ++k) {
    o.tjbar[(size_t)b * J * 3 + k] = (float)sc[sf::fit_tail_tjbar(J) + k];
    o.rjtbar[(size_t)b * J * 3 + k] = (float)sc[sf::fit_tail_rjtbar(J) + k];
    o.rjbar[(size_t)b * J * 3 + k] = (float)sc[sf::fit_tail_rjbar(J) + k];
  }
  for (int k = 0; k < J; ++k) o.jwbar[(size_t)b * J + k] = (float)sc[sf::fit_tail_jwbar(J) + k];
}

struct FaVertexArgs {
  const float *ctv, *ref, *vw;  // ref null: the default mesh (no cotangent)
  int regressed;                // the joints of the stage were regressed from the vertices
  float *acc_tv, *acc_tj, *acc_vw, *acc_jw;  // += ; acc_tj with target joints; acc_vw / acc_jw may be null
  float *meshbar, *jointsbar;   // = ; null with the default mesh
};

// grid B, block 256
__global__ __launch_bounds__(256) void k_fa_vertex(DevModel m, FaVertexArgs a, FaJointCot jc) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = m.V, J = m.J;
  if (a.meshbar) {  // (the vertices of the parts that take no sums keep a zero cotangent)
    for (int k = tid; k < V * 3; k += 256) a.meshbar[(size_t)b * V * 3 + k] = 0.f;
    __syncthreads();
  }
  for (int p = wave; p < J; p += 4) {
    const float* rec = jc.pbar + ((size_t)b * J + p) * sf::kPsum;
    for (int s = m.part_seg_start[p]; s < m.part_seg_start[p + 1]; ++s) {
      const int start = m.segments[s * 3], count = m.segments[s * 3 + 1];
      if (lane >= count) continue;
      const int i = start + lane, o = m.perm[i];
      const size_t e = (size_t)b * V + o;
      const float t[3] = {a.ctv[e * 3], a.ctv[e * 3 + 1], a.ctv[e * 3 + 2]};
      float r[3], tb[3], ab[3];
      for (int c = 0; c < 3; ++c) r[c] = a.ref ? a.ref[e * 3 + c] : m.dm[(size_t)c * m.Vp + i];
      const float wb = sf::partsum_vertex_adjoint(t, r, a.vw ? a.vw[e] : 1.f, a.vw != nullptr, rec, tb, ab);
      for (int c = 0; c < 3; ++c) {
        a.acc_tv[e * 3 + c] += tb[c];
        if (a.meshbar) a.meshbar[e * 3 + c] = ab[c];
      }
      if (a.vw && a.acc_vw) a.acc_vw[e] += wb;
    }
  }
  for (int k = tid; k < J; k += 256)
    if (a.acc_jw) a.acc_jw[(size_t)b * J + k] += jc.jwbar[(size_t)b * J + k];
  for (int k = tid; k < J * 3; k += 256) {
    const size_t e = (size_t)b * J * 3 + k;
    if (!a.regressed) a.acc_tj[e] += jc.tjbar[e];
    if (a.jointsbar) a.jointsbar[e] = jc.rjbar[e] + (a.regressed ? 0.f : jc.rjtbar[e]);
  }
  if (!a.regressed) return;
  // the regressor's transpose: joint after joint (the slots of one row are distinct: one writer per vertex and step)
  for (int j = 0; j < J; ++j) {
    __syncthreads();
    const float* gt = jc.tjbar + ((size_t)b * J + j) * 3;
    const float* gr = jc.rjtbar + ((size_t)b * J + j) * 3;
    for (int k = m.reg_start[j] + tid; k < m.reg_start[j + 1]; k += 256) {
      const size_t e = (size_t)b * V + m.perm[m.reg_slot[k]];
      const float r = m.reg_val[k];
      for (int c = 0; c < 3; ++c) {
        a.acc_tv[e * 3 + c] += r * gt[c];
        if (a.meshbar) a.meshbar[e * 3 + c] += r * gr[c];
      }
    }
  }
}

// grid B, block 256.  acc_tj null without target joints; the outputs may be null.
__global__ __launch_bounds__(256) void k_fa_uncenter(DevModel m, const float* __restrict__ acc_tv, const float* __restrict__ acc_tj,
                                                     const float* __restrict__ g_trans, float* __restrict__ out_tv,
                                                     float* __restrict__ out_tj) {
  __shared__ double red[256 * 3];
  __shared__ float corr[3];
  const int b = blockIdx.x, tid = threadIdx.x, V = m.V, J = m.J;
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < V; i += 256)
    for (int c = 0; c < 3; ++c) s[c] += (double)acc_tv[((size_t)b * V + i) * 3 + c];
  if (acc_tj)
    for (int j = tid; j < J; j += 256)
      for (int c = 0; c < 3; ++c) s[c] += (double)acc_tj[((size_t)b * J + j) * 3 + c];
  for (int c = 0; c < 3; ++c) red[tid * 3 + c] = s[c];
  __syncthreads();
  if (tid < 3) {
    double t = 0.0;
    for (int k = 0; k < 256; ++k) t += red[k * 3 + tid];
    corr[tid] = sf::centring_correction(t, g_trans ? g_trans[(size_t)b * 3 + tid] : 0.f, V + (acc_tj ? J : 0));
  }
  __syncthreads();
  if (out_tv)
    for (int k = tid; k < V * 3; k += 256) out_tv[(size_t)b * V * 3 + k] = acc_tv[(size_t)b * V * 3 + k] + corr[k % 3];
  if (out_tj && acc_tj)
    for (int k = tid; k < J * 3; k += 256) out_tj[(size_t)b * J * 3 + k] = acc_tj[(size_t)b * J * 3 + k] + corr[k % 3];
}

__global__ __launch_bounds__(256) void k_fa_add(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) dst[e] += src[e];
}

// ---- the alignment stage of a known-shape fit and its adjoint (smplfit_fit_known_shape_backward_f32, DESIGN.md §18) ----
struct FaAlign {
  const float *ctv, *ctj;  // the centred targets; ctj null (no target joints): the sums run over the vertices alone
  const float *vw, *jw;    // the weights that count (solve_weights), or null: every point counts once
};

// the block's fp64 records summed in a fixed order: red (256, kAlign) -> tot (kAlign)
__device__ __forceinline__ void fa_align_reduce(const double* s, double* red, double* tot) {
  const int tid = threadIdx.x;
  for (int k = 0; k < sf::kAlign; ++k) red[tid * sf::kAlign + k] = s[k];
  __syncthreads();
  if (tid < sf::kAlign) {
    double a = 0.0;
    for (int k = 0; k < 256; ++k) a += red[k * sf::kAlign + tid];
    tot[tid] = a;
  }
  __syncthreads();
}

// grid B, block 256.  mesh (B, V, 3), joints (B, J, 3): in the model at the last rotations, out moved by t; trans (B, 3) out.
__global__ __launch_bounds__(256) void k_fa_align(DevModel m, FaAlign a, float* __restrict__ mesh, float* __restrict__ joints,
                                                  float* __restrict__ trans) {
  __shared__ double red[256 * sf::kAlign];
  __shared__ double tot[sf::kAlign];
  const int b = blockIdx.x, tid = threadIdx.x, V = m.V, J = m.J;
  double s[sf::kAlign] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < V; i += 256) {
    const size_t e = (size_t)b * V + i;
    sf::align_point_d(a.ctv + e * 3, mesh + e * 3, a.vw ? a.vw[e] : 1.f, s);
  }
  if (a.ctj)
    for (int j = tid; j < J; j += 256) {
      const size_t e = (size_t)b * J + j;
      sf::align_point_d(a.ctj + e * 3, joints + e * 3, a.jw ? a.jw[e] : 1.f, s);
    }
  fa_align_reduce(s, red, tot);
  float t[3];
  sf::align_translation(tot, t);
  if (tid < 3) trans[(size_t)b * 3 + tid] = t[tid];
  for (int k = tid; k < V * 3; k += 256) mesh[(size_t)b * V * 3 + k] += t[k % 3];
  for (int k = tid; k < J * 3; k += 256) joints[(size_t)b * J * 3 + k] += t[k % 3];
}

struct FaAlignAdj {
  FaAlign in;
  const float *mesh, *joints;                // the aligned mesh and joints (k_fa_align's)
  float *meshbar, *jointsbar;                // in: the cotangents of the aligned mesh / joints; out: of the model's
  float* tb;                                 // (B, 3) in: the refinement's and the caller's; out: the complete tbar
  float *acc_tv, *acc_tj, *acc_vw, *acc_jw;  // += ; acc_vw / acc_jw may be null
};

// grid B, block 256.  tbar += sum meshbar + sum jointsbar (the aligned points carry t), q = tbar / W, then per point
// (one writer each): target += w q, model -= w q, weight += q . (tau - m).
__global__ __launch_bounds__(256) void k_fa_align_adj(DevModel m, FaAlignAdj a) {
  __shared__ double red[256 * sf::kAlign];
  __shared__ double tot[sf::kAlign];
  const int b = blockIdx.x, tid = threadIdx.x, V = m.V, J = m.J;
  double s[sf::kAlign] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < V; i += 256) {
    const size_t e = (size_t)b * V + i;
    for (int c = 0; c < 3; ++c) s[c] += (double)a.meshbar[e * 3 + c];
    s[3] += a.in.vw ? (double)a.in.vw[e] : 1.0;
  }
  for (int j = tid; j < J; j += 256) {
    const size_t e = (size_t)b * J + j;
    for (int c = 0; c < 3; ++c) s[c] += (double)a.jointsbar[e * 3 + c];
    if (a.in.ctj) s[3] += a.in.jw ? (double)a.in.jw[e] : 1.0;
  }
  const float tb_in[3] = {a.tb[(size_t)b * 3], a.tb[(size_t)b * 3 + 1], a.tb[(size_t)b * 3 + 2]};
  fa_align_reduce(s, red, tot);  // (its barriers lie between every thread's read of tb above and the write below)
  double q[3];
  for (int c = 0; c < 3; ++c) {
    const double tbar = (double)tb_in[c] + tot[c];
    q[c] = tbar / tot[3];
    if (tid == c) a.tb[(size_t)b * 3 + c] = (float)tbar;
  }
  for (int i = tid; i < V; i += 256) {
    const size_t e = (size_t)b * V + i;
    float g[3];
    const float wb = sf::align_point_adjoint(a.in.ctv + e * 3, a.mesh + e * 3, a.in.vw ? a.in.vw[e] : 1.f, q, g);
    for (int c = 0; c < 3; ++c) {
      a.acc_tv[e * 3 + c] += g[c];
      a.meshbar[e * 3 + c] -= g[c];
    }
    if (a.in.vw && a.acc_vw) a.acc_vw[e] += wb;
  }
  if (!a.in.ctj) return;
  for (int j = tid; j < J; j += 256) {
    const size_t e = (size_t)b * J + j;
    float g[3];
    const float wb = sf::align_point_adjoint(a.in.ctj + e * 3, a.joints + e * 3, a.in.jw ? a.in.jw[e] : 1.f, q, g);
    for (int c = 0; c < 3; ++c) {
      a.acc_tj[e * 3 + c] += g[c];
      a.jointsbar[e * 3 + c] -= g[c];
    }
    if (a.in.jw && a.acc_jw) a.acc_jw[e] += wb;
  }
}
