// Wave-per-instance kernels of libsmplfit_hip.so (one wave fits one instance; every configuration) and
// the posedirs GEMMs.  Included by smplfit_hip.hip INSIDE its anonymous namespace, after DevModel /
// Workspace / DevCtx — not a stand-alone header.
// ------------------------------------------------------------------------------------------------
// K0: centre + sort + template part sums.  grid B, block 256.
// reference: fit() centring bodyfitter.py:355-361; _part_sums :235-280 against default_mesh_tf.
// dynamic LDS: 4 waves x J x 16 floats + 20 (no static LDS: keeps the dynamic base 16-B aligned).
// ------------------------------------------------------------------------------------------------
// VW_SHARED: vw is ONE (V) row every instance reads (smplfit_replace_hands_f32), not (B, V)
template <bool WEIGHTED, bool VW_SHARED = false>
__global__ __launch_bounds__(256) void k_center_sort_partsum(DevModel m, const float* __restrict__ tv,
                                                             const float* __restrict__ tj,
                                                             const float* __restrict__ vw,
                                                             Workspace ws) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = m.V, J = m.J, Vp = m.Vp;
  float(*red)[4] = reinterpret_cast<float(*)[4]>(smem + 4 * J * sf::kPsum);  // [4][4]
  float* mu = smem + 4 * J * sf::kPsum + 16;                                // [4]
  const float* tvb = tv + (size_t)b * V * 3;
  // ---- mean over the V (+J) points
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int v = tid; v < V; v += 256) {
    sx += tvb[v * 3];
    sy += tvb[v * 3 + 1];
    sz += tvb[v * 3 + 2];
  }
  if (tj) {
    for (int j = tid; j < J; j += 256) {
      sx += tj[((size_t)b * J + j) * 3];
      sy += tj[((size_t)b * J + j) * 3 + 1];
      sz += tj[((size_t)b * J + j) * 3 + 2];
    }
  }
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  sz = wave_sum(sz);
  if (lane == 0) {
    red[wave][0] = sx;
    red[wave][1] = sy;
    red[wave][2] = sz;
  }
  for (int k = tid; k < 4 * J * sf::kPsum; k += 256) smem[k] = 0.f;
  __syncthreads();
  if (tid < 3) {
    const float n = (float)(V + (tj ? J : 0));
    const float s = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    mu[tid] = s / n;
    ws.mean[b * 3 + tid] = s / n;
  }
  __syncthreads();
  const float m0 = mu[0], m1 = mu[1], m2 = mu[2];
  if (tj)
    for (int k = tid; k < J * 3; k += 256)
      ws.tjc[(size_t)b * J * 3 + k] = tj[(size_t)b * J * 3 + k] - mu[k % 3];
  // ---- used parts: gather, centre, store sorted SoA, accumulate part sums per segment
  float* tvs = ws.tvs + (size_t)b * 3 * Vp;
  float* vws = ws.vws + (size_t)b * Vp;
  const int s_begin = (int)((long)m.nseg * wave / 4), s_end = (int)((long)m.nseg * (wave + 1) / 4);
  float acc[sf::kPsum];
#pragma unroll
  for (int k = 0; k < sf::kPsum; ++k) acc[k] = 0.f;
  for (int s = s_begin; s < s_end; ++s) {
    const int start = m.segments[s * 3], count = m.segments[s * 3 + 1], part = m.segments[s * 3 + 2];
    if (lane < count) {
      const int i = start + lane, o = m.perm[i];
      const float t[3] = {tvb[o * 3] - m0, tvb[o * 3 + 1] - m1, tvb[o * 3 + 2] - m2};
      st_stream<16>(tvs + i, t[0]);
      st_stream<16>(tvs + Vp + i, t[1]);
      st_stream<16>(tvs + 2 * Vp + i, t[2]);
      const float a[3] = {m.dm[i], m.dm[Vp + i], m.dm[2 * Vp + i]};
      float w = 1.f;
      if (WEIGHTED) {
        w = vw[(VW_SHARED ? (size_t)0 : (size_t)b * V) + o];
        vws[i] = w;
      }
      sf::partsum_vertex(t, a, w, WEIGHTED, acc);
    }
    const bool flush = (s + 1 == s_end) || (m.segments[(s + 1) * 3 + 2] != part);
    if (flush) {
#pragma unroll
      for (int k = 0; k < sf::kPsum; ++k) {
        const float r = wave_sum(acc[k]);
        if (lane == 0) smem[(wave * J + part) * sf::kPsum + k] = r;
        acc[k] = 0.f;
      }
    }
  }
  // ---- the remaining (unused-part and padding) slots: store only
  for (int i = m.n_used + tid; i < Vp; i += 256) {
    const int o = m.perm[i];
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, w = 0.f;
    if (o >= 0) {
      t0 = tvb[o * 3] - m0;
      t1 = tvb[o * 3 + 1] - m1;
      t2 = tvb[o * 3 + 2] - m2;
      if (WEIGHTED) w = vw[(VW_SHARED ? (size_t)0 : (size_t)b * V) + o];
    }
    st_stream<16>(tvs + i, t0);
    st_stream<16>(tvs + Vp + i, t1);
    st_stream<16>(tvs + 2 * Vp + i, t2);
    if (WEIGHTED) vws[i] = w;
  }
  __syncthreads();
  for (int k = tid; k < J * sf::kPsum; k += 256)
    ws.psum[(size_t)b * J * sf::kPsum + k] =
        (smem[k] + smem[J * sf::kPsum + k]) + (smem[2 * J * sf::kPsum + k] + smem[3 * J * sf::kPsum + k]);
}

// ------------------------------------------------------------------------------------------------
// K0 (LDS-staged form): one 1024-thread workgroup per instance.  The instance's (V,3) target row is
// read from HBM exactly once, fully coalesced, into LDS (83 KB SMPL / 126 KB SMPL-X); the mean, the
// gather into part-sorted SoA order and the per-part sums against the template all run out of LDS.
// (Real SMPL vertex order is not part-sorted: gathering 12-byte vertices straight from global
// memory pulled ~8x the row through the fabric.)   part_seg_start: (J+1) first segment of each part.
// dynamic LDS: 3 VL floats + 64, VL = vertices staged in LDS.  For SMPL the whole row (82.7 KB) would
// allow one workgroup per CU only; staging the first VL = 6784 vertices (80 KB) and reading the last
// 1.5 % of the row from L2 in the gather lets TWO workgroups share a CU, so one loads while the other
// gathers / sums.
// ------------------------------------------------------------------------------------------------
template <bool WEIGHTED, bool VW_SHARED = false>
__global__ __launch_bounds__(1024) void k_center_sort_partsum_lds(DevModel m, const float* __restrict__ tv,
                                                                 const float* __restrict__ tj,
                                                                 const float* __restrict__ vw,
                                                                 Workspace ws, int VL) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = m.V, J = m.J, Vp = m.Vp, n3 = 3 * V, nl = 3 * VL;
  float* raw = smem;                       // [3 VL]
  float* red = smem + ((nl + 3) & ~3);     // [16][3] + mu[3]
  const float* tvb = tv + (size_t)b * n3;
  auto at = [&](int k) { return k < nl ? raw[k] : tvb[k]; };  // element k of the row
  // ---- coalesced row load (rows are 8-byte aligned: 3V*4 is a multiple of 8 when V is even)
  // (the requests of a batch of 8 iterations are issued before the first LDS store: a guarded
  // load-store loop runs its iterations one memory latency after the other)
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  constexpr int U = 8;
  if ((n3 & 1) == 0) {
    const float2* src = reinterpret_cast<const float2*>(tvb);
    float2* dst = reinterpret_cast<float2*>(raw);
    const int nk = n3 / 2;
    for (int base = tid; base < nk; base += 1024 * U) {
      float2 xs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = base + 1024 * u;
        xs[u] = k < nk ? src[k] : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = base + 1024 * u;
        if (k < nk) {
          const float2 x = xs[u];
          if (2 * k + 1 < nl) dst[k] = x;  // nl is even here (VL even or VL == V)
          const int r = (2 * k) % 3;  // coordinate of x.x; x.y is (r+1)%3
          s0 += (r == 0 ? x.x : 0.f) + (r == 2 ? x.y : 0.f);
          s1 += (r == 1 ? x.x : 0.f) + (r == 0 ? x.y : 0.f);
          s2 += (r == 2 ? x.x : 0.f) + (r == 1 ? x.y : 0.f);
        }
      }
    }
  } else {
    for (int base = tid; base < n3; base += 1024 * U) {
      float xs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = base + 1024 * u;
        xs[u] = k < n3 ? tvb[k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = base + 1024 * u;
        if (k < n3) {
          const float x = xs[u];
          if (k < nl) raw[k] = x;
          const int r = k % 3;
          s0 += r == 0 ? x : 0.f;
          s1 += r == 1 ? x : 0.f;
          s2 += r == 2 ? x : 0.f;
        }
      }
    }
  }
  if (tj) {
    for (int j = tid; j < J; j += 1024) {
      s0 += tj[((size_t)b * J + j) * 3];
      s1 += tj[((size_t)b * J + j) * 3 + 1];
      s2 += tj[((size_t)b * J + j) * 3 + 2];
    }
  }
  s0 = wave_sum_last(s0);
  s1 = wave_sum_last(s1);
  s2 = wave_sum_last(s2);
  if (lane == 63) {
    red[wave * 3] = s0;
    red[wave * 3 + 1] = s1;
    red[wave * 3 + 2] = s2;
  }
  __syncthreads();
  if (tid < 3) {
    float s = 0.f;
    for (int w = 0; w < 16; ++w) s += red[w * 3 + tid];
    const float mean = s / (float)(V + (tj ? J : 0));
    red[48 + tid] = mean;
    ws.mean[b * 3 + tid] = mean;
  }
  __syncthreads();
  const float m0 = red[48], m1 = red[49], m2 = red[50];
  if (tj)
    for (int k = tid; k < J * 3; k += 1024)
      ws.tjc[(size_t)b * J * 3 + k] = tj[(size_t)b * J * 3 + k] - red[48 + k % 3];
  // ---- gather from LDS into sorted SoA order, coalesced stores
  float* tvs = ws.tvs + (size_t)b * 3 * Vp;
  float* vws = ws.vws + (size_t)b * Vp;
  for (int base = tid; base < Vp; base += 1024 * U) {  // the permutation entries of a batch first
    int os[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + 1024 * u;
      os[u] = i < Vp ? m.perm[i] : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + 1024 * u;
      if (i >= Vp) continue;
      const int o = os[u];
      float t0 = 0.f, t1 = 0.f, t2 = 0.f, w = 0.f;
      if (o >= 0) {
        t0 = at(o * 3) - m0;
        t1 = at(o * 3 + 1) - m1;
        t2 = at(o * 3 + 2) - m2;
        if (WEIGHTED) w = vw[(VW_SHARED ? (size_t)0 : (size_t)b * V) + o];
      }
      st_stream<16>(tvs + i, t0);
      st_stream<16>(tvs + Vp + i, t1);
      st_stream<16>(tvs + 2 * Vp + i, t2);
      if (WEIGHTED) vws[i] = w;
    }
  }
  // ---- per-part sums against the template: one wave per part
  for (int p = wave; p < J; p += 16) {
    const int s_begin = m.part_seg_start[p], s_end = m.part_seg_start[p + 1];
    float* ps = ws.psum + ((size_t)b * J + p) * sf::kPsum;
    float acc[sf::kPsum];
#pragma unroll
    for (int k = 0; k < sf::kPsum; ++k) acc[k] = 0.f;
    // table reads unguarded (clamped lane) so that the partial unroll can issue them together
#pragma unroll 4
    for (int s = s_begin; s < s_end; ++s) {
      const int start = m.segments[s * 3], count = m.segments[s * 3 + 1];
      const int i = start + (lane < count ? lane : 0), o = m.perm[i];
      const float a[3] = {m.dm[i], m.dm[Vp + i], m.dm[2 * Vp + i]};
      if (lane < count) {
        const float t[3] = {at(o * 3) - m0, at(o * 3 + 1) - m1, at(o * 3 + 2) - m2};
        sf::partsum_vertex(t, a, WEIGHTED ? vw[(VW_SHARED ? (size_t)0 : (size_t)b * V) + o] : 1.f, WEIGHTED, acc);
      }
    }
#pragma unroll
    for (int k = 0; k < sf::kPsum; ++k) {
      const float r = wave_sum_last(acc[k]);
      if (lane == 63) ps[k] = r;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// sparse post-LBS joint regression (joints-omitted path): out[b][j] = sum_k reg_val * src[b][:, slot]
// reference: bodyfitter.py:1342-1344.  grid B, block 64.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_regress_joints(DevModel m, const float* __restrict__ src,
                                                       float* __restrict__ out) {
  const int b = blockIdx.x;
  const float* s = src + (size_t)b * 3 * m.Vp;
  for (int j = threadIdx.x; j < m.J; j += 64) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = m.reg_start[j]; k < m.reg_start[j + 1]; ++k) {
      const int i = m.reg_slot[k];
      const float r = m.reg_val[k];
      a0 += r * s[i];
      a1 += r * s[m.Vp + i];
      a2 += r * s[2 * m.Vp + i];
    }
    out[((size_t)b * m.J + j) * 3] = a0;
    out[((size_t)b * m.J + j) * 3 + 1] = a1;
    out[((size_t)b * m.J + j) * 3 + 2] = a2;
  }
}

// ------------------------------------------------------------------------------------------------
// K1: joint stage.  grid B, block 64.  dynamic LDS = joint_scratch_floats.
// ------------------------------------------------------------------------------------------------
// The LDS scratch of a joint-level stage; on the GENERAL path (DevModel::general: any number of shape unknowns) the
// S-sized arrays P and T of kind 0 live in the workspace (ws.pext — which the stage writes anyway — and ws.gT) and only
// the J-sized ones in LDS.
// GEN is a TEMPLATE parameter of the stage kernels, not a run-time branch: with one pointer that may be LDS or global the
// compiler addresses the whole scratch through FLAT instructions (measured: the solve 26 -> 39 us, c4 7.4 -> 6.9 M fits/s).
template <bool GEN>
__device__ __forceinline__ sf::JointScratch gen_joint_scratch(const DevModel& m, const Workspace& ws, float* lds, int b, int kind) {
  if constexpr (!GEN) return sf::carve_joint_scratch(lds, m.J, m.S, kind);
  sf::JointScratch sh = sf::carve_joint_scratch(lds, m.J, 0, kind);
  if (kind == 0) {
    sh.P = ws.pext + (size_t)b * m.J * 3 * (m.S + 1);
    sh.T = ws.gT + (size_t)b * m.J * 3 * (m.S + 1);
  }
  return sh;
}

struct JointStageArgs {
  const float* tj;       // (B,J,3) centred target joints (given or regressed)
  const float* rj;       // (B,J,3) reference joints, or (J,3) template when rj_shared
  int rj_shared;
  const float* Gprev;    // (B,J,9) or null
  const float* jw;       // (B,J) or null
  int fit_rotations, do_prologue, joint_block, joint_block_weighted, vertex_sa_closed_form;
  int B;
  int b0;  // first instance of the launch (the odd last instance of a two-per-wave batch is a launch of its own)
  int gt_pitch;  // > 0: also write the instance-innermost copy ws.GT (row pitch = Mp) — k_prologue_bm follows
};

// N = 64: one instance per wave; N = 32: two (DevCtxHalf; the launch covers an EVEN number of instances — the last one
// of an odd batch gets a one-instance launch of the N = 64 form, so no two halves ever write the same rows)
// SMPLFIT_JOINT_OCC: waves per SIMD the one-instance form is compiled for.  3 (168 registers, no scratch) since round 5:
// measured on the SMPL-X-shaped model at B = 4096 (profiles/r05_ab_joint_occ.txt) 123 -> 99 us per launch against 4 (128
// registers, 100 B of scratch per lane with 55 joints) and 102 us for 2; identical results; 1.277 -> 1.308 M fits/s
#ifndef SMPLFIT_JOINT_OCC
#define SMPLFIT_JOINT_OCC 3
#endif
template <int N, bool GEN = false>
__global__ __launch_bounds__(64, N == 64 ? SMPLFIT_JOINT_OCC : 2) void k_joint_stage(DevModel m, JointStageArgs a, Workspace ws) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int half = (int)threadIdx.x / N, J = m.J, S = m.S;
  const int b = min(a.b0 + (int)blockIdx.x * (64 / N) + half, a.B - 1);
  typename StageCtx<N>::type cx{(int)threadIdx.x % N, N};
  sf::JointScratch sh = gen_joint_scratch<GEN>(m, ws, smem + half * sf::joint_scratch_floats(J, S, 0), b, 0);
  const int NE1 = sf::ne_size(S) + 1;
  sf::joint_stage(cx, m.jt, sh, ws.psum + (size_t)b * J * sf::kPsum, a.tj + (size_t)b * J * 3,
                  a.rj_shared ? a.rj : a.rj + (size_t)b * J * 3,
                  a.Gprev ? a.Gprev + (size_t)b * J * 9 : nullptr,
                  a.jw ? a.jw + (size_t)b * J : nullptr, a.fit_rotations != 0, a.do_prologue != 0,
                  a.joint_block != 0,
                  a.joint_block_weighted != 0, a.vertex_sa_closed_form != 0, ws.G + (size_t)b * J * 9,
                  ws.rp + (size_t)b * m.Kp, ws.jd + (size_t)b * J * sf::jd_stride(S),
                  ws.pext + (size_t)b * J * 3 * (S + 1), ws.gramj + (size_t)b * NE1,
                  a.gt_pitch > 0 ? ws.GT + b : nullptr, a.gt_pitch);
}

// ------------------------------------------------------------------------------------------------
// K2: v_posed[Mp][N] = A[Mp][Kp] . Bm[Kp][N]   (fp32 MFMA 32x32x2, exact f32)
// reference: bodyfitter.py:913-916 v_template + einsum('vcp,bp->bvc').  N = 3*Vp, column n = c*Vp + slot.
// The template needs no bias operand: pose feature P is the constant 1 and row P of Bm holds
// v_template (sf_tables.cpp), so it is added by the MFMA chain itself.
// 128x128 block tile, 4 waves x (64x64), K step 16, register-prefetched double-buffered LDS.
// grid = (N/128) * (Mp/128), n-tile major so the blocks of one posedirs column tile run together.
// ------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <bool TRANSPOSED>
__global__ __launch_bounds__(256, 2) void k_posedirs_gemm(const float* __restrict__ A,
                                                          const float* __restrict__ Bt,
                                                          float* __restrict__ C, int Mp, int N, int Kp) {
  // Both operand tiles are staged k-innermost: As[m][k], Bs[n][k], rows of 16 + 4 floats (80 B: the 16
  // lanes of a ds_read_b128 group land on 16 distinct 16-byte slots).  Within a 16-deep K step the two
  // lane halves of the 32x32x2 MFMA contract storage columns kk and 8 + kk (any pairing of the K axis is
  // valid as long as A and B agree), so a lane reads its 8 values per operand row as two 16-byte reads.
  // Bt = posedirs transposed, (N, Kp) row-major (HostTables::pdSw).
  constexpr int RS = 20;
  __shared__ __attribute__((aligned(16))) float As[2][128 * RS];
  __shared__ __attribute__((aligned(16))) float Bs[2][128 * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mtiles = Mp / 128;
  const int ntile = blockIdx.x / mtiles, mtile = blockIdx.x % mtiles;
  const int m0 = mtile * 128, n0 = ntile * 128;
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
  const int l31 = lane & 31, lk = lane >> 5;

  f32x16 acc[2][2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
  // global -> register staging: 128 rows x 16 k per operand = 2 float4 per thread each
  const int s_row = tid >> 2, s_kc = (tid & 3) * 4;
  // named registers: an indexed array captured by the staging lambdas ends up in scratch
  float4 ra0, ra1, rb0, rb1;
  const float* ag = A + (size_t)(m0 + s_row) * Kp + s_kc;
  const float* bg = Bt + (size_t)(n0 + s_row) * Kp + s_kc;
  auto gload = [&](int k0) {
    ra0 = *reinterpret_cast<const float4*>(ag + k0);
    ra1 = *reinterpret_cast<const float4*>(ag + (size_t)64 * Kp + k0);
    rb0 = *reinterpret_cast<const float4*>(bg + k0);
    rb1 = *reinterpret_cast<const float4*>(bg + (size_t)64 * Kp + k0);
  };
  auto sstore = [&](int buf) {
    *reinterpret_cast<float4*>(&As[buf][s_row * RS + s_kc]) = ra0;
    *reinterpret_cast<float4*>(&As[buf][(s_row + 64) * RS + s_kc]) = ra1;
    *reinterpret_cast<float4*>(&Bs[buf][s_row * RS + s_kc]) = rb0;
    *reinterpret_cast<float4*>(&Bs[buf][(s_row + 64) * RS + s_kc]) = rb1;
  };
  const int nk = Kp / 16;
  gload(0);
  sstore(0);
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    const int buf = it & 1;
    if (it + 1 < nk) gload((it + 1) * 16);
    const float4* ap0 = reinterpret_cast<const float4*>(&As[buf][(wm + l31) * RS + lk * 8]);
    const float4* ap1 = reinterpret_cast<const float4*>(&As[buf][(wm + 32 + l31) * RS + lk * 8]);
    const float4* bp0 = reinterpret_cast<const float4*>(&Bs[buf][(wn + l31) * RS + lk * 8]);
    const float4* bp1 = reinterpret_cast<const float4*>(&Bs[buf][(wn + 32 + l31) * RS + lk * 8]);
    // all eight fragment reads of the step first: the second half lands behind the first 16 MFMAs
    const float4 a0l = ap0[0], a1l = ap1[0], b0l = bp0[0], b1l = bp1[0];
    const float4 a0h = ap0[1], a1h = ap1[1], b0h = bp0[1], b1h = bp1[1];
    auto mfma4 = [&](float a0, float a1, float b0, float b1) {
      if (TRANSPOSED) {  // operands swapped: instances become the columns of the result tile
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, a0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, a0, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, a1, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, a1, acc[1][1], 0, 0, 0);
      } else {
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    };
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
    mfma4(a0l.x, a1l.x, b0l.x, b1l.x);
    mfma4(a0l.y, a1l.y, b0l.y, b1l.y);
    mfma4(a0l.z, a1l.z, b0l.z, b1l.z);
    mfma4(a0l.w, a1l.w, b0l.w, b1l.w);
    mfma4(a0h.x, a1h.x, b0h.x, b1h.x);
    mfma4(a0h.y, a1h.y, b0h.y, b1h.y);
    mfma4(a0h.z, a1h.z, b0h.z, b1h.z);
    mfma4(a0h.w, a1h.w, b0h.w, b1h.w);
    if (it + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }
  // C layout of 32x32: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (TRANSPOSED) {  // batch-major: [instance / 64][n][64]
          const int inst = m0 + wm + mi * 32 + l31;
          const int n = n0 + wn + ni * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          st_stream<2>(C + ((size_t)(inst >> 6) * N + n) * 64 + (inst & 63), acc[mi][ni][r]);
        } else {
          const int row = m0 + wm + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          const int col = n0 + wn + ni * 32 + l31;
          st_stream<2>(C + (size_t)row * N + col, acc[mi][ni][r]);
        }
      }
}

constexpr int kNW = 4;  // instances (= waves) per workgroup in the vertex kernels

// ------------------------------------------------------------------------------------------------
// K2, A-stationary form (Kp <= 256): each wave keeps its 32 instances' whole pose-feature rows in
// NK2 = Kp/2 VGPRs (lane = (instance, k parity), the 32x32x2 A operand) and streams 32-column tiles
// of posedirs through a double-buffered LDS tile shared by the 4 waves (128 instances) of the
// workgroup.  Per tile a wave issues NK2 back-to-back MFMAs on one accumulator (issue interval =
// dependent latency = 64 cycles), fed by 16-byte LDS reads that run one group of four MFMAs ahead
// (two register quads used alternately: with one quad every group waited for its own LDS round trip).
// Nothing the MFMA chain needs comes from global memory (no bias operand, see above), so the
// prefetch of the next tile stays in flight until the LDS stores at the end of the tile.
// Bsw: (N/32, 32, Kp) pre-transposed tiles.
// grid = (nchunk, Mp/128); workgroup y handles instances [128y, 128y+128), chunk x a run of tiles.
// ------------------------------------------------------------------------------------------------
// TRANSPOSED: the MFMA operands swap roles (instances become the columns of the 32x32 result) and the
// output is written instance-innermost, C[n][Mp] — the layout of the batch-major vertex kernels.
template <int NK2, bool TRANSPOSED>
__global__ __launch_bounds__(256, 2) void k_posedirs_gemm_as(const float* __restrict__ A,
                                                          const float* __restrict__ Bsw,
                                                          float* __restrict__ C, int N,
                                                          int tiles_per_chunk, int Mp) {
  constexpr int KP = 2 * NK2, RS = KP + 4;  // LDS row stride: +4 floats keeps 16 lanes on 16 slots
  constexpr int TILE_F4 = 32 * KP / 4;      // float4 per tile in global memory
  constexpr int NQ = NK2 / 4;               // groups of four MFMAs (one 16-byte LDS read each)
  static_assert(NQ % 2 == 0, "the fragment reads alternate between two register quads");
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][32][RS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lk = lane >> 5;
  const int m0 = (blockIdx.y * 4 + wave) * 32;
  const int ntiles = N / 32;
  const int t_begin = blockIdx.x * tiles_per_chunk;
  const int t_end = min(t_begin + tiles_per_chunk, ntiles);
  // A fragment: this lane's instance row, its k parity (contiguous thanks to rp_pos)
  float a[NK2];
  {
    const float4* src = reinterpret_cast<const float4*>(A + (size_t)(m0 + l31) * KP + lk * NK2);
#pragma unroll
    for (int q = 0; q < NK2 / 4; ++q) {
      const float4 v = src[q];
      a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
  }
  // global -> register -> LDS staging of the next tile, in named registers (an indexed array would
  // live in scratch); TILE_F4 <= 7 * 256
  static_assert(TILE_F4 <= 7 * 256, "tile too large for the staging registers");
  float4 s0, s1, s2, s3, s4, s5, s6;
#define SF_STAGE_ALL(OP) OP(0, s0) OP(1, s1) OP(2, s2) OP(3, s3) OP(4, s4) OP(5, s5) OP(6, s6)
  auto gload = [&](int tile) {
    const float4* src = reinterpret_cast<const float4*>(Bsw) + (size_t)tile * TILE_F4;
#define SF_LD(q, r)                                                       \
  if constexpr (256 * (q + 1) <= TILE_F4) r = src[tid + 256 * q];         \
  else if (tid + 256 * q < TILE_F4) r = src[tid + 256 * q];
    SF_STAGE_ALL(SF_LD)
#undef SF_LD
  };
  auto sstore = [&](int buf) {
    float* base = smem + (size_t)buf * 32 * RS;
#define SF_ST(q, r)                                                                        \
  if (256 * (q + 1) <= TILE_F4 || tid + 256 * q < TILE_F4) {                               \
    const int f = tid + 256 * q;                                                           \
    *reinterpret_cast<float4*>(base + (f / (KP / 4)) * RS + 4 * (f % (KP / 4))) = r;      \
  }
    SF_STAGE_ALL(SF_ST)
#undef SF_ST
  };
#undef SF_STAGE_ALL
  if (t_begin >= t_end) return;
  gload(t_begin);
  sstore(0);
  __syncthreads();
  for (int t = t_begin; t < t_end; ++t) {
    const int buf = (t - t_begin) & 1;
    if (t + 1 < t_end) gload(t + 1);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float4* brow = reinterpret_cast<const float4*>(smem + (size_t)buf * 32 * RS + l31 * RS + lk * NK2);
    auto mfma4 = [&](const float4& bq, int q) {
      if (TRANSPOSED) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bq.x, a[4 * q], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bq.y, a[4 * q + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bq.z, a[4 * q + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bq.w, a[4 * q + 3], acc, 0, 0, 0);
      } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q], bq.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q + 1], bq.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q + 2], bq.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q + 3], bq.w, acc, 0, 0, 0);
      }
    };
    // C layout of 32x32: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    float4 bA = brow[0], bB;
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
    for (int q = 0; q < NQ; q += 2) {
      bB = brow[q + 1];
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // the read of the NEXT group first,
      mfma4(bA, q);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);  // then this group's four MFMAs
      if (q + 2 < NQ) bA = brow[q + 2];
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      mfma4(bB, q + 1);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    if (TRANSPOSED) {  // batch-major: [m0 / 64][n][64]; 32 consecutive instances per half wave
      float* ccol = C + ((size_t)(m0 >> 6) * N + t * 32) * 64 + (m0 & 63) + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        st_stream<2>(ccol + (size_t)((r & 3) + 8 * (r >> 2) + 4 * lk) * 64, acc[r]);
    } else {
      float* crow = C + (size_t)m0 * N + t * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        st_stream<2>(crow + (size_t)((r & 3) + 8 * (r >> 2) + 4 * lk) * N, acc[r]);
    }
    if (t + 1 < t_end) sstore(buf ^ 1);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// K2 on the bf16 matrix cores, fp32-class at the vertex level: split-bf16 form of the A-stationary kernel (Kp == 208).
// On gfx950 the fp32 MFMA executes on the vector ALUs (measured: an fp32-MFMA chain and independent
// v_fma_f32 work add up, in one wave and across the waves of a SIMD, tools/ubench), so the fp32 form of
// this GEMM takes the VALU away from every vertex pass that could run beside it.  The bf16 MFMA is 16x
// faster and runs on the matrix core next to VALU work.  Every fp32 operand x is split error-free into
// bf16 terms x = x1 + x2 + x3 (x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2): 3 x 8 mantissa bits) and
// the product a.b is accumulated in fp32 from partial products, each exact in fp32: with kGemm3 (default) a1b1,
// a1b2, a2b1 (what is dropped is 2^-18 of |a||b|, on rows whose sum is a centimetre-sized pose-corrective offset) plus
// a1b3 in the k-step of the bias row (feature 1 x v_template: exact to 2^-27); with six products every term of
// order <= 2^-16 (the dropped ones <= 2^-24 relative).  Both are checked against the fp64 oracle next to the
// fp32-MFMA form in tests/test_gpu_evidence.py::test_gemm_split_precision.
// A wave keeps its 32 instances' features as 2 (3) x 13 bf16x8 fragments (104 / 156 VGPRs; lane = (instance,
// k-octet)), streams the split posedirs tile images (HostTables::pdB, 27 / 39 KB per 32 columns) through a
// double-buffered LDS ring filled by LDS-DMA (no staging registers) and issues 40 / 78 MFMAs per tile.
// grid = (nchunk, ny), block 64 x kGemmWaves (8 waves x 32 instances), dynamic LDS 2 x kGemmTileBytes.
// ------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int kGemmKS = 13;                           // k-steps of 16
constexpr int kGemmPlaneBytes = 32 * 208 * 2;         // one plane of a tile: 32 rows x 416 B
constexpr int kGemmTileBytes = sf::kGemm3 ? 2 * kGemmPlaneBytes + 32 * 32 : 3 * kGemmPlaneBytes;  // 27648 (39936)
#ifndef SMPLFIT_GEMM_WAVES
#define SMPLFIT_GEMM_WAVES 8
#endif
constexpr int kGemmWaves = SMPLFIT_GEMM_WAVES;        // waves per workgroup (32 instances each)
#ifndef SMPLFIT_GEMM_RING
#define SMPLFIT_GEMM_RING 2
#endif
// LDS ring of tile images (kGemmRing - 1 tiles requested ahead).  Measured at 4096 (SMPL): 2 / 3 / 4 slots 102 / 102 /
// 105 us -- the tile request is not what the kernel waits for: timing-only ablation builds (wrong results; since
// removed, numbers in profiles/README.md, rounds 2 and 3) of the three-product form give 83 without the output stores,
// 99 without the LDS-DMA, 96 without the fragment reads, 68.5 with none of the three (3.3 M MFMAs = 52 us of
// matrix-pipe time at 2.0 GHz + the feature prologue of the 512 workgroups); the six-product form gave 158 us -> 141 /
// 133 / 161, all three 122 us.
constexpr int kGemmRing = SMPLFIT_GEMM_RING;
static_assert(kGemmRing >= 2 && 16 * (kGemmRing - 1) + (kGemmRing - 2) * (kGemmTileBytes / 1024 / kGemmWaves + 1) <= 63,
              "s_waitcnt vmcnt is a 6-bit count");
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// Products per k-step of the split-bf16 GEMMs (sf::kGemm3, -DSMPLFIT_GEMM_PRODUCTS).  6: every term down to 2^-24 of
// |feature| |posedirs| (fp32-equivalent on every term).  3 (default): x1 y1 + x1 y2 + x2 y1 — the terms of order 2^-18
// are dropped on the POSE-CORRECTIVE rows only, whose sum is a vertex offset of at most a few centimetres: 2^-18 of that
// is below the 6e-8 m rounding of an fp32 coordinate at 1 m — while the k-step holding the bias row (feature = 1,
// posedirs row = v_template, order 1 m) also gets x1 y3, which makes the template exact to 2^-27.  Measured forward
// error against fp64 (test_gemm_split_precision): 5.7e-7 / 6.1e-7 m (poses of 0.1 / 1 rad) against 4.7e-7 / 5.5e-7 for
// the fp32 MFMA and 5.3e-7 for six products; the GEMM takes 106 instead of 159 us (SMPL), 523 instead of 657 (SMPL-X).
constexpr bool kGemm3 = sf::kGemm3;

// LDS-DMA of 64 x 16 B (lane l: src + lane_off -> lds + 16 l; src, lds wave-uniform) as inline assembly: the compiler
// models the builtin as a FLAT access of LDS, and a pending FLAT access turns every later s_waitcnt lgkmcnt(n) into
// lgkmcnt(0) -- the MFMAs of a k-step would wait for the fragment reads issued to overlap them.  The caller orders it
// (s_waitcnt vmcnt + barrier).
__device__ __forceinline__ void lds_dma16(const char* src, uint32_t lane_off, char* lds) {
  const uint32_t l = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(l), "v"(lane_off), "s"(src) : "memory", "m0");
}

// EXCLUSIVE CU.  Measured on MI355X (DESIGN.md §8 item 3, profiles/README.md): while a wave streams LDS
// fragments into bf16 MFMAs, OTHER kernels' waves resident on the same CU occasionally receive a wrong
// last quarter (lanes 48-63) of a broadcast-type read (uniform-address LDS / vector loads) — k_pair_gram_bm
// and k_lbs_partsum_bm beside this kernel produced run-to-run different sums; neither the fp32-MFMA GEMM
// nor this kernel without its LDS reads or without its MFMAs did that, and this kernel's own results are
// unaffected.  The kernel therefore never shares a CU with another kernel: every wave allocates 256 VGPRs,
// so the 8 waves of two of its workgroups (or of one 8-wave workgroup) own the whole register file of the
// CU and no other wave — of this fit's other chunk or of any other stream of the process — can become
// resident next to them.
//
// FRONT END.  PLANES = false: the wave loads its instances' fp32 feature rows (A: ws.rp) and splits them itself -- 26
// float4 requests per lane that use 32 bytes of every 832-byte row, and 104 three-way splits, repeated by each of the
// nchunk workgroups of an instance block.  PLANES = true: the producer of the features has written the split planes in
// fragment order INSTEAD of the fp32 rows (Apl: ws.rpP, sf::plane_off) and the wave fills f1 / f2 / f3[KS - 1] with 27
// requests of one contiguous 1 KB run each, no arithmetic (Route::gemm_planes: where k_prologue_bm made the features).
// The planes hold the bits the split below produces (sf::split_bf16x3 on both sides), and from the first barrier on
// the kernel is the same code: the results are bit-identical (tests/test_gpu_gemm_planes.py).
template <bool TRANSPOSED, bool PLANES>
__global__ __launch_bounds__(64 * kGemmWaves, 2) void k_posedirs_gemm_bf16x3(const float* __restrict__ A,
                                                                           const uint16_t* __restrict__ Apl,
                                                                           const uint16_t* __restrict__ Bimg,
                                                                           float* __restrict__ C, int N,
                                                                           int tiles_per_chunk, int Mp) {
  static_assert(!PLANES || (kGemm3 && kGemmKS == sf::kPlaneSteps), "the planes are those of the three-product form");
  constexpr int KS = kGemmKS, KP = 16 * KS, NW = kGemmWaves;
  constexpr int NDMA = kGemmTileBytes / 1024;  // 1 KB per wave-instruction: 39
  extern __shared__ __attribute__((aligned(16))) char smem_b[];  // [kGemmRing][kGemmTileBytes]
  asm volatile("v_mov_b32 v255, 0" ::: "v255");  // 256 VGPRs per wave: see "exclusive CU" above
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kg = lane >> 5;
  const int m0 = (blockIdx.y * NW + wave) * 32;
  const bool active = m0 < Mp;  // Mp is a multiple of 128; the last workgroup may hold idle waves
  const int ntiles = N / 32;
  const int t_begin = blockIdx.x * tiles_per_chunk;
  const int t_end = min(t_begin + tiles_per_chunk, ntiles);
  if (t_begin >= t_end) return;
  // tile t -> LDS buffer: every wave copies its 1 KB chunks (chunk c = wave + NW i) by LDS-DMA
  auto dma_tile = [&](int tile, int buf) {
    const char* src = reinterpret_cast<const char*>(Bimg) + (size_t)tile * kGemmTileBytes;
    char* dst = smem_b + buf * kGemmTileBytes;
#pragma unroll
    for (int i = 0; i < NDMA / NW; ++i) {
      const int c = wave + NW * i;
      lds_dma16(src + c * 1024, lane * 16, dst + c * 1024);
    }
    if (wave < NDMA % NW) {
      const int c = wave + NW * (NDMA / NW);
      lds_dma16(src + c * 1024, lane * 16, dst + c * 1024);
    }
  };
  // the ring holds kGemmRing - 1 tiles ahead of the one being multiplied.  Past the last tile the request is clamped to
  // it (constant counts in the waits below; nothing reads the copy).
  constexpr int LEAD = kGemmRing - 1;
#pragma unroll
  for (int q = 0; q < LEAD; ++q) dma_tile(min(t_begin + q, t_end - 1), q);
  // features of this lane's instance, its k-octet of every k-step, split into three bf16 planes
  bf16x8 f1[KS], f2[KS], f3[KS];
  if constexpr (PLANES) {
    // (lane = 32 kg + l31 is the lane order of a run; f3 of the other k-steps is never read, see the products below)
    const char* src = reinterpret_cast<const char*>(Apl) + (size_t)((active ? m0 : 0) >> 5) * sf::kPlaneGroupBytes + lane * 16;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      f1[s] = *reinterpret_cast<const bf16x8*>(src + (2 * s) * 1024);
      f2[s] = *reinterpret_cast<const bf16x8*>(src + (2 * s + 1) * 1024);
    }
    f3[KS - 1] = *reinterpret_cast<const bf16x8*>(src + (sf::kPlaneRuns - 1) * 1024);
  } else {
    const float* src = A + (size_t)((active ? m0 : 0) + l31) * KP + kg * 8;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const float4 lo = *reinterpret_cast<const float4*>(src + 16 * s);
      const float4 hi = *reinterpret_cast<const float4*>(src + 16 * s + 4);
      const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const sf::Bf16x3 t = sf::split_bf16x3(x[j]);
        f1[s][j] = t.h;
        f2[s][j] = t.m;
        f3[s][j] = t.l;
      }
    }
  }
  // this lane's fragment address inside a tile plane: row n = l31, 16-byte slot (2 s + kg) ^ ((n >> 3) & 1)
  const int frag_off = l31 * (KP * 2) + ((kg ^ ((l31 >> 3) & 1)) * 16);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the first tiles have landed (this wave's chunks)
  __builtin_amdgcn_s_barrier();
  const bool extra = wave < NDMA % NW;  // this wave copies NDMA / NW + 1 chunks of a tile
  int buf = 0, buf_req = LEAD;          // ring slots of tile t and of tile t + LEAD (the slot of t - 1: free since the barrier)
  for (int t = t_begin; t < t_end; ++t) {
    const bool more = t + 1 < t_end;
    dma_tile(min(t + LEAD, t_end - 1), buf_req);
    if (active) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const char* base = smem_b + buf * kGemmTileBytes + frag_off;
      auto frag = [&](int plane, int s) {
        if constexpr (kGemm3) {
          // third plane: the last k-step only, rows of 32 bytes (slot = this lane's k-octet)
          if (plane == 2) return *reinterpret_cast<const bf16x8*>(smem_b + buf * kGemmTileBytes + 2 * kGemmPlaneBytes + l31 * 32 + kg * 16);
        }
        return *reinterpret_cast<const bf16x8*>(base + plane * kGemmPlaneBytes + s * 32);
      };
      auto mm = [&](const bf16x8& p, const bf16x8& f) {
        if (TRANSPOSED) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p, f, acc, 0, 0, 0);
        else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f, p, acc, 0, 0, 0);
      };
      bf16x8 p1 = frag(0, 0), p2 = frag(1, 0), p3 = p1;
      if constexpr (!kGemm3) p3 = frag(2, 0);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        bf16x8 n1, n2, n3;
        if (s + 1 < KS) {  // the next step's fragments first: they land behind this step's MFMAs
          n1 = frag(0, s + 1);
          n2 = frag(1, s + 1);
          n3 = n1;
          if (!kGemm3 || s + 1 == KS - 1) n3 = frag(2, s + 1);  // (three products: the third plane for the bias step only)
        }
        if constexpr (kGemm3) {
          // the bias row (feature P = 1: v_template) sits at rp_pos(P) = KP - 1, in the last k-step
          if (s == KS - 1) mm(p3, f1[s]);
          mm(p2, f1[s]);  // small terms first
          mm(p1, f2[s]);
          mm(p1, f1[s]);
        } else {
          mm(p3, f1[s]);  // small terms first
          mm(p2, f2[s]);
          mm(p1, f3[s]);
          mm(p2, f1[s]);
          mm(p1, f2[s]);
          mm(p1, f1[s]);
        }
        if (s + 1 < KS) {
          p1 = n1;
          p2 = n2;
          p3 = n3;
        }
      }
      // C layout of 32x32: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
      if (TRANSPOSED) {  // batch-major: [m0 / 64][n][64]; 32 consecutive instances per half wave
        float* ccol = C + ((size_t)(m0 >> 6) * N + t * 32) * 64 + (m0 & 63) + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) st_stream<2>(ccol + (size_t)((r & 3) + 8 * (r >> 2) + 4 * kg) * 64, acc[r]);
      } else {
        float* crow = C + (size_t)m0 * N + t * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          st_stream<2>(crow + (size_t)((r & 3) + 8 * (r >> 2) + 4 * kg) * N, acc[r]);
      }
    }
    // the next tile's DMA chunks of this wave have landed once nothing older than what was issued after them is
    // outstanding (vmcnt counts loads and stores in issue order): the chunks of the LEAD - 1 tiles requested since and
    // the 16 stores of each of the LEAD tiles multiplied since (idle waves have no stores); then the workgroup meets:
    // every wave has finished reading this buffer and can see the next one.  The last tile drains everything: no
    // LDS-DMA may be in flight when the workgroup's LDS is released.
    constexpr int N0 = (LEAD - 1) * (NDMA / NW), N1 = (LEAD - 1) * (NDMA / NW + 1), ST = 16 * LEAD;
    if (!more) wait_vmcnt<0>();
    else if (active) {
      if (extra) wait_vmcnt<ST + N1>();
      else wait_vmcnt<ST + N0>();
    } else {
      if (extra) wait_vmcnt<N1>();
      else wait_vmcnt<N0>();
    }
    __builtin_amdgcn_s_barrier();
    buf_req = buf;
    buf = buf + 1 == kGemmRing ? 0 : buf + 1;
  }
}

// ------------------------------------------------------------------------------------------------
// K2 on the bf16 matrix cores for any K (SMPL-X: K = 487): the split-bf16 product (see k_posedirs_gemm_bf16x3)
// as an output-stationary tiled GEMM, three-product form.  Both operands come as stage images of bf16 planes: the
// posedirs images are built at create (HostTables::pdB2), the feature images of a call by k_split_features (the A
// operand does not fit registers here: 2 planes x 31 k-steps x 4 VGPRs).
// Workgroup = 8 waves, tile 256 instances x 256 columns; a wave owns 64 x 128 (2 x 4 MFMA blocks, 128 accumulator
// registers): per 16-k step it reads 12 fragments and issues 24 MFMAs.  K advances in stages of 32 (two k-steps):
// [features 2 x 256 x 64 B][posedirs half 0: 2 x 128 x 64 B][half 1][third planes of both halves, the bias row's
// stage only] = 80 KB, double-buffered by LDS-DMA = the whole 160 KB; the column halves are two consecutive 128-column
// stage images of HostTables::pdB2.  LDS rows are 64 bytes, 16-byte slots swizzled by (row >> 2) & 3: the lane groups
// of a ds_read_b128 hit 16 distinct bank quads.  Block ids are dealt so that an XCD keeps the same few instance tiles
// (their feature images stay in its L2) and walks the column tiles.  EXCLUSIVE CU as k_posedirs_gemm_bf16x3: 8 waves x
// 256 VGPRs and all of the LDS -- a form with two independent 4-wave workgroups per CU (16-k stages in a ring of three)
// is 6 % faster (335 us) but a CU holding ONE of them has room for other kernels' waves, i.e. for the neighbour
// interaction described above; it was measured and not kept.
// Software pipeline: the fragments of a k-step are read while the MFMAs of the k-step before run, the stage barrier sits
// between the two k-steps of a stage, and the LDS-DMA of the stage after the next is issued between the products of the
// second k-step (off the path from the barrier to the first MFMA).  Two findings shaped the code: hipcc models
// __builtin_amdgcn_global_load_lds as a FLAT access, and a pending FLAT access turns every later s_waitcnt lgkmcnt(n)
// into lgkmcnt(0) (lds_dma16 above); and any branch inside the k-loop lets the compiler sink the fragment reads below the
// MFMAs they are to overlap, so the stage of the bias row and the last one are peeled by template flags.
// Measured at 4096 x 31488 x 496 (12.2 M MFMAs = 191 us of matrix-pipe time at the 2.0 GHz the kernel runs at): 256 x 128
// tiles with 64 x 64 per wave: 448 us; 64 x 128 per wave: 375; + the pipeline: 357; see DESIGN.md section 4.
// Output: instance-innermost (batch-major).  grid = 8 * ceil(mt / 8) * (nt128 / 2), block 512, dynamic LDS 2 x kTg2Stage.
// ------------------------------------------------------------------------------------------------
constexpr int kTgPlanesA = sf::kGemm3 ? 2 : 3;  // feature planes a stage carries (three products: hi, mid)
constexpr int kTgStageA = kTgPlanesA * 256 * 64;  // bytes: planes of 256 rows x 32 k
constexpr int kTgStageB = 3 * 128 * 64;
constexpr int kTgStage = kTgStageA + kTgStageB;  // 73728

// feature images: grid (mt, kc32), block 256 (thread = instance row of the tile); rows >= Mrows read as zero
__global__ __launch_bounds__(256) void k_split_features(const float* __restrict__ A, uint16_t* __restrict__ img, int Mrows,
                                                        int Kp, int kc32) {
  const int mt = blockIdx.x, kc = blockIdx.y, r = threadIdx.x, row = mt * 256 + r;
  float x[32];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int k = kc * 32 + 4 * q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < Mrows && k + 3 < Kp) v = *reinterpret_cast<const float4*>(A + (size_t)row * Kp + k);
    else if (row < Mrows) {
      v.x = k < Kp ? A[(size_t)row * Kp + k] : 0.f;
      v.y = k + 1 < Kp ? A[(size_t)row * Kp + k + 1] : 0.f;
      v.z = k + 2 < Kp ? A[(size_t)row * Kp + k + 2] : 0.f;
    }
    x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
  }
  uint16_t* base = img + ((size_t)mt * kc32 + kc) * (kTgStageA / 2);
#pragma unroll
  for (int sl = 0; sl < 4; ++sl) {
    bf16x8 h, m, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const sf::Bf16x3 t = sf::split_bf16x3(x[sl * 8 + j]);
      h[j] = t.h; m[j] = t.m; l[j] = t.l;
    }
    const int ps = sl ^ ((r >> 2) & 3);
    uint16_t* d = base + (size_t)r * 32 + ps * 8;
    *reinterpret_cast<bf16x8*>(d) = h;
    *reinterpret_cast<bf16x8*>(d + 256 * 32) = m;
    if constexpr (kTgPlanesA == 3) *reinterpret_cast<bf16x8*>(d + 2 * 256 * 32) = l;
  }
}

constexpr int kTg2B = 2 * 128 * 64;                          // two planes of one 128-column half
constexpr int kTg2Bias = kTgStageA + 2 * kTg2B;              // offset of the third planes (8 KB per half)
constexpr int kTg2Stage = kTg2Bias + 2 * 128 * 64;           // 81920

__global__ __launch_bounds__(512, 1) void k_posedirs_gemm_bf16x3_tiled(const uint16_t* __restrict__ Aimg,
                                                                       const uint16_t* __restrict__ Bimg,
                                                                       float* __restrict__ C, int N, int Mp, int mt_count,
                                                                       int kc32, int bias_step) {
  static_assert(kGemm3 && kTgPlanesA == 2, "three-product form");
  extern __shared__ __attribute__((aligned(16))) char smem_b[];  // [2][kTg2Stage]
  asm volatile("v_mov_b32 v255, 0" ::: "v255");  // 256 VGPRs per wave: exclusive CU
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kg = lane >> 5;
  // block -> (instance tile, 256-column tile): XCD x = id % 8 keeps instance tiles {x, x + 8, ...}
  const int xcd = blockIdx.x & 7, rr = blockIdx.x >> 3, mt_per = (mt_count + 7) / 8;
  const int mtile = (rr % mt_per) * 8 + xcd, ntile = rr / mt_per;
  if (mtile >= mt_count) return;
  const int wm = wave & 3, wn = wave >> 2;  // the wave's 64 x 128 sub-tile
  const char* asrc = reinterpret_cast<const char*>(Aimg) + (size_t)mtile * kc32 * kTgStageA;
  const char* bsrc = reinterpret_cast<const char*>(Bimg) + (size_t)(2 * ntile) * kc32 * kTgStageB;
  const size_t bhalf = (size_t)kc32 * kTgStageB;  // distance of the second half's image
  // 64 pieces of 1 KB per stage (8 per wave): 32 of the features, 16 + 16 of the two posedirs halves (planes hi, mid);
  // the bias row's stage also gets the third planes (8 + 8 pieces: 2 per wave)
  auto dma_pieces = [&](int kc, int buf, int i0, int i1) {
    char* dst = smem_b + buf * kTg2Stage;
#pragma unroll
    for (int i = i0; i < i1; ++i) {
      const int c = wave + 8 * i;  // (wave-uniform; i < 4: features)
      const char* src = c < 32 ? asrc + (size_t)kc * kTgStageA + c * 1024
                               : bsrc + ((c - 32) >> 4) * bhalf + (size_t)kc * kTgStageB + ((c - 32) & 15) * 1024;
      lds_dma16(src, lane * 16, dst + c * 1024);
    }
    if (i1 == 8 && kc == bias_step / 2) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = wave + 8 * i;  // half e >> 3, piece e & 7 of its third plane
        lds_dma16(bsrc + (e >> 3) * bhalf + (size_t)kc * kTgStageB + kTg2B + (e & 7) * 1024, lane * 16, dst + kTg2Bias + e * 1024);
      }
    }
  };
  auto dma_stage = [&](int kc, int buf) { dma_pieces(kc, buf, 0, 8); };
  f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // fragment offsets inside a plane: row * 64 + ((2 s + kg) ^ ((row >> 2) & 3)) * 16, s = k-step of the stage (the
  // blocks of a wave are 32 rows = 2048 B apart, same swizzle; s = 1: the offset of s = 0 with bit 5 flipped)
  const int ra = wm * 64 + l31;
  const int aoff = ra * 64 + ((kg ^ ((ra >> 2) & 3)) * 16);
  const int boff = kTgStageA + wn * kTg2B + l31 * 64 + ((kg ^ ((l31 >> 2) & 3)) * 16);
  const int b3off = kTg2Bias + wn * (128 * 64) + l31 * 64 + ((kg ^ ((l31 >> 2) & 3)) * 16);
  struct Frags {
    bf16x8 a[2][2], b[4][2];  // [block][plane]
  };
  auto read_frags = [&](Frags& f, const char* base, int s2) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int i = 0; i < 2; ++i) f.a[i][p] = *reinterpret_cast<const bf16x8*>(base + (aoff ^ (s2 * 32)) + i * 2048 + p * (256 * 64));
#pragma unroll
      for (int j = 0; j < 4; ++j) f.b[j][p] = *reinterpret_cast<const bf16x8*>(base + (boff ^ (s2 * 32)) + j * 2048 + p * (128 * 64));
    }
  };
  auto mfma_step = [&](const Frags& f) {
#pragma unroll
    for (int i = 0; i < 2; ++i)      // instance block
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // column block; small terms first
        f32x16 a = acc[i][j];
        a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.b[j][1], f.a[i][0], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.b[j][0], f.a[i][1], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.b[j][0], f.a[i][0], a, 0, 0, 0);
        acc[i][j] = a;
      }
  };
  auto bias_term = [&](const Frags& f, const char* base, int s2) {  // the bias row's third term (see kGemm3)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x8 f3 = *reinterpret_cast<const bf16x8*>(base + (b3off ^ (s2 * 32)) + j * 2048);
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f3, f.a[i][0], acc[i][j], 0, 0, 0);
    }
  };
  // Software pipeline: the fragments of a k-step are read while the MFMAs of the k-step before run, and the stage
  // barrier sits between the two k-steps of a stage (after it every wave holds both k-steps of the stage in registers, so
  // the stage's buffer takes the LDS-DMA of the stage after the next).  The stage of the bias row is peeled out of the
  // loop (BIAS), and so is the last one: a branch inside the loop body lets the compiler sink the reads below the MFMAs
  // they are to overlap.
  dma_stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (kc32 > 1) dma_stage(1, 1);
  Frags fx, fy;
  read_frags(fx, smem_b, 0);
  auto first_half = [&](int kc, auto bias_c) {  // k-step 2 kc (fragments fx) under the reads of k-step 2 kc + 1 (fy)
    constexpr bool BIAS = decltype(bias_c)::value;
    const char* base = smem_b + (kc & 1) * kTg2Stage;
    read_frags(fy, base, 1);
    __builtin_amdgcn_sched_barrier(0);  // (the reads stay ahead of the MFMAs they overlap)
    if constexpr (BIAS)
      if (2 * kc == bias_step) bias_term(fx, base, 0);  // (wave-uniform)
    mfma_step(fx);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (BIAS)
      if (2 * kc + 1 == bias_step) bias_term(fy, base, 1);
  };
  auto mfma_group = [&](const Frags& f, int q) {  // product q of a k-step on the 8 blocks
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.b[j][q == 0 ? 1 : 0], f.a[i][q == 1 ? 1 : 0], acc[i][j], 0, 0, 0);
  };
  auto stage = [&](int kc, auto bias_c) {
    first_half(kc, bias_c);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's pieces of the next stage; fy arrived
    __builtin_amdgcn_s_barrier();
    read_frags(fx, smem_b + ((kc + 1) & 1) * kTg2Stage, 0);
    __builtin_amdgcn_sched_barrier(0);
    // second k-step, the LDS-DMA of stage kc + 2 (into this stage's buffer: every wave holds both k-steps in registers)
    // between its products
    const bool more = kc + 2 < kc32;
    mfma_group(fy, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (more) dma_pieces(kc + 2, kc & 1, 0, 4);
    __builtin_amdgcn_sched_barrier(0);
    mfma_group(fy, 1);
    __builtin_amdgcn_sched_barrier(0);
    if (more) dma_pieces(kc + 2, kc & 1, 4, 8);
    __builtin_amdgcn_sched_barrier(0);
    mfma_group(fy, 2);
    __builtin_amdgcn_sched_barrier(0);
  };
  const int kb = bias_step >> 1;
  int kc = 0;
  for (; kc < kb && kc + 1 < kc32; ++kc) stage(kc, std::false_type{});
  if (kc + 1 < kc32) stage(kc++, std::true_type{});  // (kc == kb)
  for (; kc + 1 < kc32; ++kc) stage(kc, std::false_type{});
  first_half(kc32 - 1, std::true_type{});
  mfma_step(fy);
  // C layout of a 32 x 32 block: lane & 31 = instance, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = column
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m0 = mtile * 256 + wm * 64 + i * 32;
    if (m0 >= Mp) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n0 = (2 * ntile + wn) * 128 + j * 32;
      float* ccol = C + ((size_t)(m0 >> 6) * N + n0) * 64 + (m0 & 63) + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) st_stream<2>(ccol + (size_t)((r & 3) + 8 * (r >> 2) + 4 * kg) * 64, acc[i][j][r]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// K3: vertex block of the normal equations.  grid ceil(B/4), block 256: wave w fits instance
// 4*blockIdx + w; the 4 waves walk the vertex tiles in lockstep so that the per-vertex constants
// (shapedirs, skinning pairs: 144 B/vertex) are fetched ONCE per workgroup and staged through a
// double-buffered LDS tile; per-instance streams (targets, v_posed) are register-prefetched one
// tile ahead.  98 fp32 accumulators per lane, DPP wave reduction, fp64 result.
// dynamic LDS: 4 joint blocks + 2 x (64 x cstride) constants.
// ------------------------------------------------------------------------------------------------
template <int S, int KW, bool WEIGHTED>
__global__ __launch_bounds__(256, 2) void k_shape_accum(DevModel m, Workspace ws, int B) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NE = sf::ne_size(S), STRIDE = sf::jd_stride(S);
  constexpr int CS = sf::cpack_stride(S, KW), TILE_F4 = 64 * CS / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int J = m.J, Vp = m.Vp, ntiles = Vp / 64;
  const int b_raw = blockIdx.x * kNW + wave;
  const int b = b_raw < B ? b_raw : B - 1;
  float* jd = smem + wave * J * STRIDE;
  float* cst = smem + kNW * J * STRIDE;  // [2][64*CS]
  float* priv = cst + 2 * 64 * CS + tid * 12;  // lane-private 12 floats (48-B stride: conflict-free b128)
  {
    const float4* src = reinterpret_cast<const float4*>(ws.jd + (size_t)b * J * STRIDE);
    float4* dst = reinterpret_cast<float4*>(jd);
    for (int k = lane; k < J * STRIDE / 4; k += 64) dst[k] = src[k];
  }
  // cooperative staging of the constants tile: TILE_F4 float4 over 256 threads (<= 3 each), kept in
  // named registers (an indexed array here ends up in scratch)
  const float4* cg = reinterpret_cast<const float4*>(m.cpackA);
  static_assert(TILE_F4 <= 1024, "constants tile too large for 4 float4 per thread");
  float4 c0, c1, c2, c3;
  auto cload = [&](int tile) {
    const float4* src = cg + (size_t)tile * TILE_F4;
    c0 = src[tid];
    if (TILE_F4 > 256 && tid + 256 < TILE_F4) c1 = src[tid + 256];
    if (TILE_F4 > 512 && tid + 512 < TILE_F4) c2 = src[tid + 512];
    if (TILE_F4 > 768 && tid + 768 < TILE_F4) c3 = src[tid + 768];
  };
  auto cstore = [&](int buf) {
    float4* dst = reinterpret_cast<float4*>(cst + buf * 64 * CS);
    dst[tid] = c0;
    if (TILE_F4 > 256 && tid + 256 < TILE_F4) dst[tid + 256] = c1;
    if (TILE_F4 > 512 && tid + 512 < TILE_F4) dst[tid + 512] = c2;
    if (TILE_F4 > 768 && tid + 768 < TILE_F4) dst[tid + 768] = c3;
  };
  const float* tvs = ws.tvs + (size_t)b * 3 * Vp;
  const float* vps = ws.vposed + (size_t)b * 3 * Vp;
  const float* vws = ws.vws + (size_t)b * Vp;
  float nx[7];
  auto sload = [&](int tile) {
    const int i = tile * 64 + lane;
    nx[0] = ld_stream<16>(vps + i); nx[1] = ld_stream<16>(vps + Vp + i); nx[2] = ld_stream<16>(vps + 2 * Vp + i);
    nx[3] = ld_stream<16>(tvs + i); nx[4] = ld_stream<16>(tvs + Vp + i); nx[5] = ld_stream<16>(tvs + 2 * Vp + i);
    nx[6] = WEIGHTED ? ld_stream<16>(vws + i) : 1.f;
  };
  cload(0);
  sload(0);
  cstore(0);
  __syncthreads();
  float acc[NE + 1];
#pragma unroll
  for (int k = 0; k <= NE; ++k) acc[k] = 0.f;
  for (int tile = 0; tile < ntiles; ++tile) {
    const float vp[3] = {nx[0], nx[1], nx[2]};
    const float tv[3] = {nx[3], nx[4], nx[5]};
    const float wv = nx[6];
    if (tile + 1 < ntiles) {
      cload(tile + 1);
      sload(tile + 1);
    }
    if (WEIGHTED) acc[NE] += wv;
    sf::shape_accum_vertex<S, KW, WEIGHTED>(jd, cst + (tile & 1) * 64 * CS + lane * CS, vp, tv, wv,
                                            priv, acc);
    if (tile + 1 < ntiles) cstore((tile + 1) & 1);
    __syncthreads();
  }
  double* out = ws.gramv + (size_t)b * (NE + 1);
  constexpr int NG = sf::ne_ng(S);
#pragma unroll
  for (int k = 0; k <= NE; ++k) {
    // unit weights: SA comes from the joint stage in closed form, W = V (bodyfitter.py:1038-1040)
    const bool dead = !WEIGHTED && ((k >= NG + S && k < NG + 4 * S) || k == NE);
    float r = 0.f;
    if (!dead) r = wave_sum_last(acc[k]);
    if (lane == 63 && b_raw < B) out[k] = dead ? (k == NE ? (double)m.V : 0.0) : (double)r;
  }
}

// ------------------------------------------------------------------------------------------------
// K3r: residual pass of the pair-Gram form (unit weights).  grid ceil(B/4), block 256, wave =
// instance, lockstep over the residual tiles (part-aligned, <= 16 distinct joints) whose constants
// blob [vertex records | MFMA A-operand weights | joint ids] is staged through double-buffered LDS.
// Per vertex ~115 FMAs: blended R/T0, residual b, u = Rt^T b, r1 += S_v^T u, Sb += b.  The per-joint
// residual moments mb_j = sum_v w_vj b_v (a scatter over the 4 skinning joints of every vertex) run on
// the otherwise idle matrix pipe: D(16 joint slots x 16) += W(16 x 4 vertices) . b(4 x 16) with
// v_mfma_f32_16x16x4_f32, 16 instructions per 64-vertex tile, then 3x4 lanes add D into the wave's LDS
// bins — deterministic, no atomics.
// dynamic LDS: 4 x [jd | bbuf 256 | bins (J+1)*4] + 2 blobs.
// ------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int S, int KW>
__global__ __launch_bounds__(256) void k_residual(DevModel m, Workspace ws, int B) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NE = sf::ne_size(S), NG = sf::ne_ng(S), STRIDE = sf::jd_stride(S);
  constexpr int CS = sf::cpack_stride(S, KW), BLOB = 64 * CS + 16 * 64 + 16, BLOB_F4 = BLOB / 4;
  static_assert(BLOB % 4 == 0 && BLOB_F4 <= 1280, "blob staging");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int J = m.J, Vp = m.Vp;
  const int b_raw = blockIdx.x * kNW + wave;
  const int b = b_raw < B ? b_raw : B - 1;
  const int per_wave = (J * STRIDE + 256 + (J + 1) * 4 + 3) / 4 * 4;
  float* jd = smem + wave * per_wave;
  float* bbuf = jd + J * STRIDE;  // [64][4]
  float* bins = bbuf + 256;       // [(J+1)][4]
  float* blob = smem + kNW * per_wave;  // [2][BLOB]
  {
    const float4* src = reinterpret_cast<const float4*>(ws.jd + (size_t)b * J * STRIDE);
    float4* dst = reinterpret_cast<float4*>(jd);
    for (int k = lane; k < J * STRIDE / 4; k += 64) dst[k] = src[k];
    for (int k = lane; k < (J + 1) * 4; k += 64) bins[k] = 0.f;
  }
  const float4* cg = reinterpret_cast<const float4*>(m.gblob);
  const float* tvs = ws.tvs + (size_t)b * 3 * Vp;
  const float* vps = ws.vposed + (size_t)b * 3 * Vp;
  // Two register stages (A, B), each holding one tile's constants-blob slice + this lane's target /
  // v_posed values; a stage is (re)loaded TWO tiles ahead of its use so that HBM / L2 latency is
  // covered by two tiles of work (one tile ahead left the loop latency-bound).  Named registers and
  // macros: a struct passed to a lambda ends up in scratch memory.
  float4 cA0, cA1, cA2, cA3, cA4, cB0, cB1, cB2, cB3, cB4;
  float vA0, vA1, vA2, tA0, tA1, tA2, vB0, vB1, vB2, tB0, tB1, tB2;
#define SF_ISSUE(P, tile_)                                                                     \
  do {                                                                                         \
    const float4* src_ = cg + (size_t)(tile_) * BLOB_F4;                                       \
    c##P##0 = src_[tid];                                                                       \
    if (BLOB_F4 > 256 && tid + 256 < BLOB_F4) c##P##1 = src_[tid + 256];                       \
    if (BLOB_F4 > 512 && tid + 512 < BLOB_F4) c##P##2 = src_[tid + 512];                       \
    if (BLOB_F4 > 768 && tid + 768 < BLOB_F4) c##P##3 = src_[tid + 768];                       \
    if (BLOB_F4 > 1024 && tid + 1024 < BLOB_F4) c##P##4 = src_[tid + 1024];                    \
    const int start_ = m.gtiles[(tile_) * 3], count_ = m.gtiles[(tile_) * 3 + 1];              \
    const int i_ = start_ + (lane < count_ ? lane : 0);                                        \
    const float keep_ = lane < count_ ? 1.f : 0.f; /* padding lanes: zero residual */          \
    v##P##0 = vps[i_] * keep_; v##P##1 = vps[Vp + i_] * keep_; v##P##2 = vps[2 * Vp + i_] * keep_; \
    t##P##0 = tvs[i_] * keep_; t##P##1 = tvs[Vp + i_] * keep_; t##P##2 = tvs[2 * Vp + i_] * keep_; \
  } while (0)
#define SF_COMMIT(P, buf_)                                                                     \
  do {                                                                                         \
    float4* dst_ = reinterpret_cast<float4*>(blob + (buf_) * BLOB);                            \
    dst_[tid] = c##P##0;                                                                       \
    if (BLOB_F4 > 256 && tid + 256 < BLOB_F4) dst_[tid + 256] = c##P##1;                       \
    if (BLOB_F4 > 512 && tid + 512 < BLOB_F4) dst_[tid + 512] = c##P##2;                       \
    if (BLOB_F4 > 768 && tid + 768 < BLOB_F4) dst_[tid + 768] = c##P##3;                       \
    if (BLOB_F4 > 1024 && tid + 1024 < BLOB_F4) dst_[tid + 1024] = c##P##4;                    \
  } while (0)
  float acc[S + 3];
#pragma unroll
  for (int k = 0; k < S + 3; ++k) acc[k] = 0.f;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int bsel = l15 < 3 ? l15 : 3;  // B-operand column: coordinate, columns >= 3 read the zero pad
  auto compute = [&](int buf, const float* vp, const float* tv) {
    const float* cur = blob + buf * BLOB;
    float bo[3];
    sf::residual_vertex<S, KW>(jd, cur + lane * CS, vp, tv, acc, bo);
    *reinterpret_cast<float4*>(bbuf + lane * 4) = make_float4(bo[0], bo[1], bo[2], 0.f);
    // scatter on the matrix pipe: D[slot][coord] += sum_vertex W[slot][vertex] b[vertex][coord]
    const float* wA = cur + 64 * CS;
    f32x4 D0 = {0.f, 0.f, 0.f, 0.f}, D1 = {0.f, 0.f, 0.f, 0.f};  // two chains: 40-cycle dependent latency
#pragma unroll
    for (int t = 0; t < 16; t += 2) {
      D0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wA[t * 64 + lane], bbuf[(4 * t + l4) * 4 + bsel], D0, 0, 0, 0);
      D1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wA[(t + 1) * 64 + lane], bbuf[(4 * t + 4 + l4) * 4 + bsel], D1, 0, 0, 0);
    }
    if (l15 < 3) {  // C/D layout 16x16: col = lane & 15, row = (lane >> 4) * 4 + r
      const int* slots = reinterpret_cast<const int*>(cur + 64 * CS + 16 * 64);
#pragma unroll
      for (int r = 0; r < 4; ++r) bins[slots[l4 * 4 + r] * 4 + l15] += D0[r] + D1[r];
    }
  };
  const int ntiles = m.ngt;
  SF_ISSUE(A, 0);
  if (ntiles > 1) SF_ISSUE(B, 1);
  SF_COMMIT(A, 0);
  __syncthreads();
  for (int tile = 0; tile < ntiles; tile += 2) {
    {
      const float vp[3] = {vA0, vA1, vA2}, tv[3] = {tA0, tA1, tA2};
      if (tile + 2 < ntiles) SF_ISSUE(A, tile + 2);
      compute(0, vp, tv);
      if (tile + 1 < ntiles) SF_COMMIT(B, 1);
      __syncthreads();
    }
    if (tile + 1 >= ntiles) break;
    {
      const float vp[3] = {vB0, vB1, vB2}, tv[3] = {tB0, tB1, tB2};
      if (tile + 3 < ntiles) SF_ISSUE(B, tile + 3);
      compute(1, vp, tv);
      if (tile + 2 < ntiles) SF_COMMIT(A, 0);
      __syncthreads();
    }
  }
#undef SF_ISSUE
#undef SF_COMMIT
  double* out = ws.gramv + (size_t)b * (NE + 1);
#pragma unroll
  for (int k = 0; k < S + 3; ++k) {
    const float r = wave_sum_last(acc[k]);
    if (lane == 63 && b_raw < B) out[k < S ? NG + k : NG + 4 * S + (k - S)] = (double)r;
  }
  if (b_raw < B) {
    if (lane == 63) out[NE] = (double)m.V;  // w_sum = num_vertices (bodyfitter.py:1038-1040)
    for (int k = lane; k < 3 * S; k += 64) out[NG + S + k] = 0.0;  // SA: closed form in the joint stage
    for (int k = lane; k < J * 3; k += 64) ws.mbj[(size_t)b * J * 3 + k] = bins[(k / 3) * 4 + k % 3];
  }
}

// ------------------------------------------------------------------------------------------------
// K3g: pair-Gram — the S x S Gramian of the vertex block from the rotations alone (unit weights).
// grid B, block 64 (one wave per instance, lanes = upper-triangle entries).  Independent of the
// targets and of the GEMM: it can run on a second stream next to K2.
// dynamic LDS: joint block + np*9 + J*3*S floats.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pair_gram(DevModel m, Workspace ws) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x, J = m.J, S = m.S, stride = sf::jd_stride(S);
  DevCtx cx{(int)threadIdx.x, 64};
  float* jd = smem;
  float* scratch = smem + J * stride;
  for (int k = threadIdx.x; k < J * stride; k += 64) jd[k] = ws.jd[(size_t)b * J * stride + k];
  __syncthreads();
  sf::pair_gram_stage(cx, m.jt, scratch, jd, ws.gramv + (size_t)b * (sf::ne_size(S) + 1));
}

// ------------------------------------------------------------------------------------------------
// K4: solve.  grid B, block 64.
// ------------------------------------------------------------------------------------------------
// mode 0: per-instance solve; 1 / 2: the two halves of a share_beta solve (sf::solve_stage)
template <int N, bool GEN = false>
__global__ __launch_bounds__(GEN ? 1024 : 64) void k_shape_solve(DevModel m, Workspace ws, int B, float beta_reg,
                                                    float beta_reg2, float kid_reg, int pair_form,
                                                    int use_ref, int mode, int b0, int cen_b0 = 0,
                                                    const int32_t* __restrict__ row_seg = nullptr) {
  // cen_b0: the instance whose system is row 0 of ws.cen (general path: the rows of a share_beta solve are written and
  // summed chunk by chunk, the workspace holds one chunk of them).  row_seg: mode 2 reads the sum of the instance's own
  // segment, row row_seg[b] of ws.censum (null: the batch is one segment)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int half = GEN ? 0 : (int)threadIdx.x / N, J = m.J, S = m.S;
  const int b = GEN ? min(b0 + (int)blockIdx.x, B - 1) : min(b0 + (int)blockIdx.x * (64 / N) + half, B - 1);
  // (general path: the stage takes any number of lanes — a 256-thread workgroup per instance for many unknowns, whose
  // S x S factorisation is S^3 / 3 updates spread over the lanes)
  typename StageCtx<N>::type cx{GEN ? (int)threadIdx.x : (int)threadIdx.x % N, GEN ? (int)blockDim.x : N};
  const int NE1 = sf::ne_size(S) + 1;
  float* scratch;
  if constexpr (GEN) scratch = ws.gsolve + (size_t)b * ((sf::gen_solve_scratch_floats(S) + 3) / 4 * 4);
  else scratch = smem + half * sf::solve_scratch_floats(S);
  sf::solve_stage(cx, m.jt, scratch, ws.gramv + (size_t)b * NE1, ws.gramj + (size_t)b * NE1,
                  ws.pext + (size_t)b * J * 3 * (S + 1), ws.jd + (size_t)b * J * sf::jd_stride(S),
                  pair_form ? ws.mbj + (size_t)b * J * 3 : nullptr, beta_reg, beta_reg2, kid_reg,
                  ws.beta + (size_t)b * S, ws.trans + (size_t)b * 3, ws.rjoints + (size_t)b * J * 3,
                  ws.jb + (size_t)b * J * 4, use_ref ? ws.regref + (size_t)b * S : nullptr, mode,
                  mode == 1 ? ws.cen + (size_t)(b - cen_b0) * (S * S + S) : ws.censum + (size_t)(row_seg ? row_seg[b] : 0) * (S * S + S),
                  ws.jbT ? ws.jbT + ((size_t)(b >> 6) * J * 4) * 64 + (b & 63) : nullptr,
                  GEN ? reinterpret_cast<double*>(smem) : nullptr);
}

// ------------------------------------------------------------------------------------------------
// Scaled last solve of fit(scale_target / scale_fit) — a niche option, kept simple: one wave per
// instance for the extra vertex sums (joint block in LDS, records and streams straight from L2/HBM).
// ------------------------------------------------------------------------------------------------
template <int S, int KW>
__global__ __launch_bounds__(64) void k_scale_extras(DevModel m, Workspace ws, int weighted) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int STRIDE = sf::jd_stride(S), CS = sf::cpack_stride(S, KW), NX = S + sf::kScaleExtras;
  const int b = blockIdx.x, lane = threadIdx.x, J = m.J, Vp = m.Vp;
  for (int k = lane; k < J * STRIDE; k += 64) smem[k] = ws.jd[(size_t)b * J * STRIDE + k];
  __syncthreads();
  const float* tvs = ws.tvs + (size_t)b * 3 * Vp;
  const float* vps = ws.vposed + (size_t)b * 3 * Vp;
  float acc[NX];
#pragma unroll
  for (int k = 0; k < NX; ++k) acc[k] = 0.f;
  for (int i = lane; i < m.V; i += 64) {  // slots [0, V) are the real vertices
    const float vp[3] = {vps[i], vps[Vp + i], vps[2 * Vp + i]};
    const float tv[3] = {tvs[i], tvs[Vp + i], tvs[2 * Vp + i]};
    const float wv = weighted ? ws.vws[(size_t)b * Vp + i] : 1.f;
    sf::scale_extras_vertex<S, KW>(smem, m.cpackA + (size_t)i * CS, vp, tv, wv, acc);
  }
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    const float r = wave_sum(acc[k]);
    if (lane == 0) ws.vextra[(size_t)b * 32 + k] = r;
  }
}

struct ScaledSolveArgs {
  const float* tj;  // centred target joints (joint block) or null
  const float* jw;  // joint weights entering the solve or null
  int joint_block, mode, pair_form, use_ref;
  float beta_reg, beta_reg2, kid_reg, scale_reg;
  int share, B;  // share_beta with a scale unknown: 1 assemble the reduced system, 2 solve the sum
  int b0, cen_b0;  // first instance of the launch; the instance whose reduced system is row 0 of ws.cen (see k_shape_solve)
  const int32_t* row_seg;  // share 2: the segment of an instance, its row of ws.censum (null: one segment)
};

// GEN (general path): the scratch in global memory (ws.gsolve), the panel of ldlt_solve in LDS, the extra sums from the
// accumulate kernel's target column (ws.gvex, S + 6 per instance), any number of threads
template <bool GEN>
__global__ __launch_bounds__(GEN ? 1024 : 64) void k_shape_solve_scaled(DevModel m, Workspace ws, ScaledSolveArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = min(a.b0 + (int)blockIdx.x, a.B - 1), J = m.J, S = m.S;
  DevCtx cx{(int)threadIdx.x, (int)blockDim.x};
  const int NE1 = sf::ne_size(S) + 1;
  float* scratch = GEN ? ws.gsolve + (size_t)b * ((sf::gen_solve_scratch_floats(S) + 3) / 4 * 4) : smem;
  sf::scaled_solve_stage(cx, m.jt, scratch, ws.gramv + (size_t)b * NE1, ws.gramj + (size_t)b * NE1,
                         GEN ? nullptr : ws.vextra + (size_t)b * 32,
                         ws.pext + (size_t)b * J * 3 * (S + 1),
                         ws.jd + (size_t)b * J * sf::jd_stride(S),
                         a.pair_form ? ws.mbj + (size_t)b * J * 3 : nullptr,
                         a.tj ? a.tj + (size_t)b * J * 3 : nullptr, a.jw ? a.jw + (size_t)b * J : nullptr,
                         a.joint_block != 0, a.mode, a.beta_reg, a.beta_reg2, a.kid_reg, a.scale_reg,
                         a.use_ref ? ws.regref + (size_t)b * S : nullptr, ws.beta_out + (size_t)b * S,
                         ws.beta + (size_t)b * S, ws.trans + (size_t)b * 3, ws.scale + b,
                         ws.rjoints + (size_t)b * J * 3, ws.jb + (size_t)b * J * 4, a.share,
                         a.share == 1 ? ws.cen + (size_t)(b - a.cen_b0) * (S * S + S)
                                      : ws.censum + (size_t)(a.row_seg ? a.row_seg[b] : 0) * (S * S + S),
                         GEN ? reinterpret_cast<double*>(smem) : nullptr,
                         GEN ? ws.gvex + (size_t)b * (S + sf::kScaleExtras) : nullptr);
  // the instance-innermost copy of the skinning translations for the batch-major LBS pass that may follow
  // (sf::solve_stage writes it itself)
  __syncthreads();
  if (a.share != 1 && !GEN)
    for (int k = threadIdx.x; k < J * 3; k += 64) {
      const int e = (k / 3) * 4 + k % 3;
      ws.jbT[((size_t)(b >> 6) * J * 4 + e) * 64 + (b & 63)] = ws.jb[(size_t)b * J * 4 + e];
    }
}

// After the scaled solve (and the LBS pass when the refinement follows): what the refinement and the
// epilogue see (bodyfitter.py:462-519).
//   scale_target: targets x s -> part sums raw, s_t x s, target joints x s; mean x s
//   scale_fit:    reference <- s reference + (1 - s) trans -> raw, s_a, reference joints; mean / s
// and the undivided shape back into ws.beta.  grid B, block 64.
__global__ __launch_bounds__(64) void k_scale_refs(DevModel m, Workspace ws, const float* __restrict__ tj_in,
                                                   int mode, int have_psum, int regressed) {
  const int b = blockIdx.x, lane = threadIdx.x, J = m.J, S = m.S;
  const float s = ws.scale[b];
  const float tr[3] = {(1.f - s) * ws.trans[b * 3], (1.f - s) * ws.trans[b * 3 + 1],
                       (1.f - s) * ws.trans[b * 3 + 2]};
  if (have_psum) {
    for (int j = lane; j < J; j += 64) {
      float* ps = ws.psum + ((size_t)b * J + j) * sf::kPsum;
      if (mode == 1) {
        for (int k = 0; k < 12; ++k) ps[k] *= s;  // raw and s_t are linear in the targets
        for (int c = 0; c < 3; ++c) ws.tjs[((size_t)b * J + j) * 3 + c] = s * tj_in[((size_t)b * J + j) * 3 + c];
      } else {
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) ps[r * 3 + c] = s * ps[r * 3 + c] + ps[9 + r] * tr[c];
        for (int c = 0; c < 3; ++c) {
          ps[12 + c] = s * ps[12 + c] + ps[15] * tr[c];
          float* rj = ws.rjoints + ((size_t)b * J + j) * 3 + c;
          *rj = s * *rj + tr[c];
          if (regressed) {
            float* rr = ws.rjreg + ((size_t)b * J + j) * 3 + c;
            *rr = s * *rr + m.reg_rowsum[j] * tr[c];
          }
        }
      }
    }
  }
  for (int k = lane; k < S; k += 64) ws.beta[(size_t)b * S + k] = ws.beta_out[(size_t)b * S + k];
  if (lane < 3) ws.mean[b * 3 + lane] = mode == 1 ? ws.mean[b * 3 + lane] * s : ws.mean[b * 3 + lane] / s;
}

// share_beta: the sums of the per-instance systems over the SEGMENTS of the batch — consecutive runs of rows, one shared
// shape per run (sf::ShareSegments; the batch as one run without a plan).  Deterministic: a fixed two-level order that
// depends on the run sizes alone.  k_share_partial: a workgroup per PARTIAL BLOCK (64 consecutive rows counted from the
// run's first row), thread = entry of the (S*S + S) record: the sum of the block's rows, eight interleaved accumulators
// (sf::sum_rows_f64: eight loads in flight; one workgroup walking all B rows, as in rounds 1-3, took 270 us per solve at
// B = 4096: a latency-bound chain of 1024 dependent rounds); k_share_reduce: one workgroup per run adds the run's partial
// rows the same way into the run's row of ws.censum.
// The tables of a plan on the device, all null for the single run [B]: a block is then (64 p, min(64, B - 64 p)), the one
// run holds every block, every row belongs to run 0.
struct ShareSegs {
  const int32_t* row_seg;   // (B)
  const int32_t* seg_blk;   // (runs, 2) first partial block, blocks
  const int32_t* blk_rows;  // (blocks, 2) first row, rows
  int nseg, nblk;
};
// grid (blocks of this launch, ceil(NC / 512)); p0: the first partial block of the launch; cen_b0: the instance whose
// system is row 0 of ws.cen (general path: the workspace holds the rows of one group of blocks).
__global__ __launch_bounds__(512) void k_share_partial(Workspace ws, ShareSegs sg, int B, int NC, int p0, int cen_b0) {
  const int e = blockIdx.y * 512 + threadIdx.x, p = p0 + blockIdx.x;
  if (e >= NC || p >= sg.nblk) return;
  const int r0 = sg.blk_rows ? sg.blk_rows[2 * p] : 64 * p;
  const int n = sg.blk_rows ? sg.blk_rows[2 * p + 1] : min(64, B - r0);
  ws.cenP[(size_t)p * NC + e] = sf::sum_rows_f64(ws.cen + (size_t)(r0 - cen_b0) * NC + e, n, (size_t)NC);
}
// grid (runs, ceil(NC / 512)): the sum of a run's partial rows into its row of ws.censum
__global__ __launch_bounds__(512) void k_share_reduce(Workspace ws, ShareSegs sg, int NC) {
  const int e = blockIdx.y * 512 + threadIdx.x, g = blockIdx.x;
  if (e >= NC || g >= sg.nseg) return;
  const int pf = sg.seg_blk ? sg.seg_blk[2 * g] : 0, np = sg.seg_blk ? sg.seg_blk[2 * g + 1] : sg.nblk;
  ws.censum[(size_t)g * NC + e] = sf::sum_rows_f64(ws.cenP + (size_t)pf * NC + e, np, (size_t)NC);
}

// ------------------------------------------------------------------------------------------------
// K5: vertices at the solved shape + part sums against the targets.  grid ceil(B/4), block 256,
// wave = instance, lockstep over the part-aligned segments with LDS-staged constants (as K3).
// MODE 0: part sums only (joints given).  MODE 1: also store the vertices (sorted SoA) for the
// joint regression of the joints-omitted path.  MODE 2: store vertices in ORIGINAL order to `out`
// (B,V,3) (shape-solve entry point / forward) over ALL slots — no part sums.
// dynamic LDS: 4 x (joint block rows R|T0 + jb) + 2 x (64 x cstride) constants + 4 x 36.
// ------------------------------------------------------------------------------------------------
template <int S, int KW, bool WEIGHTED, int MODE, bool SOLVE>
__global__ __launch_bounds__(256) void k_lbs_partsum(DevModel m, Workspace ws, int B, int nb,
                                                     const float* __restrict__ beta_in,
                                                     const float* __restrict__ trans_in,
                                                     const float* __restrict__ kid_in,
                                                     float* __restrict__ out, float beta_reg,
                                                     float beta_reg2) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int STRIDE = sf::jd_stride(S);
  constexpr int CS = sf::cpack_stride(S, KW), TILE_F4 = 64 * CS / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int J = m.J, Vp = m.Vp, V = m.V;
  const int b_raw = blockIdx.x * kNW + wave;
  const int b = b_raw < B ? b_raw : B - 1;
  const bool live = b_raw < B;
  const int per_wave =
      (J * STRIDE + J * 4 + 36 + (SOLVE ? sf::solve_scratch_floats(S) : 0) + 3) / 4 * 4;  // 16-B multiple
  float* jd = smem + wave * per_wave;
  float* jb = jd + J * STRIDE;
  float* sbeta = jb + J * 4;   // [32]
  float* strans = sbeta + 32;  // [4]
  float* cst = smem + kNW * per_wave;
  {
    const float4* src = reinterpret_cast<const float4*>(ws.jd + (size_t)b * J * STRIDE);
    float4* dst = reinterpret_cast<float4*>(jd);
    for (int k = lane; k < J * STRIDE / 4; k += 64) dst[k] = src[k];
  }
  if (SOLVE) {
    // K4 fused: this wave solves its instance's normal equations (fp64 centring + Cholesky) and
    // leaves beta / trans / per-joint skinning translations in LDS for the vertex loop below.
    // All four waves run the stage in lockstep (uniform barriers).
    DevCtx cx{lane, 64};
    const int NE1 = sf::ne_size(S) + 1;
    if (lane < 32) sbeta[lane] = 0.f;
    sf::solve_stage(cx, m.jt, strans + 4, ws.gramv + (size_t)b * NE1, ws.gramj + (size_t)b * NE1,
                    ws.pext + (size_t)b * J * 3 * (S + 1), ws.jd + (size_t)b * J * STRIDE, nullptr,
                    beta_reg, beta_reg2, beta_reg, sbeta, strans, ws.rjoints + (size_t)b * J * 3, jb);
    __syncthreads();
    if (lane < S) ws.beta[(size_t)b * S + lane] = sbeta[lane];
    if (lane < 3) ws.trans[(size_t)b * 3 + lane] = strans[lane];
  } else {
    for (int k = lane; k < J * 4; k += 64) jb[k] = ws.jb[(size_t)b * J * 4 + k];
    if (lane < S) {
      float v = (beta_in && lane < nb) ? beta_in[(size_t)b * nb + lane] : 0.f;
      if (kid_in && m.jt.n_kid && lane == S - 1) v = kid_in[b];
      sbeta[lane] = v;
    }
    if (lane < 3) strans[lane] = trans_in ? trans_in[(size_t)b * 3 + lane] : 0.f;
  }
  // MODE 2 walks the dense tiles (every slot), the other modes the part-aligned segments
  const int nsteps = MODE == 2 ? Vp / 64 : m.nseg;
  // cooperative staging of the constants tile: TILE_F4 float4 over 256 threads (<= 3 each), kept in
  // named registers (an indexed array here ends up in scratch)
  const float4* cg = reinterpret_cast<const float4*>(MODE == 2 ? m.cpackA : m.cpackB);
  static_assert(TILE_F4 <= 1024, "constants tile too large for 4 float4 per thread");
  float4 c0, c1, c2, c3;
  auto cload = [&](int step) {
    const float4* src = cg + (size_t)step * TILE_F4;
    c0 = src[tid];
    if (TILE_F4 > 256 && tid + 256 < TILE_F4) c1 = src[tid + 256];
    if (TILE_F4 > 512 && tid + 512 < TILE_F4) c2 = src[tid + 512];
    if (TILE_F4 > 768 && tid + 768 < TILE_F4) c3 = src[tid + 768];
  };
  auto cstore = [&](int buf) {
    float4* dst = reinterpret_cast<float4*>(cst + buf * 64 * CS);
    dst[tid] = c0;
    if (TILE_F4 > 256 && tid + 256 < TILE_F4) dst[tid + 256] = c1;
    if (TILE_F4 > 512 && tid + 512 < TILE_F4) dst[tid + 512] = c2;
    if (TILE_F4 > 768 && tid + 768 < TILE_F4) dst[tid + 768] = c3;
  };
  const float* tvs = ws.tvs + (size_t)b * 3 * Vp;
  const float* vps = ws.vposed + (size_t)b * 3 * Vp;
  const float* vws = ws.vws + (size_t)b * Vp;
  float* rv = ws.rverts + (size_t)b * 3 * Vp;
  float nx[7];
  int n_start = 0, n_count = 0, n_part = 0;
  auto sload = [&](int step) {
    if (MODE == 2) {
      n_start = step * 64;
      n_count = 64;
      n_part = 0;
    } else {
      n_start = m.segments[step * 3];
      n_count = m.segments[step * 3 + 1];
      n_part = m.segments[step * 3 + 2];
    }
    const int i = n_start + (lane < n_count ? lane : 0);
    nx[0] = ld_stream<16>(vps + i); nx[1] = ld_stream<16>(vps + Vp + i); nx[2] = ld_stream<16>(vps + 2 * Vp + i);
    if (MODE != 2) {
      nx[3] = ld_stream<16>(tvs + i); nx[4] = ld_stream<16>(tvs + Vp + i); nx[5] = ld_stream<16>(tvs + 2 * Vp + i);
      nx[6] = WEIGHTED ? ld_stream<16>(vws + i) : 1.f;
    }
  };
  cload(0);
  sload(0);
  cstore(0);
  __syncthreads();
  float beta[S];
#pragma unroll
  for (int s = 0; s < S; ++s) beta[s] = sbeta[s];
  const float trans[3] = {strans[0], strans[1], strans[2]};
  float acc[sf::kPsum];
#pragma unroll
  for (int k = 0; k < sf::kPsum; ++k) acc[k] = 0.f;
  for (int step = 0; step < nsteps; ++step) {
    const float vp[3] = {nx[0], nx[1], nx[2]};
    const float tv[3] = {nx[3], nx[4], nx[5]};
    const float wv = nx[6];
    const int start = n_start, count = n_count, part = n_part;
    if (step + 1 < nsteps) {
      cload(step + 1);
      sload(step + 1);
    }
    const bool flush = MODE != 2 && ((step + 1 == nsteps) || (n_part != part));
    if (lane < count) {
      float v[3];
      sf::lbs_vertex<S, KW>(jd, jb, cst + (step & 1) * 64 * CS + lane * CS, vp, beta, trans, v);
      const int i = start + lane;
      if (MODE == 2) {
        const int o = m.perm[i];
        if (o >= 0 && live) {
          out[((size_t)b * V + o) * 3] = v[0];
          out[((size_t)b * V + o) * 3 + 1] = v[1];
          out[((size_t)b * V + o) * 3 + 2] = v[2];
        }
      } else {
        if (MODE == 1 && live) {
          rv[i] = v[0];
          rv[Vp + i] = v[1];
          rv[2 * Vp + i] = v[2];
        }
        sf::partsum_vertex(tv, v, wv, WEIGHTED, acc);
      }
    }
    if (flush) {
      float* ps = ws.psum + ((size_t)b * J + part) * sf::kPsum;
#pragma unroll
      for (int k = 0; k < sf::kPsum; ++k) {
        const float r = wave_sum_last(acc[k]);
        if (lane == 63 && live) ps[k] = r;
        acc[k] = 0.f;
      }
    }
    if (step + 1 < nsteps) cstore((step + 1) & 1);
    __syncthreads();
  }
}

// the unused-part vertices of the joints-omitted path (MODE 1 stores only the used segments)
template <int S, int KW>
__global__ __launch_bounds__(256) void k_lbs_rest(DevModel m, Workspace ws) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int STRIDE = sf::jd_stride(S);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int J = m.J, Vp = m.Vp;
  float* jd = smem;
  float* jb = jd + J * STRIDE;
  for (int k = tid; k < J * STRIDE; k += 256) jd[k] = ws.jd[(size_t)b * J * STRIDE + k];
  for (int k = tid; k < J * 4; k += 256) jb[k] = ws.jb[(size_t)b * J * 4 + k];
  __syncthreads();
  float beta[S];
#pragma unroll
  for (int s = 0; s < S; ++s) beta[s] = ws.beta[(size_t)b * S + s];
  const float trans[3] = {ws.trans[b * 3], ws.trans[b * 3 + 1], ws.trans[b * 3 + 2]};
  const float* vps = ws.vposed + (size_t)b * 3 * Vp;
  float* rv = ws.rverts + (size_t)b * 3 * Vp;
  for (int i = m.n_used + tid; i < Vp; i += 256) {
    float v[3] = {0.f, 0.f, 0.f};
    if (m.perm[i] >= 0) {
      const float vp[3] = {vps[i], vps[Vp + i], vps[2 * Vp + i]};
      sf::lbs_vertex<S, KW>(jd, jb, m.cpackA + (size_t)i * sf::cpack_stride(S, KW), vp, beta, trans, v);
    }
    rv[i] = v[0];
    rv[Vp + i] = v[1];
    rv[2 * Vp + i] = v[2];
  }
}

// ------------------------------------------------------------------------------------------------
// K6: dependent refinement + epilogue.  grid B, block 64.
// ------------------------------------------------------------------------------------------------
struct RefineArgs {
  const float* tj;        // (B,J,3) joints of the joint term (centred targets or regressed)
  const float* rj_term;   // (B,J,3) reference joints of the joint term
  const float* jw;        // (B,J) or null
  int final_adjust;
  float *pose, *betas, *trans, *kid, *orient, *rel;
  int scaled;  // known-shape fit with scale_fit: rest joints are scaled by ws.scale
  int B;
  int b0;  // first instance of the launch (see k_joint_stage)
};

template <int N>
__global__ __launch_bounds__(64) void k_refine_epilogue(DevModel m, RefineArgs a, Workspace ws) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int half = (int)threadIdx.x / N, J = m.J, S = m.S;
  const int b = min(a.b0 + (int)blockIdx.x * (64 / N) + half, a.B - 1);
  typename StageCtx<N>::type cx{(int)threadIdx.x % N, N};
  sf::JointScratch sh = sf::carve_joint_scratch(smem + half * sf::joint_scratch_floats(J, S, 1), J, S, 1);
  sf::refine_stage(cx, m.jt, sh, ws.psum + (size_t)b * J * sf::kPsum, a.tj + (size_t)b * J * 3,
                   a.rj_term + (size_t)b * J * 3, ws.rjoints + (size_t)b * J * 3,
                   a.jw ? a.jw + (size_t)b * J : nullptr, ws.G + (size_t)b * J * 9,
                   ws.beta + (size_t)b * S, ws.trans + (size_t)b * 3, ws.mean + (size_t)b * 3,
                   a.final_adjust != 0, a.pose + (size_t)b * J * 3,
                   a.betas ? a.betas + (size_t)b * (S - m.jt.n_kid - m.jt.n_pad) : nullptr, a.trans + (size_t)b * 3,
                   a.kid ? a.kid + b : nullptr, a.orient ? a.orient + (size_t)b * J * 9 : nullptr,
                   a.rel ? a.rel + (size_t)b * J * 9 : nullptr, a.scaled ? ws.scale + b : nullptr);
}

// ------------------------------------------------------------------------------------------------
// known-shape fit: the given shape (betas [+ kid]) to the workspace layout, zero translation
// ------------------------------------------------------------------------------------------------
__global__ void k_fill_shape(Workspace ws, int B, int S, int n_kid, const float* __restrict__ betas,
                             int nb, const float* __restrict__ kid, const float* __restrict__ trans = nullptr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int s = 0; s < S - n_kid; ++s)
    ws.beta[(size_t)b * S + s] = (betas && s < nb) ? betas[(size_t)b * nb + s] : 0.f;
  if (n_kid) ws.beta[(size_t)b * S + S - 1] = kid ? kid[b] : 0.f;
  for (int s = 0; s < S; ++s) ws.regref[(size_t)b * S + s] = ws.beta[(size_t)b * S + s];
  for (int c = 0; c < 3; ++c) ws.trans[b * 3 + c] = trans ? trans[(size_t)b * 3 + c] : 0.f;
}

// known-shape fit: scale + translation of the posed reference onto the target, folded into the part
// sums and joints the refinement reads (sf::scale_trans_stage).  grid B, block 256.
struct ScaleTransArgs {
  const float* tj;   // (B,J,3) centred target joints or null (vertices only)
  const float* jw;   // (B,J) or null
  int weighted_v, with_scale, regressed;
  float* scale_out;  // (B) or null
};

__global__ __launch_bounds__(256) void k_scale_trans(DevModel m, ScaleTransArgs a, Workspace ws) {
  __shared__ float red[256 * 8];
  const int b = blockIdx.x, J = m.J, Vp = m.Vp;
  DevCtx cx{(int)threadIdx.x, 256};
  sf::scale_trans_stage(cx, J, m.V, Vp, red, ws.tvs + (size_t)b * 3 * Vp, ws.rverts + (size_t)b * 3 * Vp,
                        a.weighted_v ? ws.vws + (size_t)b * Vp : nullptr,
                        a.tj ? a.tj + (size_t)b * J * 3 : nullptr, ws.rjoints + (size_t)b * J * 3,
                        a.jw ? a.jw + (size_t)b * J : nullptr, a.with_scale != 0,
                        ws.psum + (size_t)b * J * sf::kPsum,
                        a.regressed ? ws.rjreg + (size_t)b * J * 3 : nullptr, m.reg_rowsum,
                        ws.trans + (size_t)b * 3, ws.scale + b);
  if (a.scale_out && threadIdx.x == 0) a.scale_out[b] = ws.scale[b];  // written by this lane above
}

// ------------------------------------------------------------------------------------------------
// forward: joint prologue.  grid B, block 64.
// ------------------------------------------------------------------------------------------------
struct ForwardArgs {
  const float *pose, *glob, *betas, *trans, *kid;
  const float* rel = nullptr;  // (B,J,3,3) relative rotations (rel_rotmats), alternative to pose / glob
  int nb;
  float *joints, *orient;
};

template <bool GEN = false>
__global__ __launch_bounds__(64) void k_forward_joint(DevModel m, ForwardArgs a, Workspace ws) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x, J = m.J, S = m.S;
  DevCtx cx{(int)threadIdx.x, 64};
  sf::JointScratch sh = gen_joint_scratch<GEN>(m, ws, smem, b, 0);
  float* jd = ws.jd + (size_t)b * J * sf::jd_stride(S);
  sf::forward_joint_stage(cx, m.jt, sh, a.pose ? a.pose + (size_t)b * J * 3 : nullptr,
                          a.glob ? a.glob + (size_t)b * J * 9 : nullptr,
                          a.betas ? a.betas + (size_t)b * a.nb : nullptr, a.betas ? a.nb : 0,
                          a.kid ? a.kid + b : nullptr, a.trans ? a.trans + (size_t)b * 3 : nullptr,
                          ws.rp + (size_t)b * m.Kp, jd,
                          a.joints + (size_t)b * J * 3,
                          a.orient ? a.orient + (size_t)b * J * 9 : nullptr,
                          a.rel ? a.rel + (size_t)b * J * 9 : nullptr);
  __syncthreads();
  // skinning translations for the vertex kernel
  for (int k = threadIdx.x; k < J * 3; k += 64) {
    const float v = jd[(k / 3) * sf::jd_stride(S) + 9 + k % 3];
    ws.jb[(size_t)b * J * 4 + (k / 3) * 4 + k % 3] = v;
    if (ws.jbT) ws.jbT[(((size_t)(b >> 6) * J * 4) + (k / 3) * 4 + k % 3) * 64 + (b & 63)] = v;  // batch-major LBS kernel
  }
}

// betas / kid / trans of the last solve to the caller's arrays (shape-solve entry point)
// `src`: (B,S) solved shape — ws.beta, or ws.beta_out (the undivided one) after a scaled solve
__global__ void k_emit_solution(Workspace ws, const float* __restrict__ src, int B, int S, int n_kid, int nb,
                                int add_mean, float* __restrict__ betas, float* __restrict__ trans,
                                float* __restrict__ kid) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int s = 0; s < nb; ++s) betas[(size_t)b * nb + s] = src[(size_t)b * S + s];  // nb = the caller's betas
  if (n_kid && kid) kid[b] = src[(size_t)b * S + S - 1];
  for (int c = 0; c < 3; ++c)
    trans[b * 3 + c] = ws.trans[b * 3 + c] + (add_mean ? ws.mean[b * 3 + c] : 0.f);
}

// scatter G given by the caller into the workspace (shape-solve entry point)
__global__ void k_copy(const float* __restrict__ src, float* __restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}


// ------------------------------------------------------------------------------------------------
// Test hook (smplfit_primitives_f32): the rotation primitives of sf_math.h, one element per thread,
// compiled for the device — the hardware rsq / rcp seeded arithmetic the joint-level kernels run.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_primitives(int op, const float* __restrict__ a,
                                                   const float* __restrict__ b, float* __restrict__ out,
                                                   int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  float x[12], y[12], r[9];
  switch (op) {
    case 0:
      for (int k = 0; k < 9; ++k) x[k] = a[(size_t)i * 9 + k];
      sf::proj_so3(x, r);
      for (int k = 0; k < 9; ++k) out[(size_t)i * 9 + k] = r[k];
      break;
    case 1:
      for (int k = 0; k < 3; ++k) x[k] = a[(size_t)i * 3 + k];
      sf::rotvec2mat(x, r);
      for (int k = 0; k < 9; ++k) out[(size_t)i * 9 + k] = r[k];
      break;
    case 2:
      for (int k = 0; k < 9; ++k) x[k] = a[(size_t)i * 9 + k];
      sf::mat2rotvec(x, r);
      for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = r[k];
      break;
    case 3:
      for (int k = 0; k < 3; ++k) {
        x[k] = a[(size_t)i * 3 + k];
        y[k] = b[(size_t)i * 3 + k];
      }
      sf::align_unit_vectors(x, y, r);
      for (int k = 0; k < 9; ++k) out[(size_t)i * 9 + k] = r[k];
      break;
    default:
      for (int k = 0; k < 3; ++k) x[k] = a[(size_t)i * 3 + k];
      for (int k = 0; k < 12; ++k) y[k] = b[(size_t)i * 12 + k];
      sf::swing_twist(x, y, y + 3, r);
      for (int k = 0; k < 9; ++k) out[(size_t)i * 9 + k] = r[k];
      break;
  }
}
