// GENERAL-path vertex kernels (included by smplfit_hip.hip): any number of shape unknowns, any number of skinning
// weights per vertex.
//
// The reference takes any num_betas (default: every column of the model file, common.py:223, 381-385) and routes the
// large counts through _fit_shape_general (pt/bodyfitter.py:202, 1104-1319): the design matrix A (B, 3V + 3J, S) in
// memory, a dense fp32 Gramian, a Cholesky solve; and it blends with the dense (V, J) skinning matrix
// (:1000-1003).  The kernels of the other two paths are instantiated for 10 / 16 unknowns and 4 / 8 weights per vertex;
// a model beyond that (HostTables::general) runs
//   * the SAME per-instance stages (sf_stages.h: joint stage, solve, refinement, forward joint stage — they take S at
//     run time) with their S-sized scratch (P, T, the S x S system) in global memory instead of LDS — the solve blocked
//     (sf::ldlt_solve with a panel in LDS) — and
//   * the vertex kernels below with run-time loops over the unknowns and the weights:
//       k_gen_accum_mfma  the vertex block of the normal equations (record layout of sf::ne_*: G upper triangle, r, SA,
//                         Sb, W) + the joint rows + the scale unknown's sums, as ONE symmetric rank-k update on the matrix
//                         cores (the default; further down in this file)
//       k_gen_accum       the same record on the vector ALUs: 4 x 4 register blocks per thread from rows in LDS — the
//                         first form, kept behind SMPLFIT_GEN_MFMA=0 as an A/B and a second implementation for the tests
//       k_gen_lbs         the vertices at the solution + part sums (the LBS forward of BodyModel.forward in MODE 2)
// Never materialised: A (25 MB per instance at S = 300): a workgroup forms the rows of 8 / 32 vertices in LDS at a time.
// fp32 products and sums, as the reference's general path; the centring identity and the solve are fp64 (stage S).
//
// ---- k_gen_accum (vector ALUs) ----
// vertices per tile of k_gen_accum (3 rows each): 8 for many unknowns (24 rows of up to 1024 floats in LDS), 32 for few
// (S <= 128: the three barriers of a tile are amortised over four times the rows)
inline int gen_tile_vertices(int S) { return S <= 128 ? 32 : 8; }
constexpr int kGenBlk = 4;       // 4 x 4 blocks of the Gramian per thread and pass
constexpr int kGenQ = 4;         // unknowns per thread for the right-hand side: S <= kGenQ * (threads of the workgroup)
constexpr int kGenMaxS = kGenQ * 256 - 1;  // (smplfit_create refuses more shape unknowns)
inline int gen_accum_threads(int S) { return S <= 88 ? 64 : 256; }
// vertices between two additions of the accumulate kernels' fp32 sums to the fp64 record (both forms).  A longer chain
// costs the solve its floor: with 2048 vertices (6144 rows) per chain the betas of a target far from the template (betas
// of +-5: residuals of a metre) sat 5e-4 from the fp64 solve and a weighted solve without a ridge 1e-3 on the one-chain
// form below, where the reference's fp32 — a blocked product — stays within 2.5e-4; emulated on the host in fp32: 6-8e-4
// with one chain, 1.4-2.0e-4 at 2048 vertices, 5-7e-5 at 512, 1.5e-5 at 128 (tests/test_gpu_general_shapes.py)
constexpr int kGenFlushVertices = 512;

__host__ __device__ inline int gen_s4(int S) { return (S + 3) & ~3; }
// dynamic LDS of k_gen_accum (bytes): rows [3 TV][S4] | b [3 TV] | w [3 TV] | R~ [TV][12] | joint ids [TV][KW] | weights [TV][KW]
// + the instance's joint rows (R | T0 | T': J x jd_stride floats) when everything fits: the rows of A are formed from
// them — per element one gather per skinning weight, from global memory 19 ms per launch at B = 4096, S = 32
inline size_t gen_accum_lds_base(int S, int KW) {
  const size_t tv = gen_tile_vertices(S), rows = 3 * tv;
  return (rows * gen_s4(S) + 2 * rows + tv * 12 + 2 * tv * KW) * 4;
}
inline bool gen_accum_stage_joints(int J, int S, int KW) {
  const size_t total = gen_accum_lds_base(S, KW) + (size_t)J * sf::jd_stride(S) * 4;
  return total <= (gen_accum_threads(S) == 64 ? 20 * 1024 : 150 * 1024);  // (one-wave form: eight workgroups per CU — at six, S = 32 lost 25 %)
}
inline size_t gen_accum_lds(int J, int S, int KW) {
  return gen_accum_lds_base(S, KW) + (gen_accum_stage_joints(J, S, KW) ? (size_t)J * sf::jd_stride(S) * 4 : 0);
}

// grid B, block 256.  WEIGHTED: the vertex weights ws.vws enter (else unit weights).
// Inputs: ws.jd (R | T0 | T' rows of the current rotations, k_joint_stage), ws.vposed (B, 3 Vp) instance-major,
// ws.tvs (B, 3, Vp) centred targets at the sorted slots.  Output: ws.gramv (B, NE + 1) doubles.
// (three waves per SIMD: <= 168 registers.  Left to itself hipcc unrolls the row loops completely — 256 + 110 registers,
// ONE workgroup per CU: 22 k fits/s where this form reaches ten times that)
// kGenThreads: 256, or ONE wave for few unknowns (S <= 88: all 4 x 4 blocks of the triangle fit one pass of 64 threads —
// eight such workgroups share a CU where two 256-thread ones would leave most of their lanes idle)
// STAGE: the instance's joint rows are copied to LDS first (a template flag, not a run-time pointer select: with one
// pointer that may be LDS or global every access becomes a FLAT one)
// flush_tiles: every so many tiles the fp32 sums are ADDED to the fp64 record and restart from zero (kGenFlushVertices
// above: one fp32 accumulator per entry over all 3 V rows is a chain of 20 k additions)
template <bool WEIGHTED, int kGenTV, int kGenThreads, bool STAGE>
__global__ __launch_bounds__(kGenThreads, 2) void k_gen_accum(DevModel m, Workspace ws, int B, int flush_tiles) {
  constexpr int kGenRows = 3 * kGenTV;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = m.S, S4 = gen_s4(S), J = m.J, Vp = m.Vp, V = m.V, KW = m.KW;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int stride = sf::jd_stride(S), row = sf::jd_row(S);
  float* rows = smem;                       // [3 TV][S4]
  float* rb = rows + kGenRows * S4;         // [3 TV] residual of the row
  float* rw = rb + kGenRows;                // [3 TV] weight of the row (0: no such vertex)
  float* Rt = rw + kGenRows;                // [TV][12] blended rotation of the vertex
  int* vj = reinterpret_cast<int*>(Rt + kGenTV * 12);  // [TV][KW] joints
  float* vwk = reinterpret_cast<float*>(vj + kGenTV * KW);  // [TV][KW] weights
  const float* jdg = ws.jd + (size_t)b * J * stride;
  float* jds = vwk + kGenTV * KW;  // [J][stride] (STAGE)
  if constexpr (STAGE) {
    for (int k = tid; k < J * stride; k += kGenThreads) jds[k] = jdg[k];
    __syncthreads();
  }
  const auto jd = [&]() {
    if constexpr (STAGE) return (const float*)jds;
    else return jdg;
  }();
  const float* vps = ws.vposed + (size_t)b * 3 * Vp;
  const float* tvs = ws.tvs + (size_t)b * 3 * Vp;
  const float* vws = WEIGHTED ? ws.vws + (size_t)b * Vp : nullptr;
  const int nb4 = S4 / 4, npair = nb4 * (nb4 + 1) / 2, per_pass = kGenThreads * kGenBlk;
  const int npass = (npair + per_pass - 1) / per_pass;
  const int NG = sf::ne_ng(S), NE = sf::ne_size(S);
  double* out = ws.gramv + (size_t)b * (NE + 1);
  const int ntile = (V + kGenTV - 1) / kGenTV;
  for (int pass = 0; pass < npass; ++pass) {
    int bi[kGenBlk], bj[kGenBlk];
#pragma unroll
    for (int k = 0; k < kGenBlk; ++k) {  // block pair p of the upper triangle (row-major over bi <= bj)
      const int p = pass * per_pass + k * kGenThreads + tid;
      bi[k] = -1;
      bj[k] = 0;
      if (p < npair) {
        int i = 0, rem = p;
        while (rem >= nb4 - i) {
          rem -= nb4 - i;
          ++i;
        }
        bi[k] = i;
        bj[k] = i + rem;
      }
    }
    float acc[kGenBlk][16];
#pragma unroll
    for (int k = 0; k < kGenBlk; ++k)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[k][e] = 0.f;
    // pass 0 also: the right-hand side entries r[s] and SA[c][s] of the unknowns s = tid + 256 q; thread 0: Sb and W
    float ar[kGenQ], asa[kGenQ][3], asb[3] = {0.f, 0.f, 0.f}, aw = 0.f;
#pragma unroll
    for (int q = 0; q < kGenQ; ++q) {
      ar[q] = 0.f;
      asa[q][0] = asa[q][1] = asa[q][2] = 0.f;
    }
    // the sums leave the registers for the record: each entry has ONE owner (a thread and a pass), so the additions of a
    // later flush need no atomics.  (The block indices pass through an empty asm: the addresses of a thread's 64 entries
    // do not change from one flush to the next, and hoisted out of the tile loop they are 128 registers — spilled.)
    bool first_flush = true;
    auto flush = [&]() {
      auto put = [&](double* o, float& v) {
        *o = first_flush ? (double)v : *o + (double)v;
        v = 0.f;
      };
#pragma unroll
      for (int k = 0; k < kGenBlk; ++k) {
        if (bi[k] < 0) continue;
        int i0 = 4 * bi[k], j0 = 4 * bj[k];
        asm volatile("" : "+v"(i0), "+v"(j0));
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y) {
            const int i = i0 + x, j = j0 + y;
            if (i <= j && j < S) put(out + sf::ne_g(S, i, j), acc[k][x * 4 + y]);
          }
      }
      if (pass == 0) {
#pragma unroll
        for (int q = 0; q < kGenQ; ++q) {
          const int s2 = tid + kGenThreads * q;
          if (s2 < S) {
            put(out + NG + s2, ar[q]);
#pragma unroll
            for (int c = 0; c < 3; ++c) put(out + NG + S + c * S + s2, asa[q][c]);
          }
        }
        if (tid == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) put(out + NG + 4 * S + c, asb[c]);
          put(out + NE, aw);
        }
      }
      first_flush = false;
    };
    for (int t = 0; t < ntile; ++t) {
      const int v0 = t * kGenTV;
      if (t > 0 && t % flush_tiles == 0) flush();
      __syncthreads();  // (the previous tile's rows have been consumed)
      if (tid < kGenTV) {  // the vertex's skinning pairs, blended rotation, position and residual
        const int i = v0 + tid;
        float R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, T0[3] = {0, 0, 0};
        float w = 0.f, res[3] = {0.f, 0.f, 0.f};
        if (i < V) {
          for (int k = 0; k < KW; ++k) {
            const int j = (m.widx[(size_t)(k >> 2) * Vp + i] >> (8 * (k & 3))) & 0xff;
            const float wk = m.wval[(size_t)k * Vp + i];
            vj[tid * KW + k] = j;
            vwk[tid * KW + k] = wk;
            const float* p = jd + j * stride;
#pragma unroll
            for (int e = 0; e < 9; ++e) R[e] += wk * p[e];
#pragma unroll
            for (int c = 0; c < 3; ++c) T0[c] += wk * p[9 + c];
          }
          const float x[3] = {vps[i], vps[Vp + i], vps[2 * Vp + i]};
#pragma unroll
          for (int c = 0; c < 3; ++c)
            res[c] = tvs[(size_t)c * Vp + i] - ((R[c * 3] * x[0] + R[c * 3 + 1] * x[1] + R[c * 3 + 2] * x[2]) + T0[c]);
          w = WEIGHTED ? vws[i] : 1.f;
        } else {
          for (int k = 0; k < KW; ++k) {
            vj[tid * KW + k] = 0;
            vwk[tid * KW + k] = 0.f;
          }
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) Rt[tid * 12 + e] = R[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          rb[tid * 3 + c] = res[c];
          rw[tid * 3 + c] = w;
        }
      }
      __syncthreads();
      // rows of A: Jac_v[c][s] = sum_c' R~[c][c'] shapedirs_v[c'][s] + sum_k w_k T'_{j_k}[c][s]   (bodyfitter.py:1136-1160)
      // (eight elements per thread at a time, their shape directions requested together: one element after the other
      // the loop is a chain of global-memory round trips — most of the kernel at few unknowns)
      constexpr int U = 8;
      for (int base = tid; base < kGenRows * S4; base += kGenThreads * U) {
        float sdv[U][3];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = base + u * kGenThreads, r = idx / S4, s = idx - r * S4, v = r / 3, i = v0 + v;
          const bool ok = idx < kGenRows * S4 && s < S && i < V;
          const float* sd = m.sdg + (size_t)(ok ? i : 0) * 3 * S4 + (ok ? s : 0);
          sdv[u][0] = ok ? sd[0] : 0.f;
          sdv[u][1] = ok ? sd[S4] : 0.f;
          sdv[u][2] = ok ? sd[2 * S4] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = base + u * kGenThreads;
          if (idx >= kGenRows * S4) break;
          const int r = idx / S4, s = idx - r * S4, v = r / 3, c = r - 3 * v, i = v0 + v;
          float val = 0.f;
          if (s < S && i < V) {
            val = (Rt[v * 12 + c * 3] * sdv[u][0] + Rt[v * 12 + c * 3 + 1] * sdv[u][1]) + Rt[v * 12 + c * 3 + 2] * sdv[u][2];
            const float* tp = jd + 12 + c * row + s;
            for (int k = 0; k < KW; ++k) val += vwk[v * KW + k] * tp[(size_t)vj[v * KW + k] * stride];
          }
          rows[idx] = val;
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kGenBlk; ++k) {
        if (bi[k] < 0) continue;
        const float* pa = rows + 4 * bi[k];
        const float* pb = rows + 4 * bj[k];
#pragma unroll 2
        for (int r = 0; r < kGenRows; ++r) {
          const float w = rw[r];
          const float4 a = *reinterpret_cast<const float4*>(pa + r * S4);
          const float4 c4 = *reinterpret_cast<const float4*>(pb + r * S4);
          const float av[4] = {w * a.x, w * a.y, w * a.z, w * a.w};
          const float cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
          for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[k][x * 4 + y] += av[x] * cv[y];
        }
      }
      if (pass == 0) {
#pragma unroll
        for (int q = 0; q < kGenQ; ++q) {
          const int s2 = tid + kGenThreads * q;
          if (s2 < S)
#pragma unroll 1
            for (int v = 0; v < kGenTV; ++v)  // (rows 3 v + c: the coordinate index stays a compile-time constant)
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                const float wa = rw[3 * v + c] * rows[(3 * v + c) * S4 + s2];
                ar[q] += wa * rb[3 * v + c];
                asa[q][c] += wa;
              }
        }
        if (tid == 0)
#pragma unroll 1
          for (int v = 0; v < kGenTV; ++v) {
#pragma unroll
            for (int c = 0; c < 3; ++c) asb[c] += rw[3 * v + c] * rb[3 * v + c];
            aw += rw[3 * v];
          }
      }
    }
    flush();
  }
}

// Vertices at a given shape + part sums against the targets, lane = vertex of a part-aligned segment (<= 64 slots of ONE
// part), a wave per segment (4 waves walk the list in turn).  grid B, block 256.
// MODE 0: part sums over the used parts (ws.psum).  MODE 1: every slot, also the vertices (sorted SoA, ws.rverts) for
// the joint regression of a joints-omitted fit.  MODE 2: the forward — vertices in ORIGINAL order to out (B, V, 3), shape
// from beta_in (B, nb) / kid_in, translation from trans_in; no targets, no part sums.
// The skinning translations at the shape come from ws.jb (stage S / k_forward_joint).
// Each wave keeps its own rows of part sums in LDS ([4][J][16]), added in wave order at the end: the sums do not
// depend on the timing of the waves.
// NI instances per workgroup: the shape blend reads the WHOLE (3 S, Vp) shape-direction table per instance — 25 MB at S = 300,
// the kernel's time (1.9 ms per launch at B = 256: the table through L2 / MALL once per instance) — so a workgroup blends
// NI instances with every value it loads.
inline int gen_lbs_ni(int S, int B) { return (S >= 48 && B >= 2048) ? 4 : 1; }  // (a small batch needs its workgroups: 256 instances as 64 workgroups ran 15 % slower)
inline size_t gen_lbs_lds(int J, int S, int B) {
  const size_t ni = gen_lbs_ni(S, B);
  return (ni * ((size_t)S + (size_t)J * 12 + 4 * (size_t)J * sf::kPsum + 4)) * 4;
}
template <int MODE, bool WEIGHTED, int NI>
__global__ __launch_bounds__(256) void k_gen_lbs(DevModel m, Workspace ws, int B, int nb, const float* __restrict__ beta_in,
                                                 const float* __restrict__ trans_in, const float* __restrict__ kid_in,
                                                 float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = m.S, J = m.J, Vp = m.Vp, V = m.V, KW = m.KW;
  const int b0 = blockIdx.x * NI, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int stride = sf::jd_stride(S);
  float* sbeta = smem;                      // [NI][S]
  float* jr = sbeta + NI * S;               // [NI][J][12] rotation | skinning translation (+ the instance's translation)
  float* pw = jr + NI * J * 12;             // [NI][4][J][16]
  float* strans = pw + NI * 4 * J * sf::kPsum;  // [NI][3] (+ pad)
  // (the last workgroup of a batch that is no multiple of NI computes its last instance again and stores it once)
  auto inst = [&](int n) { return min(b0 + n, B - 1); };
  if (tid < 3 * NI) strans[tid] = trans_in ? trans_in[(size_t)inst(tid / 3) * 3 + tid % 3] : 0.f;
  for (int k = tid; k < NI * S; k += 256) {
    const int n = k / S, s2 = k - n * S, b = inst(n);
    float v = (beta_in && s2 < nb) ? beta_in[(size_t)b * nb + s2] : 0.f;
    if (kid_in && m.jt.n_kid && s2 == S - 1) v = kid_in[b];
    sbeta[k] = v;
  }
  for (int k = tid; k < NI * 4 * J * sf::kPsum; k += 256) pw[k] = 0.f;
  __syncthreads();
  for (int k = tid; k < NI * J * 12; k += 256) {
    const int n = k / (J * 12), r = k - n * J * 12, j = r / 12, e = r - 12 * j, b = inst(n);
    jr[k] = e < 9 ? ws.jd[((size_t)b * J + j) * stride + e] : ws.jb[((size_t)b * J + j) * 4 + (e - 9)] + strans[n * 3 + e - 9];
  }
  __syncthreads();
  const int32_t* segs = MODE == 0 ? m.segments : m.segall;
  const int nseg = MODE == 0 ? m.nseg : m.nsegall;
  for (int sg = wave; sg < nseg; sg += 4) {
    const int start = segs[sg * 3], count = segs[sg * 3 + 1], part = segs[sg * 3 + 2];
    const bool used = MODE != 2 && start < m.n_used;
    const bool live = lane < count;
    const int i = start + (live ? lane : 0);
    // shape blend: x = v_posed + shapedirs . beta  (coalesced rows of the SoA shapedirs, every value for NI instances)
    float x[NI][3];
#pragma unroll
    for (int n = 0; n < NI; ++n) {
      const float* vps = ws.vposed + (size_t)inst(n) * 3 * Vp;
      x[n][0] = vps[i];
      x[n][1] = vps[Vp + i];
      x[n][2] = vps[2 * Vp + i];
    }
    // (eight unknowns' three rows requested together: one at a time the loop is a chain of L2 round trips — 1.9 ms per
    // launch at S = 300, B = 256)
    {
      constexpr int UB = 8;
      const float* sdp = m.sd + i;
      int s2 = 0;
      for (; s2 + UB <= S; s2 += UB) {
        float d[UB][3];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          d[u][0] = sdp[(size_t)(s2 + u) * Vp];
          d[u][1] = sdp[(size_t)(S + s2 + u) * Vp];
          d[u][2] = sdp[(size_t)(2 * S + s2 + u) * Vp];
        }
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
          for (int n = 0; n < NI; ++n) {
            const float bs = sbeta[n * S + s2 + u];
            x[n][0] += d[u][0] * bs;
            x[n][1] += d[u][1] * bs;
            x[n][2] += d[u][2] * bs;
          }
      }
      for (; s2 < S; ++s2) {
        const float d0 = sdp[(size_t)s2 * Vp], d1 = sdp[(size_t)(S + s2) * Vp], d2 = sdp[(size_t)(2 * S + s2) * Vp];
#pragma unroll
        for (int n = 0; n < NI; ++n) {
          const float bs = sbeta[n * S + s2];
          x[n][0] += d0 * bs;
          x[n][1] += d1 * bs;
          x[n][2] += d2 * bs;
        }
      }
    }
    // the vertex's skinning pairs once for the NI instances
    int vjk[8];
    float vwk8[8];
    const int kw8 = KW < 8 ? KW : 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      vjk[k] = k < kw8 ? (m.widx[(size_t)(k >> 2) * Vp + i] >> (8 * (k & 3))) & 0xff : 0;
      vwk8[k] = k < kw8 ? m.wval[(size_t)k * Vp + i] : 0.f;
    }
#pragma unroll
    for (int n = 0; n < NI; ++n) {
      const int b = inst(n);
      const bool store = b0 + n < B;
      const float* jrn = jr + n * J * 12;
      float R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Tb[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (k < kw8) {
          const float* p = jrn + vjk[k] * 12;
#pragma unroll
          for (int e = 0; e < 9; ++e) R[e] += vwk8[k] * p[e];
#pragma unroll
          for (int c = 0; c < 3; ++c) Tb[c] += vwk8[k] * p[9 + c];
        }
      }
      for (int k = 8; k < KW; ++k) {  // (more than eight skinning weights per vertex)
        const int j = (m.widx[(size_t)(k >> 2) * Vp + i] >> (8 * (k & 3))) & 0xff;
        const float wk = m.wval[(size_t)k * Vp + i];
        const float* p = jrn + j * 12;
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] += wk * p[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) Tb[c] += wk * p[9 + c];
      }
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (R[c * 3] * x[n][0] + R[c * 3 + 1] * x[n][1] + R[c * 3 + 2] * x[n][2]) + Tb[c];
      if (MODE == 2) {
        const int o = m.perm[i];
        if (live && store && o >= 0) {
          out[((size_t)b * V + o) * 3] = v[0];
          out[((size_t)b * V + o) * 3 + 1] = v[1];
          out[((size_t)b * V + o) * 3 + 2] = v[2];
        }
      } else {
        if (MODE == 1 && live && store) {
          float* rv = ws.rverts + (size_t)b * 3 * Vp;
          rv[i] = v[0];
          rv[Vp + i] = v[1];
          rv[2 * Vp + i] = v[2];
        }
        if (used) {
          float acc[sf::kPsum];
#pragma unroll
          for (int k = 0; k < sf::kPsum; ++k) acc[k] = 0.f;
          if (live) {
            const float* tvs = ws.tvs + (size_t)b * 3 * Vp;
            const float tv[3] = {tvs[i], tvs[Vp + i], tvs[2 * Vp + i]};
            sf::partsum_vertex(tv, v, WEIGHTED ? ws.vws[(size_t)b * Vp + i] : 1.f, WEIGHTED, acc);
          }
          float* ps = pw + (((size_t)n * 4 + wave) * J + part) * sf::kPsum;
#pragma unroll
          for (int k = 0; k < sf::kPsum; ++k) {
            const float r = wave_sum_last(acc[k]);
            if (lane == 63) ps[k] += r;
          }
        }
      }
    }
  }
  if (MODE == 1)  // padding slots of the regression source
    for (int k = tid; k < NI * (Vp - V); k += 256) {
      const int n = k / (Vp - V), i = V + (k - n * (Vp - V));
      if (b0 + n < B) {
        float* rv = ws.rverts + (size_t)(b0 + n) * 3 * Vp;
        rv[i] = 0.f;
        rv[Vp + i] = 0.f;
        rv[2 * Vp + i] = 0.f;
      }
    }
  if (MODE != 2) {
    __syncthreads();
    for (int k = tid; k < NI * J * sf::kPsum; k += 256) {
      const int n = k / (J * sf::kPsum), r = k - n * J * sf::kPsum;
      const float* p = pw + (size_t)n * 4 * J * sf::kPsum + r;
      if (b0 + n < B)
        ws.psum[(size_t)(b0 + n) * J * sf::kPsum + r] = ((p[0] + p[J * sf::kPsum]) + p[2 * J * sf::kPsum]) + p[3 * J * sf::kPsum];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// k_gen_accum on the matrix cores (round 5): the vertex block of the normal equations as ONE symmetric rank-k update
// G~ += A~^T diag(w) A~ over the rows of the design matrix, with the columns
//     A~ = [ Jac (S unknowns) | b | 1_x 1_y 1_z | t ]
// (b: residual of the row, 1_c: the row is coordinate c of an existing vertex, t: the centred target) — so that EVERY sum
// of the record is an entry of G~:  G = G~[s][s'],  r = G~[s][b],  SA[c] = G~[s][1_c],  Sb[c] = G~[b][1_c],
// W = G~[1_x][1_x], and the extra sums of the scale unknown (scaled_solve_stage): u = G~[s][t], tt = G~[t][t],
// tb = G~[b][t], bb = G~[b][b], St[c] = G~[1_c][t].  The reference forms A (B, 3V + 3J, S) in memory and calls a dense
// fp32 product (pt/bodyfitter.py:1136-1200, pt/lstsq.py); here a workgroup forms 24 or 96 rows at a time in LDS,
// and its waves hold the upper-triangle 32 x 32 blocks of G~ in accumulators, v_mfma_f32_32x32x2_f32 (fp32 products
// and sums, as the VALU form above).  S = 300: 55 blocks over eight waves, seven each; more unknowns: the
// blocks are split over gridDim.y workgroups per instance, each forming the rows it needs itself (forming a vertex's
// three rows is 9 S multiply-adds, its share of the update 3 x 1024 per block).
// Per 64 vertices one pass of 64 threads blends the rotations and evaluates the residuals (the chain of dependent
// gathers is paid once per 64 vertices instead of once per tile).
// grid (B, groups), block 64 NW.  NBW: blocks per wave.
// ------------------------------------------------------------------------------------------------
constexpr int kGen2Extra = 5;  // columns beside the unknowns
inline int gen2_nb(int S) { return (S + kGen2Extra + 31) / 32; }
// workgroup shapes (waves, blocks per wave, vertices per tile): few unknowns (S + 5 <= 64: three blocks) 4 x 1, 32;
// up to 160 columns (15 blocks) 16 x 1, 32; beyond 8 x 7, 8 — S = 300: 55 blocks in ONE workgroup, seven per wave (their
// accumulators are 112 of a wave's 256 registers; sixteen waves of four blocks leave 128 registers in
// all and the compiler spills accumulators inside the product loop: measured 8.2 ms against 7.9, then 69 ms)
inline int gen2_nw(int S) { return gen2_nb(S) <= 2 ? 4 : gen2_nb(S) <= 5 ? 16 : 8; }
inline int gen2_nbw(int S) { return gen2_nb(S) <= 5 ? 1 : 7; }
inline int gen2_tv(int S) { return gen2_nbw(S) >= 4 ? 8 : 32; }
inline int gen2_sv(int S) { return gen2_tv(S) == 8 ? 64 : 128; }  // vertices per blend pass
inline int gen2_groups(int S) {
  const int nb = gen2_nb(S), T = nb * (nb + 1) / 2, per = gen2_nw(S) * gen2_nbw(S);
  return (T + per - 1) / per;
}
// row pitch of the tile (floats): 32 nb columns, odd multiple of 32 — the two rows a matrix-core operand read touches
// (lanes 0-31 one row, 32-63 the next) then fall into disjoint halves of the 64 LDS banks
__host__ __device__ inline int gen2_ld(int S) {
  const int nb = (S + kGen2Extra + 31) / 32;
  return 32 * (nb | 1);
}
inline size_t gen2_lds_base(int S, int KW) {
  const size_t rows = 3 * gen2_tv(S), sv = gen2_sv(S);
  return (rows * gen2_ld(S) + sv * (9 + 4 * 3) + 2 * sv * KW) * 4;
}
// the instance's joint rows in LDS too when the workgroups a CU can hold otherwise still fit (16 waves: one; 4 waves: three)
inline bool gen2_stage_joints(int J, int S, int KW) {
  const size_t total = gen2_lds_base(S, KW) + (size_t)J * sf::jd_stride(S) * 4;
  return total <= (size_t)(gen2_nw(S) >= 8 ? 160 : 52) * 1024;
}
inline size_t gen2_lds(int J, int S, int KW) {
  return gen2_lds_base(S, KW) + (gen2_stage_joints(J, S, KW) ? (size_t)J * sf::jd_stride(S) * 4 : 0);
}

template <bool WEIGHTED, int NW, int NBW, bool STAGE>
__global__ __launch_bounds__(64 * NW) void k_gen_accum_mfma(DevModel m, Workspace ws, int B, double* __restrict__ vextra, int flush_every,
                                                           const float* __restrict__ tj, const float* __restrict__ jw) {
  constexpr int NT = 64 * NW, TV = NBW >= 4 ? 8 : 32, R = 3 * TV, SV = TV == 8 ? 64 : 128;
  // a thread forms the rows of QUADS — (vertex, four consecutive unknowns): the shape directions and the T' rows are 16-byte
  // loads — and requests the shape directions of its first U quads a tile ahead (every quad up to 340 unknowns)
  constexpr int U = 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = m.S, J = m.J, Vp = m.Vp, V = m.V, KW = m.KW;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, h = lane >> 5, c32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int stride = sf::jd_stride(S), row = sf::jd_row(S);
  const int nb = (S + kGen2Extra + 31) >> 5, T = nb * (nb + 1) / 2;
  const int LD = gen2_ld(S);
  float* AT = smem;                        // [R][LD]  the tile's rows of A~
  float* Rt = AT + (size_t)R * LD;         // [SV][9] blended rotation of the vertex
  float* rb = Rt + SV * 9;                 // [3 SV] residual of the row
  float* rw = rb + SV * 3;                 // [3 SV] weight of the row
  float* rt = rw + SV * 3;                 // [3 SV] target of the row
  float* r1 = rt + SV * 3;                 // [3 SV] 1: the row's vertex exists
  int* vj = reinterpret_cast<int*>(r1 + SV * 3);            // [SV][KW] joints
  float* vwk = reinterpret_cast<float*>(vj + SV * KW);      // [SV][KW] weights
  float* jds = vwk + SV * KW;                               // [J][stride] (STAGE)
  const float* jdg = ws.jd + (size_t)b * J * stride;
  for (int k = tid; k < R * LD; k += NT) AT[k] = 0.f;  // (the padding columns stay zero)
  if constexpr (STAGE)
    for (int k = tid; k < J * stride; k += NT) jds[k] = jdg[k];
  const auto jd = [&]() {
    if constexpr (STAGE) return (const float*)jds;
    else return jdg;
  }();
  // this wave's blocks of the upper triangle (row-major over I <= J), a contiguous run of the workgroup's share
  const int per_wg = (T + (int)gridDim.y - 1) / (int)gridDim.y, per_wave = (per_wg + NW - 1) / NW;
  const int wg_end = min(((int)blockIdx.y + 1) * per_wg, T);
  const int first = (int)blockIdx.y * per_wg + wave * per_wave;
  const int nblk = max(0, min(min(first + per_wave, wg_end) - first, NBW));
  int bI[NBW], bJ[NBW];
#pragma unroll
  for (int k = 0; k < NBW; ++k) {  // block first + k of the triangle
    int i = 0, rem = first + k;
    while (i < nb - 1 && rem >= nb - i) {
      rem -= nb - i;
      ++i;
    }
    bI[k] = i;
    bJ[k] = min(i + rem, nb - 1);
  }
  // operand offsets of the blocks within a pair of tile rows (slots beyond nblk: the last block again)
  int offI[NBW], offJ[NBW];
#pragma unroll
  for (int k = 0; k < NBW; ++k) {
    const int kc = k < nblk ? k : (nblk > 0 ? nblk - 1 : 0);
    int oi = 0, oj = 0;
#pragma unroll
    for (int k2 = 0; k2 < NBW; ++k2)
      if (k2 == kc) {
        oi = bI[k2];
        oj = bJ[k2];
      }
    offI[k] = h * LD + oi * 32 + c32;
    offJ[k] = h * LD + oj * 32 + c32;
  }
  f32x16 acc[NBW];
#pragma unroll
  for (int k = 0; k < NBW; ++k)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[k][e] = 0.f;
  const float* vps = ws.vposed + (size_t)b * 3 * Vp;
  const float* tvs = ws.tvs + (size_t)b * 3 * Vp;
  const float* vws = WEIGHTED ? ws.vws + (size_t)b * Vp : nullptr;
  const int nq = (S + 3) >> 2, nquads = nq * TV, S4 = 4 * nq;
  const float invq = 1.0f / (float)nq;
  // quad idx of the tile at v0: vertex idx / nq, unknowns 4 (idx % nq) ...; its shape directions (3 x 4)
  // (no select on the loaded values — an out-of-range quad reads vertex 0 / unknown 0 and is never used: with a select
  // the compiler waits for the loads where they are issued, and the request a tile ahead hides nothing)
  auto load_quad = [&](int idx, int v0, float4 (&sd)[3]) {
    const int v = min((int)(((float)idx + 0.5f) * invq), TV - 1), s0 = 4 * (idx - v * nq), i = v0 + v;
    const bool ok = idx < nquads && i < V;
    const float4* p = reinterpret_cast<const float4*>(m.sdg + (size_t)(ok ? i : 0) * 3 * S4 + (ok ? s0 : 0));
#pragma unroll
    for (int c = 0; c < 3; ++c) sd[c] = p[c * nq];  // (rows of S4 = 4 nq floats)
  };
  // the rows Jac_v[c][s] = sum_c' R~[c][c'] shapedirs_v[c'][s] + sum_k w_k T'_{j_k}[c][s] of a quad into the tile
  auto form_quad = [&](int idx, int v0, int ti, const float4 (&sd)[3]) {
    const int v = min((int)(((float)idx + 0.5f) * invq), TV - 1), s0 = 4 * (idx - v * nq), lv = ti * TV + v;
    float4 val[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float r0 = Rt[lv * 9 + c * 3], r1 = Rt[lv * 9 + c * 3 + 1], r2 = Rt[lv * 9 + c * 3 + 2];
      val[c].x = (r0 * sd[0].x + r1 * sd[1].x) + r2 * sd[2].x;
      val[c].y = (r0 * sd[0].y + r1 * sd[1].y) + r2 * sd[2].y;
      val[c].z = (r0 * sd[0].z + r1 * sd[1].z) + r2 * sd[2].z;
      val[c].w = (r0 * sd[0].w + r1 * sd[1].w) + r2 * sd[2].w;
    }
    for (int k = 0; k < KW; ++k) {
      const float wk = vwk[lv * KW + k];
      const float* tp = jd + (size_t)vj[lv * KW + k] * stride + 12 + s0;  // (rows padded to a multiple of four)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float4 t4 = *reinterpret_cast<const float4*>(tp + c * row);
        val[c].x += wk * t4.x;
        val[c].y += wk * t4.y;
        val[c].z += wk * t4.z;
        val[c].w += wk * t4.w;
      }
    }
    const bool live = v0 + v < V;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = AT + (size_t)(3 * v + c) * LD + s0;
      if (!live) val[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (s0 + 3 < S) {
        *reinterpret_cast<float4*>(o) = val[c];
      } else {  // (the last quad of a row count that is no multiple of four: the columns beside the unknowns follow)
        o[0] = val[c].x;
        if (s0 + 1 < S) o[1] = val[c].y;
        if (s0 + 2 < S) o[2] = val[c].z;
      }
    }
  };
  float4 sdv[U][3];
  auto request = [&](int v0) {
#pragma unroll
    for (int u = 0; u < U; ++u) load_quad(tid + u * NT, v0, sdv[u]);
  };
  // ---- the update: a k-step is two rows of the tile (lanes 0-31 the even one, 32-63 the odd one); rwt: the rows' weights
  auto update = [&](const float* rwt) {
    if (nblk == 0) return;
    // the operands of k-step kk + 1 are requested before the products of k-step kk are issued (two register sets; the
    // scheduling barriers keep the compiler from sinking every read next to its product again: read, wait, product, seven
    // times per k-step, was what it made of the plain loop); a wave with fewer than NBW blocks repeats its last one into
    // a spare accumulator
    float fa[2][NBW], fb[2][NBW];
    auto load = [&](int set, int kk) {
      const float* rowp = AT + (size_t)(2 * kk) * LD;
#pragma unroll
      for (int k = 0; k < NBW; ++k) {
        fa[set][k] = rowp[offI[k]];
        fb[set][k] = rowp[offJ[k]];
      }
      if (WEIGHTED) {
        const float w = rwt[2 * kk + h];
#pragma unroll
        for (int k = 0; k < NBW; ++k) fb[set][k] *= w;
      }
    };
    auto products = [&](int set) {
#pragma unroll
      for (int k = 0; k < NBW; ++k) acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][k], fb[set][k], acc[k], 0, 0, 0);
    };
    load(0, 0);
#pragma unroll 1
    for (int kk = 0; kk < R / 2; kk += 2) {  // (R / 2 is even)
      load(1, kk + 1);
      __builtin_amdgcn_sched_barrier(0);
      products(0);
      __builtin_amdgcn_sched_barrier(0);
      if (kk + 2 < R / 2) load(0, kk + 2);
      __builtin_amdgcn_sched_barrier(0);
      products(1);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // ---- the entries leave the accumulators for the record (and the scale unknown's extra sums), as fp64 sums of fp32
  // partial sums: every flush_every blend passes (64 / 128 vertices each) the accumulators are ADDED to the record and
  // restart from zero.  One fp32 accumulator per entry over all 3 V rows is a chain of 20 k additions: good for the
  // plain fit on ordinary targets (2e-5 m), not for the betas of hard ones (kGenFlushVertices) nor for the scale
  // unknown, whose column is nearly a combination of the others — scale_corr 2.3e-4 from the fp64 evaluation where the
  // reference's own fp32 is within 1e-4; a scaled iteration flushes after every pass (the sums of <= 128 vertices, as
  // the lanes of the other paths' kernels keep them).
  const int NG = sf::ne_ng(S), NE = sf::ne_size(S);
  double* out = ws.gramv + (size_t)b * (NE + 1);
  double* vex = vextra ? vextra + (size_t)b * (S + sf::kScaleExtras) : nullptr;
  bool first_flush = true;
  auto store_entry = [&](int i, int j, float v) {
    if (i > j || j >= S + kGen2Extra) return;
    double* o = nullptr;
    if (j < S) {
      o = out + sf::ne_g(S, i, j);
    } else if (j == S) {
      if (i < S) o = out + NG + i;
      else if (vex) o = vex + S + 2;  // bb
    } else if (j <= S + 3) {
      const int c = j - S - 1;
      if (i < S) o = out + NG + S + c * S + i;
      else if (i == S) o = out + NG + 4 * S + c;
      else if (i == S + 1 && c == 0) o = out + NE;
    } else if (vex) {  // the target column
      if (i < S) o = vex + i;                              // u
      else if (i == S) o = vex + S + 1;                    // tb
      else if (i <= S + 3) o = vex + S + 3 + (i - S - 1);  // St
      else o = vex + S;                                    // tt
    }
    if (o) *o = first_flush ? (double)v : *o + (double)v;
  };
  // (through 2 KB of LDS per wave, lane-private, eight registers at a time: with every store of a wave written out —
  // 112 copies of store_entry per call site — the compiler gives up unrolling and the accumulators live in scratch:
  // 162 ms per launch instead of 7.  The tile memory is free between the barrier that ends a tile and the next blend
  // pass; the slots are zeroed again: the tile's padding columns must stay zero.)
  auto flush = [&]() {
    float* mine = smem + wave * 512 + lane;
#pragma unroll
    for (int k = 0; k < NBW; ++k) {
      if (k < nblk) {
#pragma unroll
        for (int c8 = 0; c8 < 2; ++c8) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            mine[e * 64] = acc[k][c8 * 8 + e];
            acc[k][c8 * 8 + e] = 0.f;
          }
#pragma unroll 1
          for (int e = 0; e < 8; ++e) {
            const int ee = c8 * 8 + e;
            store_entry(bI[k] * 32 + (ee & 3) + 8 * (ee >> 2) + 4 * h, bJ[k] * 32 + c32, mine[e * 64]);
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) mine[e * 64] = 0.f;
    first_flush = false;
  };
  int since_flush = 0;
  request(0);
  __syncthreads();
  for (int sv0 = 0; sv0 < V; sv0 += SV) {
    if (tid < SV) {  // the vertex's skinning pairs, blended rotation, residual (bodyfitter.py:1136-1160)
      const int i = sv0 + tid;
      float Rv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, T0[3] = {0, 0, 0};
      float w = 0.f, one = 0.f, res[3] = {0.f, 0.f, 0.f}, tg[3] = {0.f, 0.f, 0.f};
      if (i < V) {
        for (int k = 0; k < KW; ++k) {
          const int j = (m.widx[(size_t)(k >> 2) * Vp + i] >> (8 * (k & 3))) & 0xff;
          const float wk = m.wval[(size_t)k * Vp + i];
          vj[tid * KW + k] = j;
          vwk[tid * KW + k] = wk;
          const float* p = jd + j * stride;
#pragma unroll
          for (int e = 0; e < 9; ++e) Rv[e] += wk * p[e];
#pragma unroll
          for (int c = 0; c < 3; ++c) T0[c] += wk * p[9 + c];
        }
        const float x[3] = {vps[i], vps[Vp + i], vps[2 * Vp + i]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          tg[c] = tvs[(size_t)c * Vp + i];
          res[c] = tg[c] - ((Rv[c * 3] * x[0] + Rv[c * 3 + 1] * x[1] + Rv[c * 3 + 2] * x[2]) + T0[c]);
        }
        w = WEIGHTED ? vws[i] : 1.f;
        one = 1.f;
      } else {
        for (int k = 0; k < KW; ++k) {
          vj[tid * KW + k] = 0;
          vwk[tid * KW + k] = 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 9; ++e) Rt[tid * 9 + e] = Rv[e];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        rb[tid * 3 + c] = res[c];
        rw[tid * 3 + c] = w;
        rt[tid * 3 + c] = tg[c];
        r1[tid * 3 + c] = one;
      }
    }
    __syncthreads();
    for (int ti = 0; ti < SV / TV; ++ti) {
      const int v0 = sv0 + ti * TV;
      if (v0 >= V) break;
      // ---- the tile's rows
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (tid + u * NT < nquads) form_quad(tid + u * NT, v0, ti, sdv[u]);
      for (int idx = tid + U * NT; idx < nquads; idx += NT) {  // (quads beyond the requested ones)
        float4 sd[3];
        load_quad(idx, v0, sd);
        form_quad(idx, v0, ti, sd);
      }
      if (tid < R) {  // the five columns beside the unknowns
        const int r = tid, c = r % 3, l3 = ti * R + r;
        float* o = AT + (size_t)r * LD + S;
        o[0] = rb[l3];
        const float one = r1[l3];
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2) o[1 + c2] = c2 == c ? one : 0.f;
        o[4] = rt[l3];
      }
      __syncthreads();
      request(v0 + TV);  // (past the last vertex: nothing is read)
      update(rw + ti * R);
      __syncthreads();
    }
    if (++since_flush == flush_every && sv0 + SV < V) {
      flush();
      since_flush = 0;
    }
  }
  // ---- the target joints are further rows of the design matrix (bodyfitter.py:1161-1170: target_both = cat(vertices,
  // joints)): row (j, c) = P'_j[c][s] of the joint stage, residual t_j - P0_j, weight jw_j — the joint block of the
  // normal equations, which the other paths take from k_joint_stage (3 J serial rows per entry: 5 ms at S = 300)
  if (tj) {
    const int S1 = S + 1;
    const float* P = ws.pext + (size_t)b * J * 3 * S1;
    const float* tjb = tj + (size_t)b * J * 3;
    for (int j0 = 0; j0 < J; j0 += TV) {
      for (int idx = tid; idx < S * TV; idx += NT) {
        const int v = min((int)(((float)idx + 0.5f) / (float)S), TV - 1), s = idx - v * S, j = j0 + v;
#pragma unroll
        for (int c = 0; c < 3; ++c) AT[(size_t)(3 * v + c) * LD + s] = j < J ? P[(size_t)(j * 3 + c) * S1 + 1 + s] : 0.f;
      }
      if (tid < R) {
        const int r = tid, c = r % 3, j = j0 + r / 3;
        const bool ok = j < J;
        const float tq = ok ? tjb[j * 3 + c] : 0.f, p0 = ok ? P[(size_t)(j * 3 + c) * S1] : 0.f;
        float* o = AT + (size_t)r * LD + S;
        o[0] = tq - p0;
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2) o[1 + c2] = (c2 == c && ok) ? 1.f : 0.f;
        o[4] = tq;
        rw[r] = ok ? (jw ? jw[(size_t)b * J + j] : 1.f) : 0.f;
      }
      __syncthreads();
      update(rw);
      __syncthreads();
    }
  }
  flush();
}
