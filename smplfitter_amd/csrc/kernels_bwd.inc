// Backward of BodyModel.forward (smplfit_forward_backward_f32): the vector-Jacobian product of smplfit_forward_ex_f32.
// Included by smplfit_hip.hip (same anonymous namespace).  DESIGN.md §12.
//
//   k_forward_joint + posedirs GEMM   recompute: the (G | t) joint block and v_posed (instance-major ws.vposed)
//   k_bwd_vertex      grid B, block 256: per instance, one read of grad_vertices; dv_posed = (sum_k w_vk G_k)^T g_v in
//                     slot order, dA_k = sum_v w_vk g_v (x) [v_posed_v, 1] and sum_v g_v.  Per-joint sums: each wave
//                     owns a row of LDS sums that it adds to in segment order; the four rows are added in wave order.
//   k_obj_vertex      the same pass for smplfit_mesh_objective_f32: g_v is not read but computed from the skinned vertex
//                     and the target (the vertex and its cotangent stay in registers), plus the instance's loss
//   k_bwd_reduce      split-K over workgroups: [dfeat | dshape] (B, P + S) = dv_posed (B, 3 Vp) . [posedirs | shapedirs]^T,
//                     partial rows per K chunk; k_bwd_combine adds the chunks in chunk order
//   k_obj_joint       lane = instance, smplfit_fit_objective_f32 only: the joint term of the objective from the posed
//                     pass's joints, its (B, J, 3) cotangent for k_bwd_joint, the instance's joint loss added to loss[b]
//   k_bwd_joint       lane = instance: sf::forward_joint_backward (reverse FK chain, J_shapedirs, Rodrigues)
// No float atomics: every sum has a fixed order, the results are bitwise run-to-run deterministic.

constexpr int kBwdTile = 64;   // rows (instances) x columns of a k_bwd_reduce workgroup
constexpr int kBwdKStep = 16;  // k per LDS stage
constexpr int kBwdKChunk = 1024;  // k per workgroup (split-K)

// extra workspace of the backward, carved behind the forward's (smplfit_forward_backward_workspace_bytes)
struct BwdWorkspace {
  float* dvp;    // (B, 3 Vp) dv_posed at the sorted slots, SoA per instance (padding slots 0)
  float* dA;     // (B, J, 12)
  float* dtv;    // (B, 3) sum_v g_v
  float* part;   // (nsplit, B, P + S) partial rows of k_bwd_reduce
  float* dfeat;  // (B, P + S)
  float* jscr;   // (B, joint_bwd_scratch_floats(J))
};

inline int bwd_nsplit(int Vp) { return (3 * Vp + kBwdKChunk - 1) / kBwdKChunk; }

// The mesh-distance objective of k_obj_vertex (smplfit_mesh_objective_f32)
struct ObjArgs {
  const float* target;  // (B, V, 3)
  const float* vw;      // (B, V) or NULL
  const float* trans;   // (B, 3) or NULL
  float scale;
  float* loss;          // (B)
};

inline size_t bwd_vertex_lds_bytes(const DevModel& d, bool obj) {
  return ((size_t)d.J * 9 + d.S + 4 * (size_t)d.J * 12 + 12 + (obj ? 4 + (size_t)d.J * 3 : 0)) * 4;
}

// The vertex pass of one instance (a workgroup of 4 waves; a wave walks the part-aligned 64-slot tiles segall[w],
// segall[w + 4], ...).  OBJ = false: the cotangent g_v is read from gv (B, V, 3).  OBJ = true: it is computed: the
// skinned vertex M x + sum_k w_k T_k + trans is built here from the blended rotation, the rest vertex and the joint
// translations (jd floats 9..11, sf_stages.h), compared with the target, and sf::mesh_objective_vertex gives the loss
// term and g_v; the instance's loss is summed per wave in segment order, the four waves in wave order.
template <bool OBJ>
__device__ __forceinline__ void bwd_vertex_body(const DevModel& m, const Workspace& ws, const BwdWorkspace& bw, int nb,
                                                const float* __restrict__ beta_in, const float* __restrict__ kid_in,
                                                const float* __restrict__ gv, const ObjArgs& oa) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = m.S, J = m.J, Vp = m.Vp, V = m.V, KW = m.KW;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int stride = sf::jd_stride(S);
  float* sG = smem;              // [J][9]
  float* sbeta = sG + J * 9;     // [S]
  float* acc = sbeta + S;        // [4][J][12]
  float* acct = acc + 4 * J * 12;  // [4][3]
  float* accl = acct + 12;         // [4] loss per wave        (OBJ)
  float* sT = accl + 4;            // [J][3] joint translations (OBJ)
  for (int k = tid; k < J * 9; k += 256) sG[k] = ws.jd[((size_t)b * J + k / 9) * stride + k % 9];
  if constexpr (OBJ)
    for (int k = tid; k < J * 3; k += 256) sT[k] = ws.jd[((size_t)b * J + k / 3) * stride + 9 + k % 3];
  for (int s = tid; s < S; s += 256) {
    float v = (beta_in && s < nb) ? beta_in[(size_t)b * nb + s] : 0.f;
    if (kid_in && m.jt.n_kid && s == S - 1) v = kid_in[b];
    sbeta[s] = v;
  }
  for (int k = tid; k < 4 * J * 12 + 12; k += 256) acc[k] = 0.f;
  float* dvp = bw.dvp + (size_t)b * 3 * Vp;
  for (int i = V + tid; i < Vp; i += 256) dvp[i] = dvp[Vp + i] = dvp[2 * Vp + i] = 0.f;
  __syncthreads();
  const float* vps = ws.vposed + (size_t)b * 3 * Vp;
  float* aw = acc + wave * J * 12;
  float tsum[3] = {0.f, 0.f, 0.f};
  float lsum = 0.f, tr[3] = {0.f, 0.f, 0.f};
  if constexpr (OBJ)
    if (oa.trans)
      for (int c = 0; c < 3; ++c) tr[c] = oa.trans[(size_t)b * 3 + c];
  for (int sg = wave; sg < m.nsegall; sg += 4) {
    const int start = m.segall[sg * 3], count = m.segall[sg * 3 + 1];
    const bool live = lane < count;
    const int i = start + (live ? lane : 0);
    float x[3] = {vps[i], vps[Vp + i], vps[2 * Vp + i]};
    for (int s = 0; s < S; ++s) {
      const float bs = sbeta[s];
      x[0] += m.sd[(size_t)s * Vp + i] * bs;
      x[1] += m.sd[(size_t)(S + s) * Vp + i] * bs;
      x[2] += m.sd[(size_t)(2 * S + s) * Vp + i] * bs;
    }
    float g[3] = {0.f, 0.f, 0.f};
    if constexpr (!OBJ)
      if (live) {
        const int o = m.perm[i];
        for (int c = 0; c < 3; ++c) g[c] = gv[((size_t)b * V + o) * 3 + c];
      }
    // blended rotation and the joints this tile touches (64-bit mask, OR over the wave)
    float M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    float Tb[3] = {0.f, 0.f, 0.f};
    uint64_t mask = 0;
    for (int k = 0; k < KW; ++k) {
      const int j = (m.widx[(size_t)(k >> 2) * Vp + i] >> (8 * (k & 3))) & 0xff;
      const float w = live ? m.wval[(size_t)k * Vp + i] : 0.f;
      if (w != 0.f) mask |= (uint64_t)1 << j;
#pragma unroll
      for (int e = 0; e < 9; ++e) M[e] += w * sG[j * 9 + e];
      if constexpr (OBJ)
#pragma unroll
        for (int c = 0; c < 3; ++c) Tb[c] += w * sT[j * 3 + c];
    }
    if constexpr (OBJ)
      if (live) {
        const size_t o = (size_t)b * V + m.perm[i];
        float v[3], t[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[c] = (M[c * 3] * x[0] + M[c * 3 + 1] * x[1] + M[c * 3 + 2] * x[2]) + Tb[c] + tr[c];
          t[c] = oa.target[o * 3 + c];
        }
        lsum += sf::mesh_objective_vertex(v, t, oa.vw ? oa.scale * oa.vw[o] : oa.scale, g);
      }
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)mask, o, 64), hi = __shfl_xor((uint32_t)(mask >> 32), o, 64);
      mask |= ((uint64_t)hi << 32) | lo;
    }
    if (live)
#pragma unroll
      for (int d = 0; d < 3; ++d) dvp[d * Vp + i] = M[d] * g[0] + M[3 + d] * g[1] + M[6 + d] * g[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) tsum[c] += g[c];
    while (mask) {  // (wave-uniform)
      const int j = __builtin_ctzll(mask);
      mask &= mask - 1;
      float w = 0.f;
      for (int k = 0; k < KW; ++k) {
        const int jk = (m.widx[(size_t)(k >> 2) * Vp + i] >> (8 * (k & 3))) & 0xff;
        if (jk == j && live) w += m.wval[(size_t)k * Vp + i];
      }
      float v[12];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float wg = w * g[c];
#pragma unroll
        for (int d = 0; d < 3; ++d) v[c * 3 + d] = wg * x[d];
        v[9 + c] = wg;
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) v[e] = wave_sum(v[e]);
      if (lane == 0)
#pragma unroll
        for (int e = 0; e < 12; ++e) aw[j * 12 + e] += v[e];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) tsum[c] = wave_sum(tsum[c]);
  if (lane == 0)
    for (int c = 0; c < 3; ++c) acct[wave * 3 + c] = tsum[c];
  if constexpr (OBJ) {
    lsum = wave_sum(lsum);
    if (lane == 0) accl[wave] = lsum;
  }
  __syncthreads();
  for (int k = tid; k < J * 12; k += 256)
    bw.dA[(size_t)b * J * 12 + k] = ((acc[k] + acc[J * 12 + k]) + acc[2 * J * 12 + k]) + acc[3 * J * 12 + k];
  if (tid < 3) bw.dtv[b * 3 + tid] = ((acct[tid] + acct[3 + tid]) + acct[6 + tid]) + acct[9 + tid];
  if constexpr (OBJ)
    if (tid == 0) oa.loss[b] = ((accl[0] + accl[1]) + accl[2]) + accl[3];
}

// grid B, block 256
__global__ __launch_bounds__(256) void k_bwd_vertex(DevModel m, Workspace ws, BwdWorkspace bw, int B, int nb,
                                                    const float* __restrict__ beta_in, const float* __restrict__ kid_in,
                                                    const float* __restrict__ gv) {
  bwd_vertex_body<false>(m, ws, bw, nb, beta_in, kid_in, gv, ObjArgs{});
}

// grid B, block 256: the same pass with the cotangent of the mesh-distance objective computed in registers
__global__ __launch_bounds__(256) void k_obj_vertex(DevModel m, Workspace ws, BwdWorkspace bw, int B, int nb,
                                                    const float* __restrict__ beta_in, const float* __restrict__ kid_in,
                                                    ObjArgs oa) {
  bwd_vertex_body<true>(m, ws, bw, nb, beta_in, kid_in, nullptr, oa);
}

// grid (ceil(NC / 64), ceil(B / 64), nsplit), block 256: a 64 x 64 tile of the partial product of K chunk z, 4 x 4
// outputs per thread.  Column q < P: posedirs feature q (pdSw holds posedirs^T as (3 Vp, Kp), features in rp_pos
// order); q in [P, P + S): shapedirs column q - P (sd: (3 S, Vp), row c * S + s).
__global__ __launch_bounds__(256) void k_bwd_reduce(DevModel m, BwdWorkspace bw, int B) {
  __shared__ float sa[kBwdKStep][kBwdTile + 4];
  __shared__ float sb[kBwdKStep][kBwdTile + 4];
  const int S = m.S, P = m.P, Kp = m.Kp, Vp = m.Vp, N = 3 * Vp, NC = P + S;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int q0 = blockIdx.x * kBwdTile, b0 = blockIdx.y * kBwdTile, z = blockIdx.z;
  const int k_begin = z * kBwdKChunk, k_end = min(N, k_begin + kBwdKChunk);
  float c[4][4] = {};
  for (int k0 = k_begin; k0 < k_end; k0 += kBwdKStep) {
    for (int e = tid; e < kBwdKStep * kBwdTile; e += 256) {
      const int kk = e % kBwdKStep, r = e / kBwdKStep, n = k0 + kk, b = b0 + r;
      sa[kk][r] = (n < k_end && b < B) ? bw.dvp[(size_t)b * N + n] : 0.f;
    }
    for (int e = tid; e < kBwdKStep * kBwdTile; e += 256) {
      const int qq = e % kBwdTile, kk = e / kBwdTile, n = k0 + kk, q = q0 + qq;
      float v = 0.f;
      if (n < k_end && q < NC) {
        if (q < P) v = m.pdSw[(size_t)n * Kp + sf::rp_pos(q, Kp)];
        else {
          const int cc = n / Vp, vv = n - cc * Vp;
          v = m.sd[(size_t)(cc * S + (q - P)) * Vp + vv];
        }
      }
      sb[kk][qq] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kBwdKStep; ++kk) {
      float a[4], bb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = sa[kk][ty * 4 + u];
        bb[u] = sb[kk][tx * 4 + u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w) c[u][w] += a[u] * bb[w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int b = b0 + ty * 4 + u;
    if (b >= B) continue;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int q = q0 + tx * 4 + w;
      if (q < NC) bw.part[((size_t)z * B + b) * NC + q] = c[u][w];
    }
  }
}

// grid ceil(B * NC / 256), block 256: the K chunks' partial rows added in chunk order
__global__ __launch_bounds__(256) void k_bwd_combine(BwdWorkspace bw, int B, int NC, int nsplit) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)B * NC;
  if (e >= n) return;
  float s = 0.f;
  for (int z = 0; z < nsplit; ++z) s += bw.part[(size_t)z * n + e];
  bw.dfeat[e] = s;
}

// The joint term of smplfit_fit_objective_f32 (k_obj_joint)
struct ObjJointArgs {
  const float* rjoints;  // (B, J, 3) joints of the posed pass, without trans (ws.rjoints)
  const float* trans;    // (B, 3) or NULL
  const float* target;   // (B, J, 3)
  const float* jw;       // (B, J) or NULL
  float scale;
  float* gjoints;        // out (B, J, 3): the joint cotangent k_bwd_joint reads
  float* loss;           // (B): written by k_obj_vertex earlier on the stream; the joint loss is added
};

constexpr int kObjJointChunk = 16;  // joints per LDS stage of k_obj_joint

// grid ceil(B / 64), block 64: one lane per instance (the grid of k_bwd_joint).  The 64 instances of a block own one
// contiguous slab of every (B, J, 3) array.  It moves in stages of kObjJointChunk joints: consecutive lanes read and
// write consecutive floats of an instance's run (192 B) into LDS rows of odd stride, then lane r walks row r without
// bank conflicts.  p = joint + trans is formed on the way in (the forward's own single addition), the cotangent
// replaces p in place and leaves by the same pattern.  The loss terms of an instance are added in joint order in one
// register; no cross-lane sum, no atomics.
__global__ __launch_bounds__(64) void k_obj_joint(ObjJointArgs a, int B, int J) {
  constexpr int JC = kObjJointChunk, W = 3 * JC + 1, WU = JC + 1;
  __shared__ float sp[64 * W];   // joints, then their cotangents
  __shared__ float sq[64 * W];   // target joints
  __shared__ float su[64 * WU];  // scale * weight
  const int lane = threadIdx.x, b0 = blockIdx.x * 64, nrow = min(64, B - b0);
  float lsum = 0.f;
  for (int j0 = 0; j0 < J; j0 += JC) {
    const int nj = min(JC, J - j0), n3 = nj * 3;
    for (int e = lane; e < nrow * n3; e += 64) {
      const int r = e / n3, k = e - r * n3;
      const size_t o = ((size_t)(b0 + r) * J + j0) * 3 + k;
      sp[r * W + k] = a.rjoints[o] + (a.trans ? a.trans[(size_t)(b0 + r) * 3 + k % 3] : 0.f);
      sq[r * W + k] = a.target[o];
    }
    for (int e = lane; e < nrow * nj; e += 64) {
      const int r = e / nj, k = e - r * nj;
      su[r * WU + k] = a.jw ? a.scale * a.jw[(size_t)(b0 + r) * J + j0 + k] : a.scale;
    }
    __syncthreads();
    if (lane < nrow)
      for (int k = 0; k < nj; ++k) {
        float* p = sp + lane * W + k * 3;
        float g[3];
        lsum += sf::mesh_objective_vertex(p, sq + lane * W + k * 3, su[lane * WU + k], g);
        p[0] = g[0], p[1] = g[1], p[2] = g[2];
      }
    __syncthreads();
    for (int e = lane; e < nrow * n3; e += 64) {
      const int r = e / n3, k = e - r * n3;
      a.gjoints[((size_t)(b0 + r) * J + j0) * 3 + k] = sp[r * W + k];
    }
    __syncthreads();
  }
  if (lane < nrow) a.loss[b0 + lane] += lsum;
}

struct JointBwdArgs {
  const float *pose, *glob, *rel, *betas, *kid;
  int nb;
  const float *gjoints, *gorient;
  bool vertex;  // the vertex pass ran: bw.dA / bw.dtv / bw.dfeat hold its sums
  float *g_pose, *g_glob, *g_rel, *g_betas, *g_trans, *g_kid;
};

// grid ceil(B / 64), block 64: one lane per instance
__global__ __launch_bounds__(64) void k_bwd_joint(DevModel m, BwdWorkspace bw, JointBwdArgs a, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int J = m.J, NC = m.P + m.S;
  float gt[3];
  const float* df = a.vertex ? bw.dfeat + (size_t)b * NC : nullptr;
  sf::forward_joint_backward(
      m.jt, a.pose ? a.pose + (size_t)b * J * 3 : nullptr, a.glob ? a.glob + (size_t)b * J * 9 : nullptr,
      a.rel ? a.rel + (size_t)b * J * 9 : nullptr, a.betas ? a.betas + (size_t)b * a.nb : nullptr, a.betas ? a.nb : 0,
      a.kid ? a.kid + b : nullptr, a.vertex ? bw.dA + (size_t)b * J * 12 : nullptr,
      a.gjoints ? a.gjoints + (size_t)b * J * 3 : nullptr, a.gorient ? a.gorient + (size_t)b * J * 9 : nullptr, df,
      df ? df + m.P : nullptr, bw.jscr + (size_t)b * sf::joint_bwd_scratch_floats(J),
      a.g_pose ? a.g_pose + (size_t)b * J * 3 : nullptr, a.g_glob ? a.g_glob + (size_t)b * J * 9 : nullptr,
      a.g_rel ? a.g_rel + (size_t)b * J * 9 : nullptr, a.g_betas ? a.g_betas + (size_t)b * a.nb : nullptr,
      a.g_kid ? a.g_kid + b : nullptr, gt);
  if (a.g_trans)
    for (int c = 0; c < 3; ++c) a.g_trans[b * 3 + c] = gt[c] + (a.vertex ? bw.dtv[b * 3 + c] : 0.f);
}
