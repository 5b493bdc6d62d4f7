// Batch-major (lane = instance) vertex kernels of libsmplfit_hip.so.  Included by smplfit_hip.hip INSIDE
// its anonymous namespace, after kernels_wave.inc — not a stand-alone header.
// ================================================================================================
// Batch-major vertex kernels: LANE = INSTANCE.  A workgroup owns 64 consecutive instances and one
// vertex group (HostTables::groups: a run of <= 384 of one part's sorted slots with <= 12 skinning joints);
// its 4 waves split the group's vertices.  Everything that depends on the vertex only (shapedirs,
// skinning weights, joint slots) is wave-uniform and arrives through scalar loads; everything that
// depends on the instance (rotations, translations, betas, accumulators) lives in the lane's
// registers or in a lane-private LDS record; the streams (v_posed, targets) are stored instance-
// innermost so that a wave reads 256 contiguous bytes per vertex coordinate.  No cross-lane
// reductions, no per-vertex constants in VGPRs / LDS.
// ================================================================================================
constexpr int kGQ = sf::kGroupJoints;

// Batch-major stream layout: [instance block of 64][n][64 instances], n = c * Vp + slot.  A workgroup
// (one instance block, one vertex group) then streams three contiguous runs per buffer.
// targets: sorted SoA per instance [B][N] -> batch-major (N = 3 Vp; 64x64 LDS tiles)
// (also the per-instance joint rows jd (B, J*jd_stride) -> jdT for the pair-Gram kernel: Ns = the source
// row length, N = the destination row count = Ns rounded up to 64)
__global__ __launch_bounds__(256) void k_transpose_targets(const float* __restrict__ src,
                                                           float* __restrict__ dst, int B, int N,
                                                           int Mp, int Ns) {
  __shared__ float tile[64][65];
  const int n0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  // all 16 requests of a thread first, then the LDS stores (a guarded load-store loop runs its
  // iterations one memory latency after the other: 49 us for the 19 MB of joint rows)
  float v[16];
  const bool col_ok = n0 + tx < Ns;
  const float* sp = src + (size_t)(b0 + ty) * Ns + n0 + tx;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = (col_ok && b0 + ty + 4 * i < B) ? sp[(size_t)4 * i * Ns] : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[ty + 4 * i][tx] = v[i];
  __syncthreads();
  float* dp = dst + ((size_t)blockIdx.y * N + n0 + ty) * 64 + tx;
#pragma unroll
  for (int i = 0; i < 16; ++i) dp[(size_t)4 * i * 64] = tile[tx][ty + 4 * i];
}

// ------------------------------------------------------------------------------------------------
// One-pass target layout of the batch-major path (replaces K0 + the transpose there): the (B, V, 3) target rows
// are read ONCE and written ONCE, straight into the instance-innermost, part-sorted stream layout.
//   k_layout_targets   grid (ceil(V/kSlabV), Mp/64), block 256: a workgroup takes 64 instances x kSlabV consecutive
//                      ORIGINAL vertices (12 kSlabV contiguous bytes per instance), turns the tile in LDS and writes one
//                      256-byte row per (vertex, coordinate) at the vertex's sorted slot; it also leaves the
//                      tile's coordinate sums per instance in `part` (slab, 3, Mp).  The values are written
//                      UNCENTRED: the mean is not known before every tile of an instance has been read.
//   k_mean_finish      grid Mp/64, block 1024 (lane = instance, the 16 waves share the slabs / joints): mean over vertices (+ joints) from the slab sums in
//                      slab order, centred target joints, and the padding slots of the stream set to the mean —
//                      the consumers form t - mean on the fly (the same float the centred copy used to hold), so a
//                      padding slot still contributes exactly 0.
//   k_template_partsum_bm  the part sums of the centred targets against the template (first rotation estimate).
// reference: fit() centring bodyfitter.py:355-361; _part_sums :235-280 against default_mesh_tf.
// ------------------------------------------------------------------------------------------------
#ifndef SMPLFIT_SLAB
#define SMPLFIT_SLAB 32
#endif
constexpr int kSlabV = SMPLFIT_SLAB;      // original vertices per workgroup
constexpr int kSlabF = 3 * kSlabV;        // floats of one instance in a tile
constexpr int kSlabRow = kSlabF + 1;      // odd LDS row stride: the column reads of the second half are conflict-free

__global__ __launch_bounds__(256) void k_layout_targets(DevModel m, const float* __restrict__ tv, float* __restrict__ tT,
                                                        float* __restrict__ part, int B, int Mp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [64][kSlabRow]
  const int slab = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int V = m.V, Vp = m.Vp;
  const int v0 = slab * kSlabV, nf = 3 * min(kSlabV, V - v0);  // floats of one instance in this tile
  const float* src = tv + ((size_t)blk * 64 * V + v0) * 3;
  // ---- the tile: element e = instance * kSlabF + f, thread t takes e = t + 256 i (consecutive lanes read
  // consecutive floats of an instance's run).  All requests of a batch are issued before the first LDS store.
  constexpr int NL = 64 * kSlabF / 256, UB = NL % 12 == 0 ? 12 : 8;
  static_assert(NL % UB == 0, "tile loads per thread");
#pragma unroll
  for (int i0 = 0; i0 < NL; i0 += UB) {
    float x[UB];
#pragma unroll
    for (int i = 0; i < UB; ++i) {
      const int e = tid + 256 * (i0 + i), inst = e / kSlabF, f = e - inst * kSlabF;
      x[i] = (f < nf && blk * 64 + inst < B) ? ld_stream<4>(src + (size_t)inst * V * 3 + f) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < UB; ++i) {
      const int e = tid + 256 * (i0 + i), inst = e / kSlabF, f = e - inst * kSlabF;
      smem[inst * kSlabRow + f] = x[i];
    }
  }
  __syncthreads();
  // ---- columns j = 3 vl + c of the tile, j = wave + 4 k: one 256-byte row each, at the vertex's sorted slot
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  float* dst = tT + (size_t)blk * 3 * Vp * 64 + lane;
#pragma unroll 4
  for (int k = 0; k < kSlabF / 4; ++k) {
    const int j = wave + 4 * k;
    if (j >= nf) break;
    const int vl = j / 3, c = j - vl * 3;
    const int slot = m.inv_slot[v0 + vl];  // wave-uniform
    const float val = smem[lane * kSlabRow + j];
    st_stream<8>(dst + ((size_t)c * Vp + slot) * 64, val);
    if (c == 0) s0 += val;
    else if (c == 1) s1 += val;
    else s2 += val;
  }
  // ---- coordinate sums of the tile per instance: waves combined in a fixed order
  __syncthreads();
  smem[(wave * 3 + 0) * 64 + lane] = s0;
  smem[(wave * 3 + 1) * 64 + lane] = s1;
  smem[(wave * 3 + 2) * 64 + lane] = s2;
  __syncthreads();
  if (tid < 192) {
    const int c = tid >> 6;
    const float sum = (smem[c * 64 + lane] + smem[(3 + c) * 64 + lane]) + (smem[(6 + c) * 64 + lane] + smem[(9 + c) * 64 + lane]);
    part[((size_t)slab * 3 + c) * Mp + blk * 64 + lane] = sum;
  }
}

// The inverse of k_layout_targets for BodyModel.forward on the batch-major kernels: the posed vertices the forward-only
// LBS pass left in the instance-innermost stream (sorted slots) -> (B, V, 3) rows in the caller's vertex order.  The same
// tile: 64 instances x kSlabV original vertices, rows read at the vertices' sorted slots (256 bytes each), turned in LDS,
// written as 12 kSlabV contiguous bytes per instance.  grid (ceil(V/kSlabV), Mp/64), block 256.
// BLEND (smplfit_replace_hands_f32; <false> is the plain kernel: in / mix unused): the store loop writes
// out = in + (new - in) * mix[v] instead, the input read at the address the result goes to, so the new mesh never reaches
// memory as (B, V, 3).  Product and sum are rounded separately, as the reference's two elementwise operations are; where
// mix[v] == 0 the input is copied (the reference's arithmetic gives in + 0), and a slab whose mix is 0 throughout — for a
// body most of them — does not read the stream at all (workgroup-uniform, in front of the barrier).  `in` may be `out`:
// an element is read by the thread that writes it.
template <bool BLEND>
__global__ __launch_bounds__(256) void k_unlayout_vertices(DevModel m, const float* __restrict__ vT, float* out, int B,
                                                           const float* in = nullptr, const float* __restrict__ mix = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [64][kSlabRow]
  const int slab = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int V = m.V, Vp = m.Vp;
  const int v0 = slab * kSlabV, nf = 3 * min(kSlabV, V - v0);
  float* dst = out + ((size_t)blk * 64 * V + v0) * 3;
  constexpr int NL = 64 * kSlabF / 256;
  if constexpr (BLEND) {
    bool any = false;
    for (int vl = 0; 3 * vl < nf; ++vl) any |= mix[v0 + vl] != 0.f;
    if (!any) {  // the input as it is
      const float* srcv = in + ((size_t)blk * 64 * V + v0) * 3;
      if (in != out) {
#pragma unroll 8
        for (int i = 0; i < NL; ++i) {
          const int e = tid + 256 * i, inst = e / kSlabF, f = e - inst * kSlabF;
          if (f < nf && blk * 64 + inst < B) dst[(size_t)inst * V * 3 + f] = srcv[(size_t)inst * V * 3 + f];
        }
      }
      return;
    }
  }
  const float* src = vT + (size_t)blk * 3 * Vp * 64 + lane;
  // all requests of a batch first, then the LDS stores (a load-store loop runs one memory latency after the other)
  constexpr int NR = kSlabF / 4, UB = NR % 12 == 0 ? 12 : 8;
  static_assert(NR % UB == 0, "rows per wave");
#pragma unroll
  for (int k0 = 0; k0 < NR; k0 += UB) {
    float x[UB];
#pragma unroll
    for (int k = 0; k < UB; ++k) {
      const int j = wave + 4 * (k0 + k), jj = j < nf ? j : 0, vl = jj / 3, c = jj - vl * 3;
      x[k] = ld_stream<1>(src + ((size_t)c * Vp + m.inv_slot[v0 + vl]) * 64);
    }
#pragma unroll
    for (int k = 0; k < UB; ++k) {
      const int j = wave + 4 * (k0 + k);
      if (j < nf) smem[lane * kSlabRow + j] = x[k];
    }
  }
  __syncthreads();
#pragma unroll 8
  for (int i = 0; i < NL; ++i) {
    const int e = tid + 256 * i, inst = e / kSlabF, f = e - inst * kSlabF;
    if (f < nf && blk * 64 + inst < B) {
      if constexpr (BLEND) {
        const float a = in[((size_t)blk * 64 * V + v0) * 3 + (size_t)inst * V * 3 + f], w = mix[v0 + f / 3];
        dst[(size_t)inst * V * 3 + f] = w == 0.f ? a : __fadd_rn(a, __fmul_rn(__fsub_rn(smem[inst * kSlabRow + f], a), w));
      } else {
        st_stream<8>(dst + (size_t)inst * V * 3 + f, smem[inst * kSlabRow + f]);
      }
    }
  }
}

// The measuring form of k_unlayout_vertices (the mesh-error step, launch_mesh_error): the same tile of the posed mesh,
// turned in LDS the same way; the caller's target tile is then read in the pattern the BLEND form reads `in` (element
// e = tid + 256 i: consecutive lanes, consecutive floats of an instance's run) and every element of the tile is replaced
// by mesh - target by the one thread that owns it — which, WRITE_MESH, first stores the mesh value to `out`, the plain
// form's store.  Behind a second barrier a thread takes a (instance, vertex) pair, reads its three differences — three
// scalar LDS reads: kSlabRow is odd, so a vertex's words are 4-byte aligned only — and writes the distance to
// err (B, V): 32 consecutive lanes write the 128 contiguous bytes of an instance's kSlabV vertices.  Without WRITE_MESH
// no (B, V, 3) is written.  Rows >= B and vertices >= V are neither read from the target nor written; every output
// element has one writer.  grid (ceil(V/kSlabV), Mp/64), block 256, as the plain form.
__device__ __forceinline__ float point_distance(float dx, float dy, float dz) {
  return __fsqrt_rn(__fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx))));
}
template <bool WRITE_MESH>
__global__ __launch_bounds__(256) void k_unlayout_error(DevModel m, const float* __restrict__ vT, float* __restrict__ out,
                                                        const float* __restrict__ target, float* __restrict__ err, int B) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [64][kSlabRow]
  const int slab = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int V = m.V, Vp = m.Vp;
  const int v0 = slab * kSlabV, nv = min(kSlabV, V - v0), nf = 3 * nv;
  const size_t tile = ((size_t)blk * 64 * V + v0) * 3;  // the tile's first float in a (B, V, 3) tensor
  const float* src = vT + (size_t)blk * 3 * Vp * 64 + lane;
  constexpr int NR = kSlabF / 4, UB = NR % 12 == 0 ? 12 : 8;
  static_assert(NR % UB == 0, "rows per wave");
#pragma unroll
  for (int k0 = 0; k0 < NR; k0 += UB) {
    float x[UB];
#pragma unroll
    for (int k = 0; k < UB; ++k) {
      const int j = wave + 4 * (k0 + k), jj = j < nf ? j : 0, vl = jj / 3, c = jj - vl * 3;
      x[k] = ld_stream<1>(src + ((size_t)c * Vp + m.inv_slot[v0 + vl]) * 64);
    }
#pragma unroll
    for (int k = 0; k < UB; ++k) {
      const int j = wave + 4 * (k0 + k);
      if (j < nf) smem[lane * kSlabRow + j] = x[k];
    }
  }
  __syncthreads();
  // ---- mesh out, mesh - target in place: all target requests of a batch first
  constexpr int NL = 64 * kSlabF / 256, UL = 8;
  static_assert(NL % UL == 0, "tile elements per thread");
#pragma unroll
  for (int i0 = 0; i0 < NL; i0 += UL) {
    float t[UL];
#pragma unroll
    for (int i = 0; i < UL; ++i) {
      const int e = tid + 256 * (i0 + i), inst = e / kSlabF, f = e - inst * kSlabF;
      t[i] = (f < nf && blk * 64 + inst < B) ? ld_stream<4>(target + tile + (size_t)inst * V * 3 + f) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < UL; ++i) {
      const int e = tid + 256 * (i0 + i), inst = e / kSlabF, f = e - inst * kSlabF;
      if (f < nf && blk * 64 + inst < B) {
        const float v = smem[inst * kSlabRow + f];
        if constexpr (WRITE_MESH) st_stream<8>(out + tile + (size_t)inst * V * 3 + f, v);
        smem[inst * kSlabRow + f] = __fsub_rn(v, t[i]);
      }
    }
  }
  __syncthreads();
  // ---- one distance per (instance, vertex)
  constexpr int NE = 64 * kSlabV / 256;
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = tid + 256 * i, inst = e / kSlabV, vl = e - inst * kSlabV;
    if (vl < nv && blk * 64 + inst < B) {
      const float* d = smem + inst * kSlabRow + 3 * vl;
      err[((size_t)blk * 64 + inst) * V + v0 + vl] = point_distance(d[0], d[1], d[2]);
    }
  }
}

// The distances of the mesh-error step where no tile is turned: err[i] = |a[i] - b[i]| over n points of two (n, 3)
// arrays, one thread per point — the joints of every route, the vertices of the wave-per-instance and general routes
// (behind their forward LBS pass).  The arithmetic of k_unlayout_error.
__global__ __launch_bounds__(256) void k_point_error(const float* __restrict__ a, const float* __restrict__ b,
                                                     float* __restrict__ err, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *pa = a + i * 3, *pb = b + i * 3;
  err[i] = point_distance(__fsub_rn(pa[0], pb[0]), __fsub_rn(pa[1], pb[1]), __fsub_rn(pa[2], pb[2]));
}

constexpr int kMeanWaves = 16;  // waves of a k_mean_finish workgroup (they share the slabs / joints / padding slots)
__global__ __launch_bounds__(64 * kMeanWaves) void k_mean_finish(DevModel m, const float* __restrict__ tj,
                                                                 const float* __restrict__ part, Workspace ws, int B, int Mp,
                                                                 int nslab) {
  constexpr int NW = kMeanWaves;
  __shared__ float red[NW * 3 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bcol = blockIdx.x * 64 + lane, J = m.J, V = m.V, Vp = m.Vp;
  const bool live = bcol < B;
  const int b = live ? bcol : B - 1;
  // slab sums: wave w takes slabs w, w + NW, ... (eight requests in flight), the NW partial sums are then added
  // in wave order — a fixed summation order
  float s[3] = {0.f, 0.f, 0.f};
  constexpr int U = 8;
  for (int sl0 = wave; sl0 < nslab; sl0 += NW * U) {
    float x[U][3];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int sl = sl0 + NW * u;
#pragma unroll
      for (int c = 0; c < 3; ++c) x[u][c] = sl < nslab ? part[((size_t)sl * 3 + c) * Mp + bcol] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += x[u][c];
  }
  if (tj)
    for (int j = wave; j < J; j += NW)
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += tj[((size_t)b * J + j) * 3 + c];
#pragma unroll
  for (int c = 0; c < 3; ++c) red[(wave * 3 + c) * 64 + lane] = s[c];
  __syncthreads();
  const float n = (float)(V + (tj ? J : 0));
  float mu[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float sum = red[c * 64 + lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) sum += red[(w * 3 + c) * 64 + lane];
    mu[c] = live ? sum / n : 0.f;
  }
  if (live) {
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) ws.mean[(size_t)b * 3 + c] = mu[c];
    }
    if (tj)
      for (int j = wave; j < J; j += NW)
#pragma unroll
        for (int c = 0; c < 3; ++c) ws.tjc[((size_t)b * J + j) * 3 + c] = tj[((size_t)b * J + j) * 3 + c] - mu[c];
  }
  float* dst = ws.tT + (size_t)blockIdx.x * 3 * Vp * 64 + lane;
  for (int slot = V + wave; slot < Vp; slot += NW)
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[((size_t)c * Vp + slot) * 64] = mu[c];
}

typedef float f2 __attribute__((ext_vector_type(2)));

// Model tables read as wave-uniform records go through the constant address space (scalar loads whatever else
// the loop does).
typedef const __attribute__((address_space(4))) float* const_f32_ptr;
__device__ __forceinline__ const_f32_ptr as_constant(const float* p) {
  return (const_f32_ptr)(unsigned long long)p;
}
typedef const __attribute__((address_space(4))) int32_t* const_i32_ptr;
__device__ __forceinline__ const_i32_ptr as_constant(const int32_t* p) {
  return (const_i32_ptr)(unsigned long long)p;
}
// posed rest position and target of one vertex, loaded straight into the halves of three aligned register pairs
// (x, y of the position; x, y of the target; the two z): packed instructions that broadcast ONE half still read the
// pair, and a pair made of values from two different buffers makes the wait for one buffer a wait for both
struct StreamBuf { f2 x01, t01, xt2; };
__device__ __forceinline__ f2 mk2(float a, float b) { f2 r; r.x = a; r.y = b; return r; }

__host__ __device__ constexpr int brec_w(int S) { return (3 * S + 3) / 4 * 4; }
__host__ __device__ constexpr int brec_stride(int S, int NJ = 4) { return brec_w(S) + NJ; }

// waves per workgroup of the batch-major vertex kernels (they split a vertex group evenly; sf::kBmWaves is what the
// host tables cut the groups' pieces for)
constexpr int kBW = sf::kBmWaves;
constexpr int kPieceRec = sf::kPieceRec;

// The four joints of a PIECE (sf::kPieceRec: a run of slots whose skinning joints number at most four) as the vertex
// loops keep them IN REGISTERS: six register pairs per joint, laid out for the packed-fp32 blend and rotation
//   (R0,R3) (R1,R4) (R2,R5) (R6,R7) (R8,tz) (tx,ty)        t = the joint's translation of this pass.
// Per vertex the blend is then 24 packed FMAs of scalar weights against these registers — no LDS read, no address
// arithmetic, and the blended record is available as soon as the vertex's weights are.
// NJ = 8 (models with 5-8 skinning weights per vertex, round 5): eight joints of a piece in registers — 96 instead of 48
// registers, so those instantiations are built for two waves per SIMD; the piece record is a pair of records (sf_tables.h)
template <int NJ = 4>
struct PieceJointsT { f2 p[NJ][6]; };
using PieceJoints = PieceJointsT<4>;
// joint k / its local segment slot of the piece record at pc (kPieceRec ints per four joints)
template <class P>
__device__ __forceinline__ int piece_joint(P pc, int k) { return pc[(k >> 2) * kPieceRec + 1 + (k & 3)]; }
template <class P>
__device__ __forceinline__ int piece_slot(P pc, int k) { return pc[(k >> 2) * kPieceRec + 5 + (k & 3)]; }
// A vertex's record (HostTables::brec: 3 S shapedirs values + its four weights in the piece's joint order).  It is
// wave-uniform and fetched with scalar loads ONE STEP AHEAD into a second set of scalar registers: a scalar load that
// misses its cache takes a good part of a step to come back from L2.  Scalar loads return out of order, so any wait
// on one is a wait for all: a step first waits for its own record (requested a step ago, the only scalar request
// outstanding), THEN requests the next one; two scheduling barriers keep that order, and the loops keep LDS reads
// (the same counter) out of the step.
template <int S, int NJ = 4>
struct VertexRec { float sd[3 * S]; float w[NJ]; };
template <int S, int NJ = 4>
__device__ __forceinline__ void load_rec(const float* brec, int v, VertexRec<S, NJ>& r) {
  const const_f32_ptr rec = as_constant(brec + (size_t)v * brec_stride(S, NJ));
#pragma unroll
  for (int k = 0; k < 3 * S; ++k) r.sd[k] = rec[k];
#pragma unroll
  for (int k = 0; k < NJ; ++k) r.w[k] = rec[brec_w(S) + k];
}
template <int S, int NJ = 4>
__device__ __forceinline__ void rec_arrived_request_next(const float* brec, const VertexRec<S, NJ>& cur, int vnext, VertexRec<S, NJ>& next) {
  // two resident records need 2 (3 S + NJ) scalar registers: with the kid unknown (S = 11) or eight weights that no
  // longer fits the ~100 a wave has, and the compiler is left to place the loads itself
  if constexpr (2 * (3 * S + NJ) <= 68) {
    asm volatile("" ::"s"(cur.w[0]));
    __builtin_amdgcn_sched_barrier(0);
    load_rec<S, NJ>(brec, vnext, next);
    __builtin_amdgcn_sched_barrier(0);
  } else {
    load_rec<S, NJ>(brec, vnext, next);
  }
}

// K5 (batch-major): vertices at the solved shape + part sums against the targets.
// grid (Mp/64, ncells / mult / kBW), block 64 * kBW: wave = one share (mult cells) of one instance block.  Output: a row of ws.psumP
// ([row][16][Mp]) after the last piece of every run of one part (piece record [10]), written by the wave itself.
// Per vertex: ~70 VALU (packed fp32); the vertex record (shapedirs, 4 weights) is read with scalar loads.
//
// WRITE_V (joints-omitted fits): the table covers every slot and the vertex at the solution is written back IN
// PLACE over its rest position in ws.vpT (a (vertex, lane) element is read and later written by the same lane of
// the same wave only; the GEMM of the next iteration rewrites the buffer): the reference joints of the next
// rotation pass are regressed from it (k_regress_joints_bm).
// FWD (with WRITE_V; the input side of a fused conversion, smplfit_convert_f32): the forward only — no targets are
// read, no part sums are formed; the posed vertices stay in ws.vpT for k_transfer_bm.
#ifndef SMPLFIT_LBS_WAVES
#define SMPLFIT_LBS_WAVES 4
#endif
// W (vertex weights given): the weight stream ws.wT is read beside the targets and the sums are the weighted ones of
// sf::partsum_vertex (raw += t (w a)^T, st += w t, sa += w a, count += w).
template <int S, int KW, bool WRITE_V = false, bool FWD = false, bool W = false>
__global__ __launch_bounds__(64 * kBW) __attribute__((amdgpu_waves_per_eu((KW == 8 || S > 12) ? 2 : SMPLFIT_LBS_WAVES, (KW == 8 || S > 12) ? 2 : SMPLFIT_LBS_WAVES))) void k_lbs_partsum_bm(DevModel m, ShareView sv, Workspace ws, int B, int Mp,
                                                                                                                                      int write_all = 1) {
  static_assert(!FWD || WRITE_V, "the forward-only variant writes the vertices");
  static_assert(!(FWD && W), "the forward-only variant reads no weights");
  constexpr int NJ = KW, RS = kPieceRec * (NJ / 4);  // joints of a piece (4 or 8), ints per piece record
  constexpr int STRIDE = sf::jd_stride(S), BW = brec_w(S), BS = brec_stride(S, NJ);
  static_assert(KW == 4 || KW == 8, "batch-major kernels: 4 or 8 skinning pairs per vertex");
  const int tid = threadIdx.x, lane = tid & 63;
  // wave index as a SCALAR: everything derived from it (share, record addresses) stays
  // wave-uniform for the compiler, so the per-vertex records are fetched with s_load
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int share = blockIdx.y * kBW + wave, blk = blockIdx.x, J = m.J, Vp = m.Vp;
  const int bcol = blk * 64 + lane;           // column of the instance-innermost buffers
  const int b = bcol < B ? bcol : B - 1;             // row of the per-instance buffers
  const int Np = (J * STRIDE + 63) / 64 * 64;
  const float* jdb = ws.jdT + (size_t)blk * Np * 64 + lane;
  // a piece's joints, lane = instance: rotations from the instance-innermost copy of the joint rows (ws.jdT) and the
  // skinning translation at the solution from the instance-innermost copy of jb (ws.jbT) — 12 coalesced 256-byte
  // reads per joint — plus the instance's translation (re-read per piece: three registers less in the loop)
  PieceJointsT<NJ> jr;
  const float* jbb = ws.jbT + (size_t)blk * J * 4 * 64 + lane;
  auto load_joints = [&](const_i32_ptr rec) {
    const float tr0 = ws.trans[b * 3], tr1 = ws.trans[b * 3 + 1], tr2 = ws.trans[b * 3 + 2];
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      const int j = piece_joint(rec, k);
      const float* row = jdb + (size_t)j * STRIDE * 64;
      const float* tb = jbb + (size_t)j * 4 * 64;
      float r[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) r[i] = row[i * 64];
      const float tbx = tb[0], tby = tb[64], tbz = tb[128];
      jr.p[k][0] = mk2(r[0], r[3]);
      jr.p[k][1] = mk2(r[1], r[4]);
      jr.p[k][2] = mk2(r[2], r[5]);
      jr.p[k][3] = mk2(r[6], r[7]);
      jr.p[k][4] = mk2(r[8], tbz + tr2);
      jr.p[k][5] = mk2(tbx + tr0, tby + tr1);
    }
  };
  // the lane's shape and target mean live in registers: an LDS read inside the loop would share its counter with the
  // scalar loads of the records and make every wait for it a wait for them
  float beta[S];
#pragma unroll
  for (int s2 = 0; s2 < S; ++s2) beta[s2] = ws.beta[(size_t)b * S + s2];
  // accumulators: P0..P2 = raw rows (cols 0,1), P3 = (raw02, raw12), s22; P4 = (st0, st1), st2;
  // P5 = (sa0, sa1), sa2
  f2 P0 = mk2(0, 0), P1 = P0, P2 = P0, P3 = P0, P4 = P0, P5 = P0;
  float s22 = 0.f, st2 = 0.f, sa2 = 0.f;
  // wave-uniform stream bases + the lane as a 32-bit offset: scalar-base addressing, no 64-bit
  // vector address arithmetic per load
  const float* vp = ws.vpT + (size_t)blk * 3 * Vp * 64;
  const float* tp = ws.tT + (size_t)blk * 3 * Vp * 64;
  const uint32_t ul = (uint32_t)lane;
  const size_t cstr = (size_t)Vp * 64;  // coordinate stride inside the instance block
  struct RawX { f2 x01; float x2; };  // (x, y) loaded straight into the halves of one register pair
  struct RawT { f2 t01; float t2; float w; };
  const float* wp = W ? ws.wT + (size_t)blk * Vp * 64 : nullptr;
  auto fetch_x = [&](int v) {
    const float* q = vp + (size_t)v * 64;
    RawX r;
    r.x01.x = ld_stream<1>(q + ul); r.x01.y = ld_stream<1>(q + cstr + ul); r.x2 = ld_stream<1>(q + 2 * cstr + ul);
    return r;
  };
  auto fetch_t = [&](int v) {
    const float* q = tp + (size_t)v * 64;
    RawT r;
    if constexpr (FWD) {
      r.t01 = mk2(0.f, 0.f); r.t2 = 0.f;
    } else {
      r.t01.x = ld_stream<1>(q + ul); r.t01.y = ld_stream<1>(q + cstr + ul); r.t2 = ld_stream<1>(q + 2 * cstr + ul);
    }
    if constexpr (W) r.w = ld_stream<1>(wp + (size_t)v * 64 + ul);
    else r.w = 1.f;
    return r;
  };
  // the stream holds the targets as given: centred where they are used (t - mean is the float the centred copy
  // used to hold)
  const f2 mu01 = FWD ? mk2(0.f, 0.f) : mk2(ws.mean[(size_t)b * 3], ws.mean[(size_t)b * 3 + 1]);
  const float mu2 = FWD ? 0.f : ws.mean[(size_t)b * 3 + 2];
  auto centre01 = [&](const f2 t) { return t - mu01; };
  auto centre2 = [&](const float t) { return t - mu2; };
  // Loaded values are only ever read as plain 32-bit operands: pairing or carrying a LOADED value takes
  // a register copy, which the compiler sinks to the loop's back edge together with a wait for every
  // outstanding load.
  // prep: rest position + shape blend of vertex v (vs) and its four weights in the piece's joint order
  auto prep = [&](const VertexRec<S, NJ>& vr, const RawX& r, f2& vs01, float& vs2, float (&wq)[NJ]) {
    const float (&rec)[3 * S] = vr.sd;
    // beta pairs against the per-coordinate shapedirs rows
    f2 bp = mk2(beta[0], beta[1]);
    f2 vx = mk2(rec[0], rec[1]) * bp, vy = mk2(rec[S], rec[S + 1]) * bp, vz = mk2(rec[2 * S], rec[2 * S + 1]) * bp;
#pragma unroll
    for (int s2 = 2; s2 + 1 < S; s2 += 2) {
      bp = mk2(beta[s2], beta[s2 + 1]);
      vx += mk2(rec[s2], rec[s2 + 1]) * bp;
      vy += mk2(rec[S + s2], rec[S + s2 + 1]) * bp;
      vz += mk2(rec[2 * S + s2], rec[2 * S + s2 + 1]) * bp;
    }
    if (S & 1) {
      vx.x += rec[S - 1] * beta[S - 1];
      vy.x += rec[2 * S - 1] * beta[S - 1];
      vz.x += rec[3 * S - 1] * beta[S - 1];
    }
    vs01 = mk2(vx.x + vx.y, vy.x + vy.y) + r.x01;
    vs2 = (vz.x + vz.y) + r.x2;
#pragma unroll
    for (int k = 0; k < NJ; ++k) wq[k] = vr.w[k];
  };
  // blend of the piece's four joints with the vertex's weights: 6 register pairs
  // (joint-outer order: the six accumulations of one joint are independent instructions back to back; with the pair
  // index outermost hipcc emits each pair's four dependent FMAs as a serial chain with wait states in between)
  auto blend = [&](const float (&wq)[NJ], f2 (&Q)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) Q[i] = mk2(0, 0);
#pragma unroll
    for (int k = 0; k < NJ; ++k)
#pragma unroll
      for (int i = 0; i < 6; ++i) Q[i] += wq[k] * jr.p[k][i];
  };
  // This wave's pieces (wave-uniform records, scalar loads).  The step sequence of the wave is: the vertices of
  // every piece in turn, followed by ONE step on the first padding slot (slot V: zero streams, an all-zero record —
  // it contributes exactly 0 to every sum) when the piece has an odd number of vertices.  Every piece is then an
  // even number of steps: the two stream buffers keep their roles across pieces, the loop has no remainder step
  // (the compiler folds a remainder into the loop and drains every outstanding load at the back edge), and the
  // requests run ahead across piece boundaries.
  const int ps = sv.piece_start[share * sv.mult], np = sv.piece_start[(share + 1) * sv.mult] - ps;
  if (np <= 0) return;
  const int vpad = m.V;
  const_i32_ptr pc = as_constant(sv.pieces + (size_t)ps * RS);
  int vb = pc[9], len = pc[0], cnt = 0;
  float wcnt = 0.f;  // (W: the sum of the weights takes the place of the count)
  const int v0 = vb;
  f2 vs01;
  float vs2, wq[NJ];
  // the part sums of one posed vertex (_part_sums, bodyfitter.py:257-280); wv = 1 without vertex weights
  auto accumulate = [&](const f2 t01, const float t2, f2 a01, float a2, const float wv) {
    if constexpr (!FWD) {
      if constexpr (W) {
        a01 = a01 * wv;
        a2 = a2 * wv;
        P4 += t01 * wv;
        st2 += t2 * wv;
        wcnt += wv;
      } else {
        P4 += t01;
        st2 += t2;
      }
      P0 += t01.x * a01;
      P1 += t01.y * a01;
      P2 += t2 * a01;
      P3 += t01 * a2;
      s22 += t2 * a2;
      P5 += a01;
      sa2 += a2;
    }
  };
  // Two buffers per stream used alternately, two steps per iteration.  A step requests the targets of the next
  // vertex and the posed rest position of the one after it, blends / poses / accumulates its own vertex (whose
  // prepared values are carried in registers, whose targets are read straight from their buffer) and LAST prepares
  // the next vertex from its rest position — so every loaded value has between one and two steps to arrive, is
  // never copied and lives exactly as long as its buffer.
  RawT tA = fetch_t(v0), tB;
  RawX xA, xB;
  VertexRec<S, NJ> recA, recB;  // records of the NEXT vertex of a step (prepared at its end), requested a step ahead
  // WRITE_V without write_all (the joints-omitted fit): only the vertices the joint regressor reads are written back —
  // a flag in the spare float behind the record's shapedirs (sf_tables.cpp), requested with the record two steps ahead
  // into the flag slot of that record's buffer
  constexpr bool kFlagged = WRITE_V && !FWD && BW > 3 * S;
  auto slot_flag = [&](int v) { return as_constant(m.brec + (size_t)v * BS)[3 * S]; };
  float fA = 1.f, fB = 1.f;
  {
    const RawX xi = fetch_x(v0);
    const int v1st = len > 1 ? v0 + 1 : vpad;
    xA = fetch_x(v1st);
    load_rec<S, NJ>(m.brec, v0, recB);
    load_rec<S, NJ>(m.brec, v1st, recA);
    if constexpr (kFlagged) {
      fB = slot_flag(v0);
      fA = slot_flag(v1st);
    }
    prep(recB, xi, vs01, vs2, wq);
  }
  auto step = [&](int vcur, int vn1, int vn2, const RawT& cur, RawT& fill_t, const RawX& next, RawX& fill_x,
                  const VertexRec<S, NJ>& rn1, VertexRec<S, NJ>& rn2, float& flag2) {
    rec_arrived_request_next<S, NJ>(m.brec, rn1, vn2, rn2);  // vn1's record is here; vn2's is requested
    const float fcur = flag2;  // (this vertex's flag came with the record this buffer held two steps ago)
    if constexpr (kFlagged) flag2 = slot_flag(vn2);
    fill_t = fetch_t(vn1);
    fill_x = fetch_x(vn2);
    f2 Q[6];
    blend(wq, Q);
    // posed vertex (translation already folded into the joints' records)
    const f2 a01 = (Q[0] * vs01.x + Q[1] * vs01.y) + (Q[2] * vs2 + Q[5]);
    const float a2 = (Q[3].x * vs01.x + Q[3].y * vs01.y) + (Q[4].x * vs2 + Q[4].y);
    // (centred target z, posed z) as ONE aligned register pair, pinned by an empty asm: the sums broadcast either half
    // through packed instructions, which read the whole pair — left to the allocator, a half that is a load's
    // destination register turns the loop's last wait into vmcnt(0) (see StreamBuf)
    f2 tz_az = mk2(centre2(cur.t2), a2);
    asm volatile("" : "+v"(tz_az));
    accumulate(centre01(cur.t01), tz_az.x, a01, tz_az.y, cur.w);
    if constexpr (WRITE_V) {
      if (vcur != vpad && (!kFlagged || write_all || fcur != 0.f)) {  // wave-uniform: a real vertex (never the padding slot) that is read later
        float* q = const_cast<float*>(vp) + (size_t)vcur * 64;
        q[ul] = a01.x; (q + cstr)[ul] = a01.y; (q + 2 * cstr)[ul] = a2;
      }
    }
    prep(rn1, next, vs01, vs2, wq);
  };
  for (int p = 0; p < np; ++p) {
    const bool more = p + 1 < np;
    const int len_next = more ? pc[RS] : 0, vn = more ? pc[RS + 9] : vpad, l2 = len + (len & 1);
    load_joints(pc);
    // The joints are "used" HERE (empty asm statements), so their loads — which the compiler would otherwise sink
    // to their first use inside the vertex loop — are complete before it: the loop is left with nothing but its
    // own requests pending and its waits are exact partial waits (the other buffer stays in flight), not vmcnt(0).
#pragma unroll
    for (int k = 0; k < NJ; ++k)
#pragma unroll
      for (int i = 0; i < 6; ++i) asm volatile("" : "+v"(jr.p[k][i].x), "+v"(jr.p[k][i].y));
    // vertex of step i of this piece, continued into the first steps of the next piece
    auto at = [&](int i) {  // (scalar selects, no branches: the step pair stays one scheduling region)
      const int k = i - l2;
      int r = ((k >= 0) & (k < len_next)) ? vn + k : vpad;
      r = i < len ? vb + i : r;
      return r;
    };
    for (int i = 0; i < l2; i += 2) {
      step(vb + i, at(i + 1), at(i + 2), tA, tB, xA, xB, recA, recB, fB);
      step(at(i + 1), at(i + 2), at(i + 3), tB, tA, xB, xA, recB, recA, fA);
    }
    cnt += len;
    if constexpr (!FWD) {
      const int row = pc[10];
      if (row >= 0) {  // the last piece of a run of one part: the wave's sums of the run go to their row
        float* out = ws.psumP + (size_t)row * sf::kPsum * Mp + bcol;
        const float acc[sf::kPsum] = {P0.x, P0.y, P3.x, P1.x, P1.y, P3.y, P2.x, P2.y, s22,
                                      P4.x, P4.y, st2, P5.x, P5.y, sa2, W ? wcnt : (float)cnt};
#pragma unroll
        for (int k = 0; k < sf::kPsum; ++k) out[(size_t)k * Mp] = acc[k];
        P0 = mk2(0, 0); P1 = P0; P2 = P0; P3 = P0; P4 = P0; P5 = P0;
        s22 = 0.f; st2 = 0.f; sa2 = 0.f;
        cnt = 0;
        wcnt = 0.f;
      }
    }
    vb = vn;
    len = len_next;
    pc += RS;
  }
}

// Part sums of the centred targets against the TEMPLATE (the first rotation estimate of a fit): the k_lbs_partsum_bm
// sums with a_v = the rest template (wave-uniform, scalar loads), over the same share table and into the same rows
// (then k_psum_combine).  A share's contiguous pieces of one part are walked as one run.
template <bool W>
__global__ __launch_bounds__(64 * kBW) void k_template_partsum_bm(DevModel m, ShareView sv, Workspace ws, int B, int Mp) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int share = blockIdx.y * kBW + wave, blk = blockIdx.x, Vp = m.Vp;
  const int bcol = blk * 64 + lane, b = bcol < B ? bcol : B - 1;
  const float mu0 = ws.mean[(size_t)b * 3], mu1 = ws.mean[(size_t)b * 3 + 1], mu2 = ws.mean[(size_t)b * 3 + 2];
  const float* tp = ws.tT + (size_t)blk * 3 * Vp * 64 + lane;
  const float* wp = W ? ws.wT + (size_t)blk * Vp * 64 + lane : nullptr;  // (padding slots hold weight 0)
  const size_t cstr = (size_t)Vp * 64;
  const const_f32_ptr dm = as_constant(m.dm);
  const int vpad = m.V;  // padding slot: target = mean, template = 0 -> contributes exactly 0
  const int ps = sv.piece_start[share * sv.mult], np = sv.piece_start[(share + 1) * sv.mult] - ps;
  const int RS = sv.rec;  // ints per piece record (12, or 24 for pieces of up to eight joints)
  const_i32_ptr pc = as_constant(sv.pieces + (size_t)ps * RS);
  float acc[sf::kPsum];
#pragma unroll
  for (int k = 0; k < sf::kPsum; ++k) acc[k] = 0.f;
  constexpr int U = 4;
  int p = 0;
  while (p < np) {
    // a run: consecutive pieces up to the one that closes a row (or the next one starts elsewhere)
    const int v0 = pc[9];
    int v1 = v0 + pc[0], row = pc[10];
    ++p;
    pc += RS;
    while (row < 0 && p < np && pc[9] == v1) {
      v1 += pc[0];
      row = pc[10];
      ++p;
      pc += RS;
    }
    for (int v = v0; v < v1; v += U) {
      float t[U][3], a[U][3], wv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int vv = v + u < v1 ? v + u : vpad;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          t[u][c] = ld_stream<1>(tp + (size_t)c * cstr + (size_t)vv * 64);
          a[u][c] = dm[c * Vp + vv];
        }
        wv[u] = W ? ld_stream<1>(wp + (size_t)vv * 64) : 1.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float tc[3] = {t[u][0] - mu0, t[u][1] - mu1, t[u][2] - mu2};
        const float aw[3] = {W ? a[u][0] * wv[u] : a[u][0], W ? a[u][1] * wv[u] : a[u][1], W ? a[u][2] * wv[u] : a[u][2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[r * 3 + c] += tc[r] * aw[c];
          acc[9 + r] += W ? tc[r] * wv[u] : tc[r];
          acc[12 + r] += aw[r];
        }
        if constexpr (W) acc[15] += wv[u];
      }
    }
    if constexpr (!W) acc[15] += (float)(v1 - v0);
    if (row >= 0) {
      float* out = ws.psumP + (size_t)row * sf::kPsum * Mp + bcol;
#pragma unroll
      for (int k = 0; k < sf::kPsum; ++k) {
        out[(size_t)k * Mp] = acc[k];
        acc[k] = 0.f;
      }
    }
  }
}

// Sparse post-LBS joint regression on an instance-innermost stream (joints-omitted fits):
// out[b][j] = sum_k reg_val[k] (src[slot_k][b] - mean[b] if SUB_MEAN).  reference: bodyfitter.py:1342-1344.
// grid (Mp/64, J), block 64 (lane = instance); the entries of a joint in table order.
template <bool SUB_MEAN>
__global__ __launch_bounds__(64) void k_regress_joints_bm(DevModel m, const float* __restrict__ src, const float* __restrict__ mean,
                                                          float* __restrict__ out, int B) {
  const int lane = threadIdx.x, blk = blockIdx.x, j = blockIdx.y, Vp = m.Vp;
  const int bcol = blk * 64 + lane, b = bcol < B ? bcol : B - 1;
  const float* s = src + (size_t)blk * 3 * Vp * 64 + lane;
  const size_t cstr = (size_t)Vp * 64;
  float mu[3] = {0.f, 0.f, 0.f};
  if (SUB_MEAN)
    for (int c = 0; c < 3; ++c) mu[c] = mean[(size_t)b * 3 + c];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  const int k0 = m.reg_start[j], k1 = m.reg_start[j + 1];
  constexpr int U = 4;
  for (int k = k0; k < k1; k += U) {
    float x[U][3], r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = k + u < k1 ? k + u : k1 - 1;
      const int slot = m.reg_slot[kk];
      r[u] = k + u < k1 ? m.reg_val[kk] : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) x[u][c] = s[(size_t)c * cstr + (size_t)slot * 64];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      a0 += r[u] * (x[u][0] - mu[0]);
      a1 += r[u] * (x[u][1] - mu[1]);
      a2 += r[u] * (x[u][2] - mu[2]);
    }
  }
  if (bcol < B) {
    float* o = out + ((size_t)b * m.J + j) * 3;
    o[0] = a0; o[1] = a1; o[2] = a2;
  }
}

// K3 (batch-major, unit weights): residual pass of the pair-Gram form over ALL slots.
//   b_v = t_v - (Rt_v v_posed_v + T0_v);  Sb = sum b;  r1 = sum_v S_v^T (Rt_v^T b_v);
//   mb_q = sum_v w_vq b_v for the joint slots q of the current SEGMENT (a run of pieces whose joints number <= kGQ).
// grid (Mp/64, ncells / mult / kBW), block 64*kBW: wave = one share (mult cells) of one instance block.  The four joints of the current
// piece live in registers (PieceJoints, with T0 as the translation) and so do their four moment accumulators; at the
// end of a piece the wave adds them into ITS rows of the LDS accumulator [kBW][kGQ x 3][64] (lane-private columns,
// plain read-add-write: no atomics) and, behind the last piece of a segment (piece record [10] >= 0), moves the
// segment's rows to ws.resP.  The waves never meet: no barrier.
// Output: ws.resP = [cell][16][Mp] ([r1 : S][Sb : 3]) followed by [segment row][kGQ x 3][Mp] (moments).
constexpr size_t kResidualLds = (size_t)kBW * kGQ * 3 * 64 * 4;
// (res_share_rec(S), the floats of a cell record, and kResRowRec = 3 kGQ, those of a segment row: sf_tables.h)

#ifndef SMPLFIT_RES_WAVES
#define SMPLFIT_RES_WAVES 4
#endif
template <int S, int NJ = 4>
__global__ __launch_bounds__(64 * kBW) __attribute__((amdgpu_waves_per_eu((NJ == 8 || S > 12) ? 2 : SMPLFIT_RES_WAVES, (NJ == 8 || S > 12) ? 2 : SMPLFIT_RES_WAVES))) void k_residual_bm(
    DevModel m, ShareView sv, Workspace ws, int B, int Mp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int STRIDE = sf::jd_stride(S), BW = brec_w(S), BS = brec_stride(S, NJ), RS = kPieceRec * (NJ / 4);
  constexpr int kResShareRec = res_share_rec(S);
  constexpr int SP = (S + 1) / 2;  // register pairs of r1 (odd S: the last pair's second half is unused)
  constexpr int NM = kGQ * 3;      // moment rows of a wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int share = blockIdx.y * kBW + wave, blk = blockIdx.x, J = m.J, Vp = m.Vp;
  const int bcol = blk * 64 + lane;
  const int b = bcol < B ? bcol : B - 1;
  const int Np = (J * STRIDE + 63) / 64 * 64;
  const float* jdb = ws.jdT + (size_t)blk * Np * 64 + lane;
  // the wave's moment accumulators (the slots of a segment) start at zero
  float* macc = smem + (size_t)wave * NM * 64 + lane;
#pragma unroll
  for (int r = 0; r < NM; ++r) macc[r * 64] = 0.f;
  // The stream holds the targets as given: they are centred here (t - mean is the float the centred copy used to
  // hold).  The mean lives in registers: an LDS read inside the loop would share its counter with the scalar loads
  // of the next vertex's record and make every wait for it a wait for them.
  const float mu0 = ws.mean[(size_t)b * 3], mu1 = ws.mean[(size_t)b * 3 + 1], mu2v = ws.mean[(size_t)b * 3 + 2];
  // a piece's joints from the instance-innermost copy of the joint rows (ws.jdT): 12 coalesced 256-byte reads each
  PieceJointsT<NJ> jr;
  auto load_joints = [&](const_i32_ptr rec) {
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      const float* row = jdb + (size_t)piece_joint(rec, k) * STRIDE * 64;
      float r[12];  // R0..R8, T0x T0y T0z
#pragma unroll
      for (int i = 0; i < 12; ++i) r[i] = row[i * 64];
      jr.p[k][0] = mk2(r[0], r[3]);
      jr.p[k][1] = mk2(r[1], r[4]);
      jr.p[k][2] = mk2(r[2], r[5]);
      jr.p[k][3] = mk2(r[6], r[7]);
      jr.p[k][4] = mk2(r[8], r[11]);
      jr.p[k][5] = mk2(r[9], r[10]);
    }
  };
  f2 r1p[SP], m01[NJ];
  float m2[NJ];
#pragma unroll
  for (int k = 0; k < SP; ++k) r1p[k] = mk2(0, 0);
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    m01[k] = mk2(0, 0);
    m2[k] = 0.f;
  }
  // wave-uniform stream bases + the lane as a 32-bit offset (scalar-base addressing)
  const float* vp = ws.vpT + (size_t)blk * 3 * Vp * 64;
  const float* tp = ws.tT + (size_t)blk * 3 * Vp * 64;
  const uint32_t ul = (uint32_t)lane;
  const size_t cstr = (size_t)Vp * 64;
  float sb[3] = {0.f, 0.f, 0.f};  // Sb = sum_v b_v = the sum of the moments: the skinning weights of a vertex sum to
                                  // one (route_of checks it), so the residual sum needs no accumulators of its own
  const int ps = sv.piece_start[share * sv.mult], np = sv.piece_start[(share + 1) * sv.mult] - ps;
  {
    // The wave's step sequence: the vertices of every piece in turn, plus one step on the first padding slot (zero
    // streams, all-zero record: contributes exactly 0) behind a piece with an odd number of vertices — see
    // k_lbs_partsum_bm.
    const int vpad = m.V;
    const_i32_ptr pc = as_constant(sv.pieces + (size_t)ps * RS);
    int vb = pc[9], len = pc[0];
    const int v0 = vb;
    // two resident records (this vertex's and the next one's, requested a step ahead) need 2 (3 S + 4) scalar registers:
    // with the kid unknown (S = 11) that is 74 of the ~100 a wave has and the loop spills — such a model loads ONE
    // record, at the head of its own step (the other three waves of the SIMD cover the round trip)
    constexpr bool kRecAhead = 2 * (3 * S + NJ) <= 68;
    VertexRec<S, NJ> recA, recB;
    if constexpr (kRecAhead) load_rec<S, NJ>(m.brec, v0, recA);
    auto request = [&](int v, StreamBuf& sb2) {
      const float* q = vp + (size_t)v * 64;
      const float* r = tp + (size_t)v * 64;
      sb2.x01.x = ld_stream<1>(q + ul); sb2.x01.y = ld_stream<1>(q + cstr + ul); sb2.xt2.x = ld_stream<1>(q + 2 * cstr + ul);
      sb2.t01.x = ld_stream<1>(r + ul); sb2.t01.y = ld_stream<1>(r + cstr + ul); sb2.xt2.y = ld_stream<1>(r + 2 * cstr + ul);
    };
    // two stream buffers used alternately: a buffer is refilled with the vertex two steps ahead as soon as its
    // values are consumed.  (Measured in round 3: the same requests issued by hand as inline assembly, pinned a true
    // two steps ahead with exact vmcnt waits, run at the same speed — the loop is not waiting for its streams — and
    // the compiler spills in-flight asm results under register pressure: not kept.)
    StreamBuf rA, rB;
    request(v0, rA);
    request(len > 1 ? v0 + 1 : vpad, rB);
    auto step = [&](int vcur, int vn1, int vn2, StreamBuf& buf, VertexRec<S, NJ>& rc, VertexRec<S, NJ>& rn) {
      if constexpr (kRecAhead) rec_arrived_request_next<S, NJ>(m.brec, rc, vn1, rn);  // this vertex's record is here; the next one's is requested
      else load_rec<S, NJ>(m.brec, vcur, rc);
      // (S = 11: the four weights land in an odd-aligned run of scalar registers; hipcc then builds the pairs some packed
      // operations want THROUGH SCRATCH — a store and a reload per step, and the reload's wait drains every stream
      // request: the weights are moved to vector registers by hand instead)
      float cwv[NJ];
      if constexpr (!kRecAhead) {
#pragma unroll
        for (int k = 0; k < NJ; ++k) asm volatile("v_mov_b32 %0, %1" : "=v"(cwv[k]) : "s"(rc.w[k]));
      }
      const float (&cw)[NJ] = kRecAhead ? rc.w : cwv;
      const float (&rec)[3 * S] = rc.sd;
      // blend of the piece's 4 joints: (R0,R3) (R1,R4) (R2,R5) (R6,R7) (R8,T0z) (T0x,T0y)
      f2 Q[6];  // (joint-outer order: independent instructions back to back, see k_lbs_partsum_bm)
#pragma unroll
      for (int i = 0; i < 6; ++i) Q[i] = mk2(0, 0);
#pragma unroll
      for (int k = 0; k < NJ; ++k)
#pragma unroll
        for (int i = 0; i < 6; ++i) Q[i] += cw[k] * jr.p[k][i];
      // residual
      // (the two z values are consumed through ONE packed operation, so that they stay an aligned register pair of
      // this buffer — see StreamBuf)
      const f2 zz = buf.xt2 - mk2(0.f, mu2v);  // (x2, t2 - mean2)
      const f2 pos01 = (Q[0] * buf.x01.x + Q[1] * buf.x01.y) + (Q[2] * zz.x + Q[5]);
      const float pos2 = (Q[3].x * buf.x01.x + Q[3].y * buf.x01.y) + (Q[4].x * zz.x + Q[4].y);
      const f2 b01 = (buf.t01 - mk2(mu0, mu1)) - pos01;
      const float b2 = zz.y - pos2;
      request(vn2, buf);  // the buffer is consumed: refill it with the vertex two steps ahead
      // u = Rt^T b
      const float u0 = (Q[0].x * b01.x + Q[0].y * b01.y) + Q[3].x * b2;
      const float u1 = (Q[1].x * b01.x + Q[1].y * b01.y) + Q[3].y * b2;
      const float u2 = (Q[2].x * b01.x + Q[2].y * b01.y) + Q[4].x * b2;
      // (odd S: the second half of the last pair is unused — and must not index past the record's rows)
      auto row2 = [&](int base, int k) { return mk2(rec[base + 2 * k], 2 * k + 1 < S ? rec[base + 2 * k + 1] : 0.f); };
#pragma unroll
      for (int k = 0; k < SP; ++k) r1p[k] += (row2(0, k) * u0 + row2(S, k) * u1) + row2(2 * S, k) * u2;
#pragma unroll
      for (int k = 0; k < NJ; ++k) {
        m01[k] += cw[k] * b01;
        m2[k] += cw[k] * b2;
      }
    };
    for (int p = 0; p < np; ++p) {
      const bool more = p + 1 < np;
      const int len_next = more ? pc[RS] : 0, vn = more ? pc[RS + 9] : vpad, l2 = len + (len & 1);
      load_joints(pc);
      // The joints are "used" HERE (empty asm statements), so their loads — which the compiler would otherwise sink
      // to their first use inside the vertex loop — are complete before it: the loop is left with nothing but its
      // own requests pending and its waits are exact partial waits (the other buffer stays in flight), not vmcnt(0).
#pragma unroll
      for (int k = 0; k < NJ; ++k)
#pragma unroll
        for (int i = 0; i < 6; ++i) asm volatile("" : "+v"(jr.p[k][i].x), "+v"(jr.p[k][i].y));
      auto at = [&](int i) {  // (scalar selects, no branches: the step pair stays one scheduling region)
        const int k = i - l2;
        int r = ((k >= 0) & (k < len_next)) ? vn + k : vpad;
        r = i < len ? vb + i : r;
        return r;
      };
      for (int i = 0; i < l2; i += 2) {
        step(vb + i, at(i + 1), at(i + 2), rA, recA, kRecAhead ? recB : recA);
        step(at(i + 1), at(i + 2), at(i + 3), rB, kRecAhead ? recB : recA, recA);
      }
      // end of the piece: its four moment sums go to the wave's accumulator rows of the joints' segment slots (two
      // padding joints of a piece may share a slot: the adds are sequential)
#pragma unroll
      for (int k = 0; k < NJ; ++k) {
        float* a = macc + (size_t)piece_slot(pc, k) * 3 * 64;
        a[0] += m01[k].x;
        a[64] += m01[k].y;
        a[128] += m2[k];
        m01[k] = mk2(0, 0);
        m2[k] = 0.f;
      }
      const int row = pc[10];
      if (row >= 0) {  // end of a segment: its moment rows leave the accumulator
        float* out = ws.resP + ((size_t)sv.ncells * kResShareRec + (size_t)row * kResRowRec) * Mp + bcol;
        const int nr = 3 * (pc[11] & 0xff);
        for (int r = 0; r < nr; r += 3) {
          const float x = macc[r * 64], y = macc[(r + 1) * 64], z = macc[(r + 2) * 64];
          out[(size_t)r * Mp] = x;
          out[(size_t)(r + 1) * Mp] = y;
          out[(size_t)(r + 2) * Mp] = z;
          sb[0] += x; sb[1] += y; sb[2] += z;
          macc[r * 64] = 0.f; macc[(r + 1) * 64] = 0.f; macc[(r + 2) * 64] = 0.f;
        }
        const int cell = (pc[11] >> 8) - 1;
        if (cell >= 0) {  // end of a cell: its record r1 | Sb; the sums restart (the rows do not depend on the multiplier)
          float* oc = ws.resP + (size_t)cell * kResShareRec * Mp + bcol;
#pragma unroll
          for (int k = 0; k < SP; ++k) {
            oc[(size_t)(2 * k) * Mp] = r1p[k].x;
            if (2 * k + 1 < S) oc[(size_t)(2 * k + 1) * Mp] = r1p[k].y;
            r1p[k] = mk2(0, 0);
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            oc[(size_t)(S + c) * Mp] = sb[c];
            sb[c] = 0.f;
          }
        }
      }
      vb = vn;
      len = len_next;
      pc += RS;
    }
  }
}

// K3g (batch-major): the Gramian of the vertex block from the rotations alone (the "pair-Gram" form of
// sf::pair_gram_stage), lane = instance.  With Q_p = R_j1^T R_j2 for the joint pairs p = (j1, j2) that share a vertex,
// D_j = R_j^T T'_j and the host constants c1 / c2 / c3 of the pairs (and of the single joints),
//   G[i,i2] = g0 + sum_p sum_{a,a'} Q_p[a][a'] E_p[a a'][i,i2]                        E = c1 symmetrised (HostTables::pair_E)
//                + sym( sum_j [ A_j D_j + T'_j^T Z_j ] )[i,i2]                        sym(M) = M + M^T
//   A_j[x][a] = c2_jj[a][x] + sum_{p ni j} sum_b (R_j^T R_o)[a][b] c2_p[b][x]        o = the pair's other joint
//   Z_j       = 1/2 c3_jj T'_j + sum_{p ni j} 1/2 c3_p T'_o                           (D_j1^T Q_p D_j2 = T'_j1^T T'_j2)
// — the second and third term of every pair (c2^T U + D1^T V in sf::pair_gram_stage) regrouped BY JOINT, so that the
// bilinear products are J instead of (number of pairs): 0.11 MFLOP per instance where the pair-by-pair form of
// round 3 took 0.25, and every constant arrives through scalar loads (that form staged 900 constants per pair in
// LDS and read them back as broadcasts: 256 registers, 100 B of scratch, a quarter of its VALU issue bound).
// Work units of an instance block: the J joints twice (A_j, D_j and their product; Z_j and its product — one unit
// each: together they would not fit the 128 registers of four waves per SIMD) and chunks of kPgPairs pairs (the E
// term); a wave takes ONE unit, the kPgWaves waves of a workgroup add their upper triangles through LDS
// in a fixed order.  grid (ceil(units / kPgWaves), Mp/64).  Output: ws.gramP[workgroup][NG][Mp].
#ifndef SMPLFIT_PG_UNROLL
#define SMPLFIT_PG_UNROLL 9
#endif
// (kPgWaves, kPgPairs: smplfit_hip.hip, beside pair_gram_units — the workspace carve uses the same constants)
constexpr int kPgRound = 8;  // register pairs of the triangle added per LDS round (kPgWaves x kPgRound x 64 x 8 B = 32 KB)

// (S > 12: the triangle alone is 136+ registers — two waves per SIMD)
template <int S>
__global__ __launch_bounds__(64 * kPgWaves) __attribute__((amdgpu_waves_per_eu(S > 12 ? 2 : 4, S > 12 ? 2 : 4))) void k_pair_gram_bm(DevModel m, Workspace ws, int B, int Mp) {
  constexpr int STRIDE = sf::jd_stride(S), ROW = sf::jd_row(S), NG = sf::ne_ng(S), NGP = (NG + 3) / 4 * 4, NP2 = NGP / 2;
  constexpr int SE = (S + 1) & ~1, SP = SE / 2;
  __shared__ f2 red[kPgWaves][kPgRound][64];
  const int tid = threadIdx.x, lane = tid & 63, J = m.J, np = m.jt.np;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int unit = blockIdx.x * kPgWaves + wave;
  const int npc = (np + kPgPairs - 1) / kPgPairs;
  const int Np = (J * STRIDE + 63) / 64 * 64;
  const float* jdb = ws.jdT + (size_t)blockIdx.y * Np * 64;
  const uint32_t ul = (uint32_t)lane;
  // ONE register array for the two kinds of unit: a pair chunk accumulates its upper triangle in V[0, NP2); a joint
  // unit keeps its two 3 x S factors X = V[0, 3 SP), Y = V[3 SP, 6 SP) (declared apart, the compiler keeps both
  // alive through the reduction and spills)
  constexpr int NV = NP2 > 6 * SP ? NP2 : 6 * SP;
  f2 V[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) V[k] = mk2(0.f, 0.f);
#define SF_X(q, k) V[(q) * SP + (k)]
#define SF_Y(q, k) V[(3 + (q)) * SP + (k)]
  auto load_R = [&](int j, float (&R)[9]) {
    const float* row = jdb + (size_t)j * STRIDE * 64;  // wave-uniform
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (row + k * 64)[ul];
  };
  auto load_T = [&](int j, f2 (&T)[3 * SP]) {  // T'_j (3 x S), rows padded to SE with zero
    const float* row = jdb + ((size_t)j * STRIDE + 12) * 64;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < SP; ++k) {
        T[c * SP + k].x = (row + (c * ROW + 2 * k) * 64)[ul];
        T[c * SP + k].y = 2 * k + 1 < S ? (row + (c * ROW + 2 * k + 1) * 64)[ul] : 0.f;
      }
  };
  // a joint unit's result is the symmetrised product of two 3 x S factors, sym(X^T Y)[i,i2] = sum_r X[r][i] Y[r][i2] +
  // X[r][i2] Y[r][i]: the factors stay in registers and the entries are formed round by round where the workgroup
  // adds its waves' triangles (a unit never holds the whole triangle beside its factors)
  // the entries [2 r0, 2 (r0 + kPgRound)) of the triangle as register pairs (every index a compile-time constant once
  // the loops are unrolled: an index the compiler cannot fold would put the whole array into scratch)
  auto sym_round = [&](int r0, f2 (&v)[kPgRound]) {
#pragma unroll
    for (int k = 0; k < kPgRound; ++k) v[k] = mk2(0.f, 0.f);
    int e = 0;
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int i2 = i; i2 < S; ++i2, ++e) {
        if (e / 2 < r0 || e / 2 >= r0 + kPgRound) continue;
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float xi = (i & 1) ? SF_X(q, i / 2).y : SF_X(q, i / 2).x, xi2 = (i2 & 1) ? SF_X(q, i2 / 2).y : SF_X(q, i2 / 2).x;
          const float yi = (i & 1) ? SF_Y(q, i / 2).y : SF_Y(q, i / 2).x, yi2 = (i2 & 1) ? SF_Y(q, i2 / 2).y : SF_Y(q, i2 / 2).x;
          acc += xi * yi2 + xi2 * yi;
        }
        if (e & 1) v[e / 2 - r0].y = acc;
        else v[e / 2 - r0].x = acc;
      }
  };
  const bool joint_unit = unit < 2 * J;
  if (unit < J) {
    // ---- joint unit, first product: sym(A_j D_j)
    const int j = unit;
    const const_i32_ptr jn = as_constant(m.jn);
    const int n0 = m.jn_start[j], n1 = m.jn_start[j + 1];
    float Rj[9];
    load_R(j, Rj);
    {  // A[a][x] = X
      const const_f32_ptr c2 = as_constant(m.diag_c2e + (size_t)j * 3 * SE);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < SP; ++k) SF_X(a, k) = mk2(c2[a * SE + 2 * k], c2[a * SE + 2 * k + 1]);
    }
    for (int n = n0; n < n1; ++n) {
      const int o = jn[2 * n], p = jn[2 * n + 1];
      float Ro[9];
      load_R(o, Ro);
      const const_f32_ptr c2 = as_constant(m.pair_c2e + (size_t)p * 3 * SE);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b2 = 0; b2 < 3; ++b2) {
          const float q = (Rj[a] * Ro[b2] + Rj[3 + a] * Ro[3 + b2]) + Rj[6 + a] * Ro[6 + b2];  // (R_j^T R_o)[a][b]
#pragma unroll
          for (int k = 0; k < SP; ++k) SF_X(a, k) += q * mk2(c2[b2 * SE + 2 * k], c2[b2 * SE + 2 * k + 1]);
        }
    }
    f2 Tj[3 * SP];  // T'_j -> Y = D_j = R_j^T T'_j
    load_T(j, Tj);
#pragma unroll
    for (int k = 0; k < SP; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) SF_Y(a, k) = (Rj[a] * Tj[k] + Rj[3 + a] * Tj[SP + k]) + Rj[6 + a] * Tj[2 * SP + k];
  } else if (unit < 2 * J) {
    // ---- joint unit, second product: sym(T'_j^T Z_j)
    const int j = unit - J;
    const const_i32_ptr jn = as_constant(m.jn);
    const int n0 = m.jn_start[j], n1 = m.jn_start[j + 1];
    f2 Tj[3 * SP];  // X = T'_j, Y = Z_j
    load_T(j, Tj);
    const float h = 0.5f * m.jt.diag_c3[j];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < SP; ++k) {
        SF_X(c, k) = Tj[c * SP + k];
        SF_Y(c, k) = h * Tj[c * SP + k];
      }
    for (int n = n0; n < n1; ++n) {
      const int o = jn[2 * n], p = jn[2 * n + 1];
      const float h2 = 0.5f * m.jt.pair_c3[p];
      f2 To[3 * SP];
      load_T(o, To);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < SP; ++k) SF_Y(c, k) += h2 * To[c * SP + k];
    }
  } else if (unit < 2 * J + npc) {
    // ---- a chunk of pairs: the E term
    const int p0 = (unit - 2 * J) * kPgPairs, p1 = min(p0 + kPgPairs, np);
    for (int p = p0; p < p1; ++p) {
      const int j1 = m.jt.pair_j[2 * p], j2 = m.jt.pair_j[2 * p + 1];
      float R1[9], R2[9];
      load_R(j1, R1);
      load_R(j2, R2);
      const const_f32_ptr E = as_constant(m.pair_E + (size_t)p * 9 * NGP);
#pragma unroll SMPLFIT_PG_UNROLL
      for (int aa = 0; aa < 9; ++aa) {
        const int a = aa / 3, a2 = aa - 3 * a;
        // Q[a][a2]: selected with scalar indices from registers (no indexed register access: three selects)
        const float r1a = a == 0 ? R1[0] : a == 1 ? R1[1] : R1[2], r1b = a == 0 ? R1[3] : a == 1 ? R1[4] : R1[5],
                    r1c = a == 0 ? R1[6] : a == 1 ? R1[7] : R1[8];
        const float r2a = a2 == 0 ? R2[0] : a2 == 1 ? R2[1] : R2[2], r2b = a2 == 0 ? R2[3] : a2 == 1 ? R2[4] : R2[5],
                    r2c = a2 == 0 ? R2[6] : a2 == 1 ? R2[7] : R2[8];
        const float q = (r1a * r2a + r1b * r2b) + r1c * r2c;
        const const_f32_ptr Er = E + aa * NGP;
#pragma unroll
        for (int k = 0; k < NP2; ++k) V[k] += q * mk2(Er[2 * k], Er[2 * k + 1]);
      }
    }
  }
  // ---- the workgroup's waves add their triangles in wave order, kPgRound register pairs per round
  const int bcol = blockIdx.y * 64 + lane;
  float* out = ws.gramP + (size_t)blockIdx.x * NG * Mp + bcol;
#pragma unroll
  for (int r0 = 0; r0 < NP2; r0 += kPgRound) {
    if (r0 > 0) __syncthreads();
    if (joint_unit) {
      f2 v[kPgRound];
      sym_round(r0, v);
#pragma unroll
      for (int k = 0; k < kPgRound; ++k)
        if (r0 + k < NP2) red[wave][k][lane] = v[k];
    } else {
#pragma unroll
      for (int k = 0; k < kPgRound; ++k)
        if (r0 + k < NP2) red[wave][k][lane] = V[r0 + k];
    }
    __syncthreads();
    if (wave < kPgRound && r0 + wave < NP2) {
      f2 sum = red[0][wave][lane];
#pragma unroll
      for (int w = 1; w < kPgWaves; ++w) sum += red[w][wave][lane];
      const int e = 2 * (r0 + wave);
      if (e < NG) out[(size_t)e * Mp] = sum.x;
      if (e + 1 < NG) out[(size_t)(e + 1) * Mp] = sum.y;
    }
  }
}
#undef SF_X
#undef SF_Y

// K3c: partial sums of the two kernels above -> the normal-equation record the solve stage reads
// (gramv: G | r1 | SA = 0 (closed form in the joint stage) | Sb | W = V) and the per-joint residual
// moments ws.mbj.  grid (ceil(B/256), S + 3 + 3 J + NG): blockIdx.y = output element.
template <int S>
__global__ __launch_bounds__(256) void k_gram_combine_bm(DevModel m, ShareView sv, Workspace ws, int B, int Mp) {
  constexpr int NG = sf::ne_ng(S), NE = sf::ne_size(S), kResShareRec = res_share_rec(S);
  const int b = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y, J = m.J;
  if (b >= B) return;
  double* out = ws.gramv + (size_t)b * (NE + 1);
  // rows [r0, r0 + n * step) of a buffer at column b, added in a FIXED order: eight rows requested together (a row at a
  // time the loop is one memory latency per row: 64 cell rows = most of the kernel), their sum formed as a tree
  auto sum_rows = [&](const float* buf, size_t r0, size_t step, int n) {
    float acc = 0.f;
    int g = 0;
    for (; g + 8 <= n; g += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = buf[(r0 + (size_t)(g + u) * step) * Mp + b];
      acc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    for (; g < n; ++g) acc += buf[(r0 + (size_t)g * step) * Mp + b];
    return acc;
  };
  if (e < S + 3) {  // r1 / Sb: cells in table order
    const float acc = sum_rows(ws.resP, (size_t)e, kResShareRec, sv.ncells);
    out[e < S ? NG + e : NG + 4 * S + (e - S)] = (double)acc;
    if (e == 0) {
      for (int k = 0; k < 3 * S; ++k) out[NG + S + k] = 0.0;
      out[NE] = (double)m.V;  // w_sum = num_vertices (bodyfitter.py:1038-1040)
    }
  } else if (e < S + 3 + 3 * J) {  // residual moment of joint j, coordinate c
    const int j = (e - S - 3) / 3, c = (e - S - 3) % 3;
    float acc = 0.f;
    for (int k = sv.aux_start[j]; k < sv.aux_start[j + 1]; ++k)  // segments in table order
      acc += ws.resP[((size_t)sv.aux_rows[k] + c) * Mp + b];
    ws.mbj[((size_t)b * J + j) * 3 + c] = acc;
  } else {  // Gramian entry: instance-independent part + the chunks of the pair kernel
    const int k = e - (S + 3 + 3 * J);
    int i = 0, r = k;
    while (r >= S - i) {
      r -= S - i;
      ++i;
    }
    const int nwg = pair_gram_workgroups(J, m.jt.np);
    const float acc = m.jt.diag_g0[i * S + i + r] + sum_rows(ws.gramP, (size_t)k, NG, nwg);
    out[k] = (double)acc;
  }
}

// ------------------------------------------------------------------------------------------------
// K1p (batch-major, round 6): the shape PROLOGUE of the joint stage with LANE = INSTANCE and a WAVE PER JOINT — what
// sf::joint_stage does behind its rotations (bodyfitter.py:869-916 and the joint block :1051-1053, _gram_block
// :1598-1625) with a wave per one / two instances: FK positions with their beta-Jacobian, T = P - G J_ext, the relative
// rotations as the GEMM's pose features, the joint rows the vertex kernels read, the joint block of the normal
// equations (+ the closed-form vertex SA).  k_joint_stage then only fits the rotations (do_prologue = 0) and leaves an
// instance-innermost copy ws.GT of them.  In the wave-per-instance stage those phases were three of its four equal
// chains (level FK 17 k, joint rows 19 k, 99 wave sums 22 k of 86 k cycles, 24 of 32 lanes busy); here
//   * the level-by-level FK is a SUM ALONG THE JOINT'S ANCESTORS, root first — P_j = J_ext_0 + sum_k G_(a_k) bone_(a_(k+1))
//     in the order the levels add them, so the positions are the same floats — which makes every joint independent:
//     no LDS state, no barrier; the ancestors' rotations are coalesced 256-byte rows of ws.GT, the bones scalar loads;
//   * the joint rows go STRAIGHT to ws.jdT (256-byte rows: the transpose launch is gone) and P to ws.pextT, which
//     k_solve_bm stages with 16-byte requests instead of gathering the instance-major ws.pext;
//   * a joint's three rows' terms of the 99 sums of the joint block stay in its wave's registers; the eight waves of a
//     workgroup add them through LDS (a tree in a fixed order) and write ONE partial record ws.gramjP[workgroup], which
//     k_solve_bm adds in workgroup order (the sums differ from the wave stage's lane tree in the last bits only).
// grid (Mp / 64, ceil(J / kProWaves)), block 64 kProWaves; a wave beyond the last joint contributes zeros.
// ------------------------------------------------------------------------------------------------
struct PrologueArgs {
  const float* tj;  // (B, J, 3) centred target joints (given or regressed)
  const float* jw;  // (B, J) or null
  int joint_block, joint_block_weighted, sa_closed_form, B;
  int planes;  // the pose features go to the GEMM's split-bf16 planes ws.rpP instead of ws.rp (Route::gemm_planes)
};
constexpr int kProChain = 5;  // ancestors' rotations requested together

template <int S>
__global__ __launch_bounds__(64 * kProWaves) void k_prologue_bm(DevModel m, PrologueArgs a, Workspace ws, int Mp) {
  constexpr int S1 = S + 1, STRIDE = sf::jd_stride(S), ROW = sf::jd_row(S), NG = sf::ne_ng(S), NE = sf::ne_size(S), NE1 = NE + 1;
  constexpr int SE = (S + 1) & ~1, NR = kProWaves / 2;
  extern __shared__ __attribute__((aligned(16))) float red[];  // [NR][NE1][64]
  const int tid = threadIdx.x, lane = tid & 63, blk = blockIdx.x, J = m.J;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = blockIdx.y * kProWaves + wave;
  const int bcol = blk * 64 + lane, b = bcol < a.B ? bcol : a.B - 1;
  const size_t pitch = (size_t)Mp;
  const float* GT = ws.GT + bcol;
  float acc[NE1];  // this joint's terms of the record: G (upper triangle) | r | SA (3 S) | Sb (3) | W
#pragma unroll
  for (int e = 0; e < NE1; ++e) acc[e] = 0.f;
  if (j < J) {
    const sf::JointTabs& tb = m.jt;
    const const_f32_ptr jext = as_constant(tb.j_ext), bext = as_constant(tb.bone_ext);
    // ---- FK along the chain of ancestors (sf::joint_stage :892-907, level by level: the same additions in the same order)
    float P[3][S1];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int s = 0; s < S1; ++s) P[c][s] = jext[c * S1 + s];  // root row: J_ext_0
    const int c0 = m.anc_start[j], d = m.anc_start[j + 1] - c0;
    float Gp[9];  // the parent's rotation (the last ancestor's)
#pragma unroll
    for (int k = 0; k < 9; ++k) Gp[k] = 0.f;
    for (int k0 = 0; k0 < d; k0 += kProChain) {
      float Ga[kProChain][9];
#pragma unroll
      for (int u = 0; u < kProChain; ++u) {
        const int an = m.anc[c0 + (k0 + u < d ? k0 + u : d - 1)];
#pragma unroll
        for (int k = 0; k < 9; ++k) Ga[u][k] = GT[(size_t)(an * 9 + k) * pitch];
      }
#pragma unroll
      for (int u = 0; u < kProChain; ++u)
        if (k0 + u < d) {
          // the joint this step reaches: the next ancestor, or j itself behind the last one
          const int nx = k0 + u + 1 < d ? m.anc[c0 + k0 + u + 1] : j;
          const const_f32_ptr be = bext + (size_t)nx * 3 * S1;
#pragma unroll
          for (int s = 0; s < S1; ++s) {
            const float b0 = be[s], b1 = be[S1 + s], b2 = be[2 * S1 + s];
#pragma unroll
            for (int c = 0; c < 3; ++c) P[c][s] = P[c][s] + (Ga[u][c * 3] * b0 + Ga[u][c * 3 + 1] * b1 + Ga[u][c * 3 + 2] * b2);
          }
#pragma unroll
          for (int k = 0; k < 9; ++k) Gp[k] = Ga[u][k];
        }
    }
    float Gj[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Gj[k] = GT[(size_t)(j * 9 + k) * pitch];
    // ---- T = P - G J_ext (:909-911); the joint's row of ws.jdT; P to ws.pextT
    float T[3][S1];
    {
      const const_f32_ptr je = jext + (size_t)j * 3 * S1;
#pragma unroll
      for (int s = 0; s < S1; ++s) {
        const float e0 = je[s], e1 = je[S1 + s], e2 = je[2 * S1 + s];
#pragma unroll
        for (int c = 0; c < 3; ++c) T[c][s] = P[c][s] - (Gj[c * 3] * e0 + Gj[c * 3 + 1] * e1 + Gj[c * 3 + 2] * e2);
      }
    }
    {
      float* row = ws.jdT + ((size_t)blk * ((J * STRIDE + 63) / 64 * 64) + (size_t)j * STRIDE) * 64 + lane;
#pragma unroll
      for (int k = 0; k < 9; ++k) row[k * 64] = Gj[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        row[(9 + c) * 64] = T[c][0];
#pragma unroll
        for (int s = 0; s < ROW; ++s) row[(12 + c * ROW + s) * 64] = s < S ? T[c][1 + s] : 0.f;
      }
#pragma unroll
      for (int k = 12 + 3 * ROW; k < STRIDE; ++k) row[k * 64] = 0.f;
      float* pe = ws.pextT + (size_t)(j * 3) * S1 * pitch + bcol;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int s = 0; s < S1; ++s) pe[(size_t)(c * S1 + s) * pitch] = P[c][s];
    }
    // ---- relative rotations -> pose features (:869-876, :913); the constant features behind them by the root's wave
    // a.planes: as the split-bf16 planes the GEMM multiplies (ws.rpP, sf::plane_off: the bits its own front end would
    // split from ws.rp) INSTEAD of the fp32 rows, which only that front end reads behind this kernel — the row stores
    // are the expensive ones (a cache line per lane and feature; a plane store covers 32 lanes with four); the pad
    // lanes up to Mp write zeros there (every lane of a GEMM wave reads its run)
    const bool live = bcol < a.B;
    float* rp = ws.rp + (size_t)b * tb.Kp;
    char* pl = reinterpret_cast<char*>(ws.rpP);
    auto feature = [&](int p, float x) {
      const int pos = sf::rp_pos(p, tb.Kp);
      if (!a.planes) {
        if (live) rp[pos] = x;
      } else {
        const sf::Bf16x3 t = sf::split_bf16x3(live ? x : 0.f);
        *reinterpret_cast<__bf16*>(pl + sf::plane_off(bcol, pos, 0)) = t.h;
        *reinterpret_cast<__bf16*>(pl + sf::plane_off(bcol, pos, 1)) = t.m;
        if ((pos >> 4) == sf::kPlaneSteps - 1) *reinterpret_cast<__bf16*>(pl + sf::plane_off(bcol, pos, 2)) = t.l;
      }
    };
    if (j > 0) {
      float rel[9];
      sf::m3_tmul(Gp, Gj, rel);
#pragma unroll
      for (int k = 0; k < 9; ++k) feature((j - 1) * 9 + k, rel[k]);
    } else {
      for (int k = 0; k < tb.Kp - tb.P; ++k) feature(tb.P + k, k == 0 ? 1.f : 0.f);
    }
    // ---- this joint's rows of the joint block (sf::joint_gram_by_joint: the same per-row terms) + the closed-form vertex SA
    const float w = a.joint_block_weighted ? a.jw[(size_t)b * J + j] : 1.0f;
    const float cw = a.sa_closed_form ? tb.cw_joint[j] : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (a.joint_block) {
        const float dd = a.tj[((size_t)b * J + j) * 3 + c] - P[c][0];
#pragma unroll
        for (int i = 0; i < S; ++i) {
          const float wp = w * P[c][1 + i];
#pragma unroll
          for (int k = i; k < S; ++k) acc[sf::ne_g(S, i, k)] += wp * P[c][1 + k];
          acc[NG + i] += wp * dd;
          acc[NG + S + c * S + i] += wp;
        }
        acc[NG + 4 * S + c] += dd * w;
      }
      if (a.sa_closed_form) {  // sum_v Jac_v[c][i] = sum_j (G_j CS_j)[c][i] + cw_j T'_j[c][i]
        const const_f32_ptr cs = as_constant(tb.cs_joint) + (size_t)j * 3 * S;
#pragma unroll
        for (int i = 0; i < S; ++i)
          acc[NG + S + c * S + i] += (Gj[c * 3] * cs[i] + Gj[c * 3 + 1] * cs[S + i] + Gj[c * 3 + 2] * cs[2 * S + i]) + cw * T[c][1 + i];
      }
    }
    if (a.joint_block) acc[NE] += w;
    (void)SE;
  }
  // ---- the workgroup's waves add their records: (w, w + NR) -> w, then pairs again, in a fixed order
#pragma unroll
  for (int half = NR; half >= 1; half >>= 1) {
    if (wave >= half && wave < 2 * half) {
#pragma unroll
      for (int e = 0; e < NE1; ++e) red[((wave - half) * NE1 + e) * 64 + lane] = acc[e];
    }
    __syncthreads();
    if (wave < half) {
#pragma unroll
      for (int e = 0; e < NE1; ++e) acc[e] += red[(wave * NE1 + e) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* out = ws.gramjP + (size_t)blockIdx.y * NE1 * pitch + bcol;
#pragma unroll
    for (int e = 0; e < NE1; ++e) out[(size_t)e * pitch] = acc[e];
  }
}

// ------------------------------------------------------------------------------------------------
// K6' (batch-major, round 6): the dependent refinement + the epilogue (sf::refine_stage, bodyfitter.py:1418-1544 and
// :513-539) with LANE = INSTANCE, and the part-sum combine of the last LBS pass folded in.  k_refine_epilogue runs a
// wave per one / two instances with a lane per JOINT: the five levels of the refinement are a dependent chain in which
// two or three lanes compute an fp64 projection each while the others wait (40 us at 4096 instances, 84 at 16384).
// Here a workgroup of kRefWaves waves owns 64 instances (one per lane) and its WAVES take the joints:
//   phase 0  the block's target / reference joints (instance-major, 64 consecutive instances are one contiguous run:
//            coalesced) transposed into LDS; the part sums of the adjustable parts straight from the rows of the last
//            LBS pass (ws.psumP: instance-innermost, the rows of a part added in table order — k_psum_combine's order,
//            whose launch behind that pass is skipped); shape, translation, mean per lane.
//   phase 1  rest joints from the shape, bones, the root position (:1441-1460, :1481), a wave per (joint, coordinate).
//   phase 2  the adjustable parts (:1505-1537) BY DEPENDENCY instead of by level: a part's refinement needs the FK
//            position of its joint, i.e. the refined rotations of its adjustable ANCESTORS only — the reference's level
//            batches serialise the legs (hip, knee, ankle) with the arms (shoulder, elbow): five projections in a row
//            where the longest chain has three.  The parts are grouped by their top-most adjustable ancestor, a wave
//            takes a group in level order and walks each part's ancestors from the root itself (:1491-1498: the same
//            additions in the same order as the level FK) — no barrier inside the phase.  Per part: cross-covariance
//            about the FK position, the children's joint terms, proj_so3 for 64 instances at once, composed with the
//            part's rotation; all rotations live in LDS (ws.GT staged in phase 0, the refined ones written in place).
//   phase 3  relative rotations and the log map (:523-539), a wave per joint; pose (and the optional orientation
//            outputs) through an LDS tile so that the caller's instance-major rows are written coalesced.
// The arithmetic of every value is that of sf::refine_stage on the same inputs.  grid Mp / 64, block 64 * kRefWaves.
// Applies with k_prologue_bm (ws.GT valid), models of at most 32 joints (the LDS budget) — route_of.
// ------------------------------------------------------------------------------------------------
constexpr int kRefPitch = 65;  // LDS pitch of the transposed joint arrays (the fill walks k at a fixed instance)
constexpr int kRefParts = 4;   // adjustable parts of one group at most (a wave keeps their part sums in registers)
__host__ __device__ inline int refine_bm_lds_floats(int J) { return 2 * 3 * J * kRefPitch + 2 * 3 * J * 64 + 9 * J * kRefPitch; }
// The two pieces of data movement that k_refine_bm and the K1r kernels below share (lane = instance, column bcol).
// The part sums of one part, added onto ps (the caller zeroes it): its rows of the last LBS pass (psumP,
// instance-innermost) in table order — k_psum_combine's order —, AHEAD rows requested together, then added in turn.  The
// adds, and so the bits, do not depend on AHEAD or CLAMP.  Requests behind the part's last row are skipped (k_rotations_spread,
// AHEAD 8: a part has two to seven rows) or, CLAMP, repeat the last row (the three callers with AHEAD 4: one straight run
// of requests; skipping them costs k_refine_bm<10> two registers, 169 against 167, which is an occupancy step).
template <int AHEAD, bool CLAMP = false>
__device__ __forceinline__ void gather_part_sums(const ShareView& sv, const float* __restrict__ psumP, int part, size_t pitch,
                                                 int bcol, float (&ps)[sf::kPsum]) {
  const int q0 = sv.aux_start[part], q1 = sv.aux_start[part + 1];
  for (int q = q0; q < q1; q += AHEAD) {
    float v[AHEAD][sf::kPsum];
#pragma unroll
    for (int r = 0; r < AHEAD; ++r)
      if (CLAMP || q + r < q1) {
        const float* src = psumP + (size_t)sv.aux_rows[q + r < q1 ? q + r : q1 - 1] * sf::kPsum * pitch + bcol;
#pragma unroll
        for (int k = 0; k < sf::kPsum; ++k) v[r][k] = src[(size_t)k * pitch];
      }
#pragma unroll
    for (int r = 0; r < AHEAD; ++r)
      if (q + r < q1) {
#pragma unroll
        for (int k = 0; k < sf::kPsum; ++k) ps[k] += v[r][k];
      }
  }
}
// The target / reference joints of the block's ni instances from i0 on (rows of J3 consecutive floats; rj_stride 0: one
// reference row for all), transposed into LDS with pitch kRefPitch: wave w takes the instances w, w + kRefWaves, ...,
// NH requests of 64 lanes cover a row (J3 <= 64 NH), every request before the first LDS store; with NH = 3 a request that
// lies wholly behind the row is skipped (wave-uniform), with two both are made (a model of 22 .. 32 joints needs both, and
// the straight run of requests is what k_refine_bm and k_rotations_bm were measured with).  No barrier in here.
template <int NH>
__device__ __forceinline__ void stage_block_joints(const float* __restrict__ tj, const float* __restrict__ rj, size_t rj_stride,
                                                   int i0, int ni, int J3, int wave, int lane, float* tjs, float* rjs) {
  float tv[64 / kRefWaves][NH], rv[64 / kRefWaves][NH];
#pragma unroll
  for (int u = 0; u < 64 / kRefWaves; ++u) {
    const int inst = wave + u * kRefWaves, ii = inst < ni ? inst : ni - 1;
    const float* tg = tj + (size_t)(i0 + ii) * J3;
    const float* rg = rj + (size_t)(i0 + ii) * rj_stride;
#pragma unroll
    for (int h = 0; h < NH; ++h)
      if (NH <= 2 || 64 * h < J3) {
        const int k = lane + 64 * h, kk = k < J3 ? k : J3 - 1;
        tv[u][h] = tg[kk];
        rv[u][h] = rg[kk];
      }
  }
#pragma unroll
  for (int u = 0; u < 64 / kRefWaves; ++u) {
    const int inst = wave + u * kRefWaves;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int k = lane + 64 * h;
      if (k < J3) {
        tjs[k * kRefPitch + inst] = tv[u][h];
        rjs[k * kRefPitch + inst] = rv[u][h];
      }
    }
  }
}
template <int S>
__global__ __launch_bounds__(64 * kRefWaves) void k_refine_bm(DevModel m, RefineArgs a, ShareView sv, Workspace ws, const float* rj_true,
                                                                int Mp, RefGroups rg) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int S1 = S + 1;
  const sf::JointTabs& tb = m.jt;
  const int J = tb.J, J3 = 3 * J, B = a.B;
  const int nadj = a.final_adjust ? tb.adj_level_start[tb.adj_last_level + 1] : 0;
  float* tjs = smem;                       // [3 J][65] joints of the joint term
  float* rjs = tjs + J3 * kRefPitch;       // [3 J][65] reference joints of the joint term
  float* Ts = rjs + J3 * kRefPitch;        // [3 J][64] bones
  float* pos = Ts + J3 * 64;               // [3 J][64] rest joints from the shape, then FK positions
  float* Rs = pos + J3 * 64;               // [J][9][65] rotations: as fitted (ws.GT), the adjustable parts refined in place (the
                                           // orientations are written to the caller's rows straight from here: pitch 65)
  const int tid = threadIdx.x, lane = tid & 63, blk = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bcol = blk * 64 + lane, b = bcol < B ? bcol : B - 1;
  const size_t pitch = (size_t)Mp;
  const int i0 = blk * 64, ni = min(64, B - i0);
  auto load_R = [&](int j, float (&R)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rs[(j * 9 + k) * kRefPitch + lane];
  };
  // ---- phase 0: every global read of the kernel, requested before anything is used
  float beta[S], trans[3];
#pragma unroll
  for (int s = 0; s < S; ++s) beta[s] = ws.beta[(size_t)b * S + s];
#pragma unroll
  for (int c = 0; c < 3; ++c) trans[c] = ws.trans[(size_t)b * 3 + c];
  float ps[kRefParts][sf::kPsum], ca[kRefParts][3];
  int mine[kRefParts];
  if (a.final_adjust) {
    // the wave's adjustable parts: their part sums — the rows of the last LBS pass in table order (k_psum_combine's
    // order; four rows requested together) — and their joints at the final solve
    // the wave's parts in level order (at most kRefParts: route_of)
    for (int u = 0, ai = 0; u < kRefParts; ++u) {
      while (ai < nadj && rg.wave[ai] != wave) ++ai;
      mine[u] = ai < nadj ? ai++ : -1;
    }
#pragma unroll
    for (int u = 0; u < kRefParts; ++u) {
      const int ai = mine[u];
#pragma unroll
      for (int k = 0; k < sf::kPsum; ++k) ps[u][k] = 0.f;
      if (ai >= 0) {
        const int prt = tb.adj_parts[ai];
        gather_part_sums<4, true>(sv, ws.psumP, prt, pitch, bcol, ps[u]);
#pragma unroll
        for (int c = 0; c < 3; ++c) ca[u][c] = rj_true[((size_t)b * J + prt) * 3 + c];
      }
    }
    // target / reference joints of the block, transposed (J <= 32: at most two requests of 64 lanes per row)
    stage_block_joints<2>(a.tj, a.rj_term, (size_t)J3, i0, ni, J3, wave, lane, tjs, rjs);
  }
  {  // the rotations as fitted: rows of 64 instances, nine requests in flight per step
    const float* GT = ws.GT + bcol;
    for (int r0 = wave * 9; r0 < J * 9; r0 += kRefWaves * 9) {
      float v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] = GT[(size_t)(r0 + k) * pitch];
#pragma unroll
      for (int k = 0; k < 9; ++k) Rs[(r0 + k) * kRefPitch + lane] = v[k];
    }
  }
  if (a.final_adjust) {
    // ---- phase 1: rest joints from the shape (pos), bones, root position
    for (int k = wave; k < J3; k += kRefWaves) {
      const const_f32_ptr je = as_constant(tb.j_ext) + (size_t)k * S1;
      float acc = 0.f;
#pragma unroll
      for (int s = 0; s < S; ++s) acc += je[1 + s] * beta[s];
      float v = je[0] + acc;
      if (a.scaled) v *= ws.scale[b];
      pos[k * 64 + lane] = v;
    }
    __syncthreads();
    for (int k = wave; k < J3; k += kRefWaves) {
      const int j = k / 3, c = k - 3 * j;
      Ts[k * 64 + lane] = pos[k * 64 + lane] - (j > 0 ? pos[(tb.parents[j] * 3 + c) * 64 + lane] : 0.f);
    }
    __syncthreads();
    if (wave < 3) pos[wave * 64 + lane] = pos[wave * 64 + lane] + trans[wave];  // root position (rest joint of the root + trans)
    __syncthreads();
    // ---- phase 2: the wave's group, ancestors first; no barrier (a part reads refined rotations of its own group only)
#pragma unroll
    for (int u = 0; u < kRefParts; ++u) {
      const int ai = mine[u];
      if (ai < 0) continue;
      const int i = tb.adj_parts[ai];
      // FK position of the joint from the root along its ancestors (the level FK's additions in the same order)
      float ct[3] = {pos[lane], pos[64 + lane], pos[128 + lane]};
      const int c0 = m.anc_start[i], d = m.anc_start[i + 1] - c0;
      for (int k = 0; k < d; ++k) {
        const int p = m.anc[c0 + k], j = k + 1 < d ? m.anc[c0 + k + 1] : i;
        float Rp[9], rb[3];
        load_R(p, Rp);
        const float bone[3] = {Ts[(j * 3) * 64 + lane], Ts[(j * 3 + 1) * 64 + lane], Ts[(j * 3 + 2) * 64 + lane]};
        sf::m3_vec(Rp, bone, rb);
#pragma unroll
        for (int c = 0; c < 3; ++c) ct[c] = ct[c] + rb[c];
      }
      float A[9];
      sf::centered_cov(ps[u], ps[u] + 9, ps[u] + 12, ps[u][15], ct, ca[u], A);
      for (int m0 = tb.cas_start[i]; m0 < tb.cas_start[i + 1]; ++m0) {
        const int mj = tb.cas_flat[m0];
        const float w = a.jw ? a.jw[(size_t)b * J + mj] : 1.0f;
        float est[3], dfl[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          est[c] = tjs[(mj * 3 + c) * kRefPitch + lane] - ct[c];
          dfl[c] = (rjs[(mj * 3 + c) * kRefPitch + lane] - ca[u][c]) * w;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) A[r * 3 + c] += est[r] * dfl[c];
      }
      float Rf[9], Gi[9], Rn[9];
      sf::proj_so3(A, Rf);
      load_R(i, Gi);
      sf::m3_mul(Rf, Gi, Rn);
#pragma unroll
      for (int k = 0; k < 9; ++k) Rs[(i * 9 + k) * kRefPitch + lane] = Rn[k];
    }
    __syncthreads();
  } else {
    __syncthreads();
  }
  // ---- phase 3: relative rotations, log map.  The pose and the relative rotations go through LDS tiles
  // [64 instances][row + 1] over the dead joint arrays (one pass over the joints when both tiles fit), the orientations
  // straight from Rs (pitch 65: a transposed read is conflict-free too) — the caller's instance-major rows are written
  // as runs of consecutive floats.
  float* tile = smem;  // (over tjs .. pos: nothing below reads them)
  auto src_joint = [&](int j) { return (a.final_adjust && tb.toe_src[j] >= 0) ? tb.toe_src[j] : j; };  // toes copy the feet (:1539-1543)
  auto store_rows = [&](float* out, const float* t, int n, int TP) {  // n floats per instance from a tile to the caller's rows
    for (int inst = wave; inst < ni; inst += kRefWaves) {
      float* row = out + (size_t)(i0 + inst) * n;
      for (int k = lane; k < n; k += 64) row[k] = t[inst * TP + k];
    }
  };
  const int TPp = J3 + 1, TPr = 9 * J + 1;
  float* tile_r = tile + 64 * TPp;
  const bool both = a.rel && 64 * (TPp + TPr) <= 2 * J3 * kRefPitch + 2 * J3 * 64;
  for (int j = wave; j < J; j += kRefWaves) {
    float Rj[9], rel[9], rv[3];
    load_R(src_joint(j), Rj);
    if (j > 0) {
      float Rp[9];
      load_R(src_joint(tb.parents[j]), Rp);
      sf::m3_tmul(Rp, Rj, rel);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) rel[k] = Rj[k];
    }
    sf::mat2rotvec(rel, rv);
#pragma unroll
    for (int c = 0; c < 3; ++c) tile[lane * TPp + j * 3 + c] = rv[c];
    if (both) {
#pragma unroll
      for (int k = 0; k < 9; ++k) tile_r[lane * TPr + j * 9 + k] = rel[k];
    }
  }
  if (a.orient) {  // (reads Rs only: no barrier needed in front)
    constexpr int NH = (32 * 9 + 63) / 64;  // J <= 32
    int off[NH];  // the lane's elements k = lane + 64 h of a row: where they sit in Rs (a toe's come from its foot)
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int k = lane + 64 * h, kk = k < J * 9 ? k : 0, j = kk / 9;
      off[h] = (src_joint(j) * 9 + (kk - 9 * j)) * kRefPitch;
    }
    for (int inst = wave; inst < ni; inst += kRefWaves) {
      float* row = a.orient + (size_t)(i0 + inst) * J * 9;
#pragma unroll
      for (int h = 0; h < NH; ++h)
        if (lane + 64 * h < J * 9) row[lane + 64 * h] = Rs[off[h] + inst];
    }
  }
  __syncthreads();
  store_rows(a.pose, tile, J3, TPp);
  if (a.rel) {
    if (both) {
      store_rows(a.rel, tile_r, J * 9, TPr);
    } else {  // (fewer than 22 joints: the second tile does not fit beside the first)
      __syncthreads();
      for (int j = wave; j < J; j += kRefWaves) {
        float Rj[9], rel[9];
        load_R(src_joint(j), Rj);
        if (j > 0) {
          float Rp[9];
          load_R(src_joint(tb.parents[j]), Rp);
          sf::m3_tmul(Rp, Rj, rel);
        } else {
#pragma unroll
          for (int k = 0; k < 9; ++k) rel[k] = Rj[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) tile[lane * TPr + j * 9 + k] = rel[k];
      }
      __syncthreads();
      store_rows(a.rel, tile, J * 9, TPr);
    }
  }
  if (wave == 0 && bcol < B) {
    const int nb = S - tb.n_kid - tb.n_pad;
    if (a.betas)
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (s < nb) a.betas[(size_t)b * nb + s] = beta[s];
    if (tb.n_kid && a.kid) a.kid[b] = beta[S - 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) a.trans[(size_t)b * 3 + c] = trans[c] + ws.mean[(size_t)b * 3 + c];
  }
}

// ------------------------------------------------------------------------------------------------
// K1r (batch-major, round 6): the part ROTATIONS of the joint stage (sf::joint_stage up to its prologue,
// _fit_global_rotations, bodyfitter.py:1321-1416, toes :147-156, composition :422-433) with LANE = INSTANCE, the
// part-sum combine in front of it folded in.  The parts are independent of each other, so this is k_refine_bm's scheme
// without a chain: a workgroup of kRefWaves waves owns 64 instances, wave w takes the joints w, w + 8, ...; phase 0
// requests everything from global memory — the part sums of the wave's parts straight from the rows of the pass that
// produced them (ws.psumP, a part's rows in table order: k_psum_combine's order, whose launch is gone), the previous
// rotations of its joints (ws.GT, in place; the first pass of a warm-started fit reads the instance-major ws.G), the
// block's target / reference joints transposed into LDS (coalesced: 64 consecutive instances are one run) —, phase 1
// fits every part's rotation (Kabsch on the part's joints, swing + twist of a bone part, or the projection of the
// cross-covariance of its vertices: the code of sf::joint_stage per lane), phase 2 gives the toes their feet's
// rotations, composes with the previous ones and writes ws.GT rows (coalesced).  k_prologue_bm follows.
// grid Mp / 64, block 64 * kRefWaves.  Applies with k_refine_bm (route_of).
// ------------------------------------------------------------------------------------------------
constexpr int kRotJoints = 4;   // joints a wave fits per round (their part sums and previous rotations in registers)
constexpr int kRotMaxJ = 64;    // (three 64-lane requests cover a row of 3 J joint coordinates)
struct RotArgs {
  const float* tj;    // (B, J, 3) centred target joints (given or regressed)
  const float* rj;    // (B, J, 3) reference joints, or (J, 3) when rj_shared
  const float* jw;    // (B, J) or null
  const float* Gim;   // (B, J, 9) previous rotations, instance-major (gprev_mode 2)
  int rj_shared;
  int gprev_mode;     // 0: none (identity); 1: ws.GT; 2: Gim
  int B;
  int8_t slot[kRotMaxJ];  // the joint's slot among the joints a toe copies, or -1 (host: rot_bm_slots)
};
__host__ __device__ inline int rot_bm_lds_floats(int J) { return J <= kRotJoints * kRefWaves ? 2 * 3 * J * kRefPitch + 9 * J * 64 : 2 * 3 * J * kRefPitch + kRotSlots * 9 * 64; }
// ---- The arithmetic of K1r, stated ONCE for the three kernels below: the fit of one part on one lane (part_rotation)
// and the composition with the previous rotation (compose_prev).  The kernels must return the same bits (a call takes
// one or another by its size; tests/test_gpu_rot_spread.py), and the compiler contracts a * b + c * d by how it happens
// to pack the products of an inlined site in pairs, so the expressions on which that showed — each was a last bit of a
// rotation — have every rounding spelled out here, and these are the only statements of them:
//   the centred covariance (centered_cov_k1r: three fused steps per element, the product ct ca rounded first);
//   the middle element of H = R_swing A^T inside the swing + twist (swing_twist_k1r: sf::swing_twist with that one
//     statement added — (third product, rounded) + fma(second, (first product, rounded)));
//   the weighted sums of the multi-joint Kabsch (part_rotation: every sum fused but sa[0]);
//   the composition (compose_prev: fma(r2 g2, fma(r0 g0, r1 g1)), and its first element on models of up to 32 joints).
// Everything else is sf:: code whose results did not depend on the site.
__device__ __forceinline__ void centered_cov_k1r(const float* raw, const float* st, const float* sa, float sw, const float* ct,
                                                 const float* ca, float* A) {  // sf::centered_cov
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      A[r * 3 + c] = __builtin_fmaf(sw, ct[r] * ca[c], __builtin_fmaf(-ct[r], sa[c], __builtin_fmaf(-st[r], ca[c], raw[r * 3 + c])));
}
__device__ inline void swing_twist_k1r(const float* b_ref, const float* b_tgt, const float* A, float* R) {  // sf::swing_twist
  const float nr = sqrtf(b_ref[0] * b_ref[0] + b_ref[1] * b_ref[1] + b_ref[2] * b_ref[2]);
  const float nt = sqrtf(b_tgt[0] * b_tgt[0] + b_tgt[1] * b_tgt[1] + b_tgt[2] * b_tgt[2]);
  const float br[3] = {sf::divide_no_nan(b_ref[0], nr), sf::divide_no_nan(b_ref[1], nr), sf::divide_no_nan(b_ref[2], nr)};
  const float bt[3] = {sf::divide_no_nan(b_tgt[0], nt), sf::divide_no_nan(b_tgt[1], nt), sf::divide_no_nan(b_tgt[2], nt)};
  float Rsw[9], H[9];
  sf::align_unit_vectors(br, bt, Rsw);
  sf::m3_mult(Rsw, A, H);  // H = R_swing A^T
  {
#pragma clang fp contract(off)
    const float p3 = Rsw[3] * A[3], p5 = Rsw[5] * A[5];
    H[4] = p5 + __builtin_fmaf(Rsw[4], A[4], p3);
  }
  const float trH = H[0] + H[4] + H[8];
  float Hb[3];
  sf::m3_vec(H, bt, Hb);
  const float bHb = bt[0] * Hb[0] + bt[1] * Hb[1] + bt[2] * Hb[2];
  const float vee[3] = {H[5] - H[7], H[6] - H[2], H[1] - H[3]};
  const float ang = atan2f(bt[0] * vee[0] + bt[1] * vee[1] + bt[2] * vee[2], trH - bHb);
  const float rv[3] = {bt[0] * ang, bt[1] * ang, bt[2] * ang};
  float Rtw[9];
  sf::rotvec2mat(rv, Rtw);
  sf::m3_mul(Rtw, Rsw, R);
}
// The rotation R of part f for the lane's instance b (sf::joint_stage up to its prologue, per lane): from the part's
// sums ps (gather_part_sums; read for bone and leaf parts only) and the block's joints in LDS (stage_block_joints).
__device__ __forceinline__ void part_rotation(const sf::JointTabs& tb, int f, const float (&ps)[sf::kPsum], const float* tjs,
                                              const float* rjs, int lane, const float* __restrict__ jw, int b, float (&R)[9]) {
  auto TJ = [&](int mj, int c) { return tjs[(mj * 3 + c) * kRefPitch + lane]; };
  auto RJ = [&](int mj, int c) { return rjs[(mj * 3 + c) * kRefPitch + lane]; };
  const int type = tb.part_type[f];
  sf::m3_identity(R);
  if (type == 0) return;
  const int c0 = tb.cas_start[f], n = tb.cas_start[f + 1] - c0;
  const float inv = 1.0f / (float)n;
  float ct[3] = {0, 0, 0}, ca[3] = {0, 0, 0};
  for (int q = 0; q < n; ++q) {
    const int mj = tb.cas_flat[c0 + q];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ct[c] += inv * TJ(mj, c);
      ca[c] += inv * RJ(mj, c);
    }
  }
  float A[9];
  if (type == 1) {  // multi-joint part: Kabsch on its joints only (:1361-1383)
    float raw[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, st[3] = {0, 0, 0}, sa[3] = {0, 0, 0}, sw = 0;
    for (int q = 0; q < n; ++q) {
      const int mj = tb.cas_flat[c0 + q];
      const float w = jw ? jw[(size_t)b * tb.J + mj] : 1.0f;
      const float t[3] = {TJ(mj, 0), TJ(mj, 1), TJ(mj, 2)}, rj[3] = {RJ(mj, 0), RJ(mj, 1), RJ(mj, 2)};
      // (the steps matter once w is not 1: every sum fused but sa[0], which adds the rounded product)
      float aa[3];
      {
#pragma clang fp contract(off)
        aa[0] = rj[0] * w, aa[1] = rj[1] * w, aa[2] = rj[2] * w;
        sa[0] = sa[0] + aa[0];
      }
      sa[1] = __builtin_fmaf(rj[1], w, sa[1]);
      sa[2] = __builtin_fmaf(rj[2], w, sa[2]);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) raw[r * 3 + c] = __builtin_fmaf(t[r], aa[c], raw[r * 3 + c]);
        st[r] = __builtin_fmaf(t[r], w, st[r]);
      }
      sw += w;
    }
    centered_cov_k1r(raw, st, sa, sw, ct, ca, A);
  } else {
    centered_cov_k1r(ps, ps + 9, ps + 12, ps[15], ct, ca, A);
  }
  if (type == 2) {  // bone part: swing + twist (:1389-1412)
    const int k0 = tb.cas_flat[c0], k1 = tb.cas_flat[c0 + 1];
    float br[3], bt[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      br[c] = RJ(k1, c) - RJ(k0, c);
      bt[c] = TJ(k1, c) - TJ(k0, c);
    }
    swing_twist_k1r(br, bt, A, R);
  } else {
    sf::proj_so3(A, R);
  }
}
// The previous rotation of joint j (gprev_mode 1: its row of ws.GT, GT at the lane's column; 2: the instance-major Gim).
__device__ __forceinline__ void load_prev(const RotArgs& a, const float* GT, size_t pitch, int J, int b, int j, float (&G)[9]) {
  if (a.gprev_mode == 1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = GT[(size_t)(j * 9 + k) * pitch];
  } else if (a.gprev_mode == 2) {
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = a.Gim[((size_t)b * J + j) * 9 + k];
  }
}
// G = R Gp, the composition with the previous rotation (:422-433; gprev_mode 0: G = R).  A toe whose previous rotation
// has its foot's bits gets its foot's bits.
// one_round: models of up to kRotJoints * kRefWaves = 32 joints round the FIRST element in another order, (r0 g0 rounded,
// then fma(r1, g3, .)) + (r2 g6 rounded) — what the one-round kernel gave when it left the product to the compiler, and
// what every fit of those models has returned since.  Kept as behaviour; the other eight elements do not differ.
__device__ __forceinline__ void compose_prev(const float (&R)[9], const float (&Gp)[9], int gprev_mode, bool one_round, float (&G)[9]) {
  if (gprev_mode != 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        G[r * 3 + c] = __builtin_fmaf(R[r * 3 + 2], Gp[6 + c], __builtin_fmaf(R[r * 3], Gp[c], R[r * 3 + 1] * Gp[3 + c]));
    if (one_round) {
#pragma clang fp contract(off)
      const float p0 = R[0] * Gp[0], p2 = R[2] * Gp[6];
      G[0] = __builtin_fmaf(R[1], Gp[3], p0) + p2;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = R[k];
  }
}
__device__ __forceinline__ void store_rotation_row(float* GT, size_t pitch, int j, const float (&G)[9]) {  // row j of ws.GT
#pragma unroll
  for (int k = 0; k < 9; ++k) GT[(size_t)(j * 9 + k) * pitch] = G[k];
}

// Models of at most kRotJoints * kRefWaves = 32 joints: ONE round — the wave's joints all at once, every rotation through
// LDS ([J][9][64]), the toes composed with the others behind one barrier.  (The form with rounds below, which carries the
// SMPL-X-shaped model, runs this case 6 us slower — 52 against 46 us with the prologue at 4096 instances —: kept apart.)
__global__ __launch_bounds__(64 * kRefWaves) void k_rotations_bm(DevModel m, RotArgs a, ShareView sv, Workspace ws, int Mp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const sf::JointTabs& tb = m.jt;
  const int J = tb.J, J3 = 3 * J, B = a.B;
  float* tjs = smem;                   // [3 J][65] centred target joints
  float* rjs = tjs + J3 * kRefPitch;   // [3 J][65] reference joints
  float* Rs = rjs + J3 * kRefPitch;    // [J][9][64] the parts' fitted rotations (a toe reads its foot's)
  const int tid = threadIdx.x, lane = tid & 63, blk = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bcol = blk * 64 + lane, b = bcol < B ? bcol : B - 1;
  const size_t pitch = (size_t)Mp;
  const int i0 = blk * 64, ni = min(64, B - i0);
  float* GT = ws.GT + bcol;
  // ---- phase 0: every global read
  float ps[kRotJoints][sf::kPsum], Gp[kRotJoints][9];
#pragma unroll
  for (int u = 0; u < kRotJoints; ++u) {
    const int j = wave + u * kRefWaves;
#pragma unroll
    for (int k = 0; k < sf::kPsum; ++k) ps[u][k] = 0.f;
    if (j >= J) continue;
    if (tb.part_type[j] >= 2) gather_part_sums<4, true>(sv, ws.psumP, j, pitch, bcol, ps[u]);  // bone and leaf parts
    load_prev(a, GT, pitch, J, b, j, Gp[u]);
  }
  stage_block_joints<2>(a.tj, a.rj, a.rj_shared ? (size_t)0 : (size_t)J3, i0, ni, J3, wave, lane, tjs, rjs);
  __syncthreads();
  // ---- phase 1: the parts' rotations
#pragma unroll
  for (int u = 0; u < kRotJoints; ++u) {
    const int j = wave + u * kRefWaves;
    if (j >= J) continue;
    float R[9];
    part_rotation(tb, j, ps[u], tjs, rjs, lane, a.jw, b, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) Rs[(j * 9 + k) * 64 + lane] = R[k];
  }
  __syncthreads();
  // ---- phase 2: toes take the feet (:147-156); compose with the previous rotations; rows of ws.GT
#pragma unroll
  for (int u = 0; u < kRotJoints; ++u) {
    const int j = wave + u * kRefWaves;
    if (j >= J) continue;
    const int src = tb.toe_src[j] >= 0 ? tb.toe_src[j] : j;
    float R[9], G[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rs[(src * 9 + k) * 64 + lane];
    compose_prev(R, Gp[u], a.gprev_mode, true, G);
    store_rotation_row(GT, pitch, j, G);
  }
}

// More joints (33 .. 64): rounds of kRotJoints joints per wave; only the rotations a toe copies go through LDS.
__global__ __launch_bounds__(64 * kRefWaves) void k_rotations_bm_rounds(DevModel m, RotArgs a, ShareView sv, Workspace ws, int Mp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const sf::JointTabs& tb = m.jt;
  const int J = tb.J, J3 = 3 * J, B = a.B;
  float* tjs = smem;                   // [3 J][65] centred target joints
  float* rjs = tjs + J3 * kRefPitch;   // [3 J][65] reference joints
  float* Rs = rjs + J3 * kRefPitch;    // [kRotSlots][9][64] fitted rotations of the joints a toe copies
  const int tid = threadIdx.x, lane = tid & 63, blk = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bcol = blk * 64 + lane, b = bcol < B ? bcol : B - 1;
  const size_t pitch = (size_t)Mp;
  const int i0 = blk * 64, ni = min(64, B - i0);
  float* GT = ws.GT + bcol;
  stage_block_joints<(3 * kRotMaxJ + 63) / 64>(a.tj, a.rj, a.rj_shared ? (size_t)0 : (size_t)J3, i0, ni, J3, wave, lane, tjs, rjs);
  // the wave's toes (at most two: route_of): their previous rotations are requested now, used behind the last barrier
  int toej[2] = {-1, -1};
  float Gtoe[2][9];
  for (int j = wave, n = 0; j < J; j += kRefWaves)
    if (tb.toe_src[j] >= 0 && n < 2) toej[n++] = j;
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (toej[u] >= 0) load_prev(a, GT, pitch, J, b, toej[u], Gtoe[u]);
  // ---- rounds of kRotJoints joints per wave: request (part sums, previous rotations), fit, compose and write; a toe
  // waits for its foot
  for (int r0 = 0; r0 < J; r0 += kRotJoints * kRefWaves) {
    float ps[kRotJoints][sf::kPsum], Gp[kRotJoints][9];
#pragma unroll
    for (int u = 0; u < kRotJoints; ++u) {
      const int j = r0 + wave + u * kRefWaves;
#pragma unroll
      for (int k = 0; k < sf::kPsum; ++k) ps[u][k] = 0.f;
      if (j >= J) continue;
      if (tb.part_type[j] >= 2) gather_part_sums<4, true>(sv, ws.psumP, j, pitch, bcol, ps[u]);  // bone and leaf parts
      if (tb.toe_src[j] < 0) load_prev(a, GT, pitch, J, b, j, Gp[u]);
    }
    if (r0 == 0) __syncthreads();  // (the joints in LDS)
#pragma unroll
    for (int u = 0; u < kRotJoints; ++u) {
      const int j = r0 + wave + u * kRefWaves;
      if (j >= J) continue;
      float R[9], G[9];
      part_rotation(tb, j, ps[u], tjs, rjs, lane, a.jw, b, R);
      const int sl = a.slot[j];
      if (sl >= 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) Rs[(sl * 9 + k) * 64 + lane] = R[k];
      }
      if (tb.toe_src[j] < 0) {
        compose_prev(R, Gp[u], a.gprev_mode, false, G);
        store_rotation_row(GT, pitch, j, G);
      }
    }
  }
  __syncthreads();
  // ---- toes take the feet (:147-156)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (toej[u] < 0) continue;
    const int sl = a.slot[tb.toe_src[toej[u]]];
    float R[9], G[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rs[(sl * 9 + k) * 64 + lane];
    compose_prev(R, Gtoe[u], a.gprev_mode, false, G);
    store_rotation_row(GT, pitch, toej[u], G);
  }
}

// K1r spread over the chip (calls of up to kRotSpreadMaxBatch instances; the two kernels above serve larger ones and
// SMPLFIT_ROT_SPREAD=0): ONE joint per wave.
// Workgroup (blk, y) owns the 64 instances of block blk and the joints y * kRefWaves .. + kRefWaves - 1; wave w fits the
// part of joint j = y * kRefWaves + w for its 64 lanes.  A toe (toe_src[j] >= 0) fits its FOOT's part itself — the same
// inputs through the same code, so the foot's bits — and composes with its own previous rotation: no rotation crosses
// waves, LDS holds only the block's transposed target / reference joints, and the one barrier is the one behind them.
// Every row of the part's sums is requested before the first add (kRotAhead rows a batch: the coarse cell tables give a
// part at most 7 rows, so one batch), added in table order: the sums, and with them every rotation, keep the bits of the
// kernels above.  The chain of a wave is one memory round trip, one projection and one row store.
// grid (Mp / 64, ceil(J / kRefWaves)), block 64 * kRefWaves.
constexpr int kRotAhead = 8;  // part-sum rows in flight per wave (16 registers each)
constexpr int kRotSpreadMaxBatch = 4096;  // most instances of a call that take this form (route_of; SMPLFIT_ROT_SPREAD_B)
__host__ __device__ inline int rot_spread_lds_floats(int J) { return 2 * 3 * J * kRefPitch; }
__global__ __launch_bounds__(64 * kRefWaves) void k_rotations_spread(DevModel m, RotArgs a, ShareView sv, Workspace ws, int Mp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const sf::JointTabs& tb = m.jt;
  const int J = tb.J, J3 = 3 * J, B = a.B;
  float* tjs = smem;                   // [3 J][65] centred target joints
  float* rjs = tjs + J3 * kRefPitch;   // [3 J][65] reference joints
  const int tid = threadIdx.x, lane = tid & 63, blk = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = blockIdx.y * kRefWaves + wave;  // the joint whose row of ws.GT the wave writes
  const bool live = j < J;
  const int f = live && tb.toe_src[j] >= 0 ? tb.toe_src[j] : live ? j : 0;  // the part it fits (a toe: its foot's)
  const int bcol = blk * 64 + lane, b = bcol < B ? bcol : B - 1;
  const size_t pitch = (size_t)Mp;
  const int i0 = blk * 64, ni = min(64, B - i0);
  float* GT = ws.GT + bcol;
  // ---- every global read: the part sums, the previous rotation, the block's joints
  float ps[sf::kPsum], Gp[9];
#pragma unroll
  for (int k = 0; k < sf::kPsum; ++k) ps[k] = 0.f;
  if (live) {
    if (tb.part_type[f] >= 2) gather_part_sums<kRotAhead>(sv, ws.psumP, f, pitch, bcol, ps);  // bone and leaf parts
    load_prev(a, GT, pitch, J, b, j, Gp);
  }
  stage_block_joints<(3 * kRotMaxJ + 63) / 64>(a.tj, a.rj, a.rj_shared ? (size_t)0 : (size_t)J3, i0, ni, J3, wave, lane, tjs, rjs);
  __syncthreads();
  if (!live) return;  // (a wave behind the last joint only took part in the transpose)
  // ---- the part's rotation, composed with the joint's own previous rotation; row j of ws.GT
  float R[9], G[9];
  part_rotation(tb, f, ps, tjs, rjs, lane, a.jw, b, R);
  compose_prev(R, Gp, a.gprev_mode, J <= kRotJoints * kRefWaves, G);
  store_rotation_row(GT, pitch, j, G);
}

// the rotations instance-innermost (ws.GT) -> instance-major (ws.G): the wave-per-instance refinement of a model whose
// joints do not fit k_refine_bm reads them there.  grid (Mp / 64, chunks of 16 joints), block 256.
__global__ __launch_bounds__(256) void k_gt_to_g(Workspace ws, int J, int B, int Mp) {
  __shared__ float tile[64 * (16 * 9 + 1)];
  constexpr int TP = 16 * 9 + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x;
  const int j0 = blockIdx.y * 16, nj = min(16, J - j0), n = nj * 9;
  const int i0 = blk * 64, ni = min(64, B - i0);
  const float* GT = ws.GT + (size_t)j0 * 9 * Mp + i0 + lane;
  for (int k = wave; k < n; k += 4) tile[lane * TP + k] = GT[(size_t)k * Mp];
  __syncthreads();
  for (int inst = wave; inst < ni; inst += 4) {
    float* row = ws.G + ((size_t)(i0 + inst) * J + j0) * 9;
    for (int k = lane; k < n; k += 64) row[k] = tile[inst * TP + k];
  }
}

// ------------------------------------------------------------------------------------------------
// K4' (batch-major, round 6): the normal-equation combine AND the shape solve as ONE kernel with LANE = INSTANCE —
// what k_gram_combine_bm + k_shape_solve (sf::solve_stage, a wave per one / two instances) do in two launches
// (17 + 29 us per 4096 instances, three times per fit; bodyfitter.py:1054-1101).
//
// A workgroup owns IB = 16 consecutive instances; a wave is RL = 64 / IB = 4 "row lanes" x 16 instances, so a row of
// partial sums (instance-innermost, written by k_residual_bm / k_pair_gram_bm) is read as 64-byte segments.  The
// workgroups of one 64-instance block are dealt to ONE XCD (block id % 8 = XCD) so that the 128-byte lines they share
// are fetched into that L2 once.  The kernel is a chain of memory round trips (the partial sums come from HBM / the
// Infinity Cache: the producers ran on other XCDs), so what counts is how few DEPENDENT ones there are:
//   phase A  every partial sum -> LDS in about two round trips: a thread ("slot" = wave x row lane, 64 per workgroup)
//            requests ALL rows of its bundles before it adds any —
//            T1 bundle (entry e of r1 | Sb, group of eight cells): the tree sum of the group;
//            T2 bundle (entry of the Gramian): the pair-Gram workgroups' rows in order + the instance-independent part;
//            T4 the joint block of the joint stage (ws.gramj, instance-major: gathered);
//            T3 a wave per joint, row lane = coordinate: the joint's residual-moment rows (CSR of the residual cell
//               table, wave-uniform: scalar loads) added in table order;
//            and the T0 | T' rows of ws.jdT, which phases B and D read (staged when the LDS has room: J <= 32).
//   phase B  a (task, instance) per thread, from LDS: the T' part of Jac^T b, sum_j T'_j^T mb_j, as kSolveParts partial
//            sums per unknown in fp64; the entries of the centred, regularised system and SA / W (one fp64 division
//            each: in one lane per instance they would be 95 divisions in a row); then (B') the right-hand side.
//   phase C  one lane per instance: the L D L^T factorisation with the system in a lane-private LDS column (55
//            doubles: beside x and 1 / D it would not fit the 128 registers of a 1024-thread workgroup),
//            substitutions in registers, translation.  The other threads hold the FK rows (ws.pext, gathered) they
//            requested before the phase.
//   phase D  joints and skinning translations at the solution for (joint, coordinate) x instance: ws.rjoints, ws.jb
//            and the instance-innermost ws.jbT the LBS pass reads.
// EVERY sum is formed in the order k_gram_combine_bm and sf::solve_stage form it (groups of eight rows as a tree, the
// groups and the left-over rows in turn; the joints of a run in turn; the same expressions in the solve), so the
// results are those of the two-kernel path bit for bit (tests/test_gpu_parity.py::test_solve_bm_matches_two_kernels)
// and do not depend on the batch an instance sits in.  grid align_up(Mp / IB, 8 RL), block 64 kSolveWaves.
// ------------------------------------------------------------------------------------------------
constexpr int kSolveWaves = 8;  // (8 waves: 256 registers per lane — at 16 waves / 128 registers the kernel spilled, and in this
                                // latency-bound code every reload is a memory round trip: phase D took 10 us)
constexpr int kSolveT3 = 64;  // most moment rows of a joint (coarse residual table) the kernel takes; the launch checks
__host__ __device__ constexpr size_t solve_bm_lds_bytes(int S, int IB, int J, int ncells, int maxn, bool stage) {
  return (size_t)IB * (8 * (sf::kSolveParts * S + S * S + 3 * S + 2 * (S + 3)) +
                       4 * (sf::ne_ng(S) + (S + 3) * (ncells / 8) + 3 * J + (sf::ne_size(S) + 1) + (S + 3) +
                            (stage ? 2 * 3 * J * (S + 1) + 1 : 0))) + (size_t)4 * J * maxn;
}
struct SolveBmArgs {
  float beta_reg, beta_reg2, kid_reg;
  int use_ref;
  int maxn;      // most moment rows of a joint, rounded up to a multiple of 16 (<= kSolveT3): row pitch of ShareView::aux_pad
  int lg_ngrp;   // log2(cells / 8)
  int stage_px;  // the joint rows (T0 | T') and the FK rows of the 16 instances are staged in LDS by phase A (they fit beside the sums: up to ~30 joints)
  int gj_parts;  // > 0: the joint block comes as this many partial records ws.gramjP of k_prologue_bm (else ws.gramj, instance-major)
  int pext_t;    // the FK rows come instance-innermost (ws.pextT of k_prologue_bm; else ws.pext, instance-major)
  uint32_t res_bytes, gram_bytes, jdt_bytes;  // sizes of ws.resP / ws.gramP / ws.jdT (buffer descriptors; < 2^31)
};
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
// four consecutive instances of a row of partial sums: 16 bytes at the lane's offset + a wave-uniform row offset
__device__ __forceinline__ f4 buf_load4(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// What shaped the kernel (phase stamps of a debug build, since removed: profiles/README.md, round 6 files): it is NOT bound by bytes or by memory
// latency but by how many vector-memory instructions a CU has to issue — the partial sums are rows of Mp floats, a
// workgroup of 16 instances owns 64 bytes of each of ~3600 rows, and a wave-wide dword request (four 64-byte pieces
// of four rows) occupied the CU's address path for ~20 cycles: 900 of them were 9 us, the address arithmetic and the
// 8600 instructions of the first, unrolled form another 10.  So a LANE HOLDS FOUR INSTANCES (16-byte requests: a
// wave-wide request covers 16 rows), every bundle of rows has its own lane (256 slots per workgroup: one bundle each,
// all of its rows requested before the first is added: one memory round trip), addresses are buffer offsets (the
// lane's (entry, instance quad) offset in one register + a wave-uniform row offset in the instruction's scalar
// operand; the moment rows' offsets prepared in LDS, padded with an out-of-range offset for which the hardware returns
// 0: no predication), and the phases are loops around small bodies.
template <int S, int IB>
__global__ __launch_bounds__(64 * kSolveWaves) void k_solve_bm(DevModel m, ShareView sv, Workspace ws, int B, int Mp, SolveBmArgs a) {
  static_assert(IB == 16, "a lane holds 4 of the workgroup's 16 instances");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NW = kSolveWaves, NSLOT = NW * 16, NG = sf::ne_ng(S), NE = sf::ne_size(S), NE1 = NE + 1;
  constexpr int REC = res_share_rec(S), STRIDE = sf::jd_stride(S), ROW = sf::jd_row(S), S1 = S + 1, NP = sf::kSolveParts;
  constexpr uint32_t kOob = 0x80000000u;  // (buffer sizes stay below 2^31 bytes: a request at this offset returns 0)
  const int J = m.J, ngrp = 1 << a.lg_ngrp, maxn = a.maxn;
  double* r2p = reinterpret_cast<double*>(smem);  // [NP * S][IB]; phase C: 1 / D in its first S rows
  double* Ms = r2p + NP * S * IB;                 // [S][S][IB] the system (lower triangle used)
  double* saw = Ms + S * S * IB;                  // [3 S][IB] SA / W
  double* xs = saw + 3 * S * IB;                  // [S + 3][IB] right-hand side, Sb / W
  double* chd = xs + (S + 3) * IB;                // [S + 3][IB] r1 | Sb of the vertex block + joint block (fp64)
  float* gv = reinterpret_cast<float*>(chd + (S + 3) * IB);  // [NG][IB] vertex block of the Gramian
  float* p1 = gv + NG * IB;                       // [(S + 3) ngrp][IB] group sums of r1 | Sb
  float* mbs = p1 + (S + 3) * ngrp * IB;          // [3 J][IB] residual moments
  float* fj = mbs + 3 * J * IB;                   // [NE + 1][IB] joint block
  float* bt = fj + NE1 * IB;                      // [S + 3][IB] shape, translation (fp32)
  uint32_t* moff = reinterpret_cast<uint32_t*>(bt + (S + 3) * IB);  // [J][maxn] byte offsets of the moment rows
  float* pxs = reinterpret_cast<float*>(moff + J * maxn);           // [3 J][S + 1][IB] FK rows (a.stage_px)
  float* tps = pxs + (a.stage_px ? ((3 * J * S1) | 1) * IB : 0);            // [3 J][S + 1][IB] T0 | T' of (joint, coordinate) (a.stage_px)
  // the four workgroups of a 64-instance block on one XCD
  const int wg = blockIdx.x, wslot = wg >> 3;
  const int grp = (((wslot >> 2) << 3) + (wg & 7)) * 4 + (wslot & 3);
  if (grp * IB >= B) return;
  const int tid = threadIdx.x, lane = tid & 63, quad = lane & 3;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slot = wave * 16 + (lane >> 2);  // one of 256 task slots; the lane holds the instances 4 quad .. 4 quad + 3 of it
  const int c0 = grp * IB + 4 * quad;        // first of its columns (< Mp: the partial-sum rows are complete up to Mp)
  const int i0 = 4 * quad;                   // ... and of its LDS columns
  const uint32_t Mp4 = (uint32_t)Mp * 4u, c4 = (uint32_t)c0 * 4u;
  const uint32_t jd0 = ((uint32_t)(c0 >> 6) * (uint32_t)((J * STRIDE + 63) / 64 * 64) * 64u + (uint32_t)(c0 & 63)) * 4u;
  const __amdgpu_buffer_rsrc_t rs_res = __builtin_amdgcn_make_buffer_rsrc(ws.resP, 0, a.res_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_gram = __builtin_amdgcn_make_buffer_rsrc(ws.gramP, 0, a.gram_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_jdt = __builtin_amdgcn_make_buffer_rsrc(ws.jdT, 0, a.jdt_bytes, 0x00020000);
  auto JD4 = [&](int e) { return buf_load4(rs_jdt, jd0 + (uint32_t)e * 256u, 0); };  // joint-row element e of the four instances
  auto LF4 = [&](const float* base, int e) { return *reinterpret_cast<const f4*>(base + e * IB + i0); };
  // T'[c][s2] (s2 >= 0) / T0[c] (s2 = -1) of joint j for the lane's four instances
  auto TP4 = [&](int j, int c, int s2) {
    if (a.stage_px) return LF4(tps, (j * 3 + c) * S1 + 1 + s2);
    return JD4(s2 < 0 ? j * STRIDE + 9 + c : j * STRIDE + 12 + c * ROW + s2);
  };
  auto tree8 = [](const f4* v) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); };
  auto bcl = [&](int u) { return c0 + u < B ? c0 + u : B - 1; };  // instance u of the lane, clamped (instance-major buffers)
  // ---------------- phase A: every partial sum -> LDS; a bundle of rows per slot
  {
    const int nwg = pair_gram_workgroups(J, m.jt.np), n1 = (S + 3) * ngrp, nb = n1 + NG + 3 * J;
    // ---- requests first, LDS stores last: the byte offsets of the joints' moment rows (ShareView::aux_pad: a row of
    // maxn per joint, -1 behind its last), the joint block of the joint stage (instance-major: gathered), and — staged
    // for phases B and D, which then read no global memory — the joint rows T0 | T' (ws.jdT: 16 bytes per row and lane)
    // and the FK rows (ws.pext, instance-major: a wave reads 64 consecutive floats of ONE instance's row, two cache lines
    // per request — with a lane per instance every lane of a request was in a line of its own: 9 us)
    const int nrow = 3 * J * S1, PXP = nrow | 1;  // PXP: LDS pitch of an instance's FK row (odd: the four instances of a lane fall into different banks)
    const int mrow0 = tid < J * maxn ? sv.aux_pad[tid] : -1, mrow1 = tid + 64 * NW < J * maxn ? sv.aux_pad[tid + 64 * NW] : -1;
    f4 st_g = {0.f, 0.f, 0.f, 0.f}, st_t[8];
    float st_p[2][IB];
    auto gramj4 = [&](int e) {  // entry e of the joint block for the lane's four instances
      f4 v;
      if (a.gj_parts > 0) {  // the prologue workgroups' partial records in workgroup order
        v = *reinterpret_cast<const f4*>(ws.gramjP + (size_t)e * Mp + c0);
        for (int q = 1; q < a.gj_parts; ++q) v += *reinterpret_cast<const f4*>(ws.gramjP + ((size_t)q * NE1 + e) * Mp + c0);
      } else {
        v.x = ws.gramj[(size_t)bcl(0) * NE1 + e];
        v.y = ws.gramj[(size_t)bcl(1) * NE1 + e];
        v.z = ws.gramj[(size_t)bcl(2) * NE1 + e];
        v.w = ws.gramj[(size_t)bcl(3) * NE1 + e];
      }
      return v;
    };
    if (slot < NE1) st_g = gramj4(slot);
    if (a.stage_px) {
#pragma unroll
      for (int h = 0; h < 8; ++h) {
        const int q = slot + h * NSLOT < nrow ? slot + h * NSLOT : 0, jc = q / S1, s2 = q - jc * S1, j = jc / 3, c = jc - 3 * j;
        st_t[h] = JD4(s2 == 0 ? j * STRIDE + 9 + c : j * STRIDE + 12 + c * ROW + (s2 - 1));
      }
      if (a.pext_t) {  // instance-innermost rows: 16 bytes per row and lane, as the joint rows (st_p holds 8 of them)
#pragma unroll
        for (int h = 0; h < 8; ++h) {
          const int q = slot + h * NSLOT < nrow ? slot + h * NSLOT : 0;
          const f4 v = *reinterpret_cast<const f4*>(ws.pextT + (size_t)q * Mp + c0);
          st_p[h >> 2][4 * (h & 3)] = v.x; st_p[h >> 2][4 * (h & 3) + 1] = v.y; st_p[h >> 2][4 * (h & 3) + 2] = v.z; st_p[h >> 2][4 * (h & 3) + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const int e = tid + g * 64 * NW < nrow ? tid + g * 64 * NW : 0;
#pragma unroll
          for (int h = 0; h < IB; ++h) st_p[g][h] = ws.pext[(size_t)(grp * IB + h < B ? grp * IB + h : B - 1) * nrow + e];
        }
      }
    }
    auto stage_store = [&]() {
      if (slot < NE1) *reinterpret_cast<f4*>(fj + slot * IB + i0) = st_g;
      for (int e = slot + NSLOT; e < NE1; e += NSLOT)  // (more than 128 entries: eleven unknowns)
        *reinterpret_cast<f4*>(fj + e * IB + i0) = gramj4(e);
      if (a.stage_px) {
#pragma unroll
        for (int h = 0; h < 8; ++h)
          if (slot + h * NSLOT < nrow) *reinterpret_cast<f4*>(tps + (slot + h * NSLOT) * IB + i0) = st_t[h];
        for (int q = slot + 8 * NSLOT; q < nrow; q += NSLOT) {  // (more than 1024 rows)
          const int jc = q / S1, s2 = q - jc * S1, j = jc / 3, c = jc - 3 * j;
          *reinterpret_cast<f4*>(tps + q * IB + i0) = JD4(s2 == 0 ? j * STRIDE + 9 + c : j * STRIDE + 12 + c * ROW + (s2 - 1));
        }
        if (a.pext_t) {  // LDS layout [row][16 instances], as the joint rows
#pragma unroll
          for (int h = 0; h < 8; ++h)
            if (slot + h * NSLOT < nrow) {
              f4 v = {st_p[h >> 2][4 * (h & 3)], st_p[h >> 2][4 * (h & 3) + 1], st_p[h >> 2][4 * (h & 3) + 2], st_p[h >> 2][4 * (h & 3) + 3]};
              *reinterpret_cast<f4*>(pxs + (slot + h * NSLOT) * IB + i0) = v;
            }
          for (int q = slot + 8 * NSLOT; q < nrow; q += NSLOT)
            *reinterpret_cast<f4*>(pxs + q * IB + i0) = *reinterpret_cast<const f4*>(ws.pextT + (size_t)q * Mp + c0);
        } else {
#pragma unroll
          for (int g = 0; g < 2; ++g)
            if (tid + g * 64 * NW < nrow) {
#pragma unroll
              for (int h = 0; h < IB; ++h) pxs[h * PXP + tid + g * 64 * NW] = st_p[g][h];
            }
          for (int e = tid + 2 * 64 * NW; e < nrow; e += 64 * NW)
#pragma unroll
            for (int h = 0; h < IB; ++h) pxs[h * PXP + e] = ws.pext[(size_t)(grp * IB + h < B ? grp * IB + h : B - 1) * nrow + e];
        }
      }
    };
    __builtin_amdgcn_sched_barrier(0);
    // ---- the bundles.  A slot's first bundle goes out BEFORE the barrier behind which the moment rows' offsets are
    // in LDS, unless it is a moment bundle; everything else behind it: two rounds of requests for the SMPL-shaped model
    auto bundle = [&](int q) {
      if (q < n1) {  // T1: entry e of r1 | Sb, group g of eight cells — the tree sum of the group (sum_rows)
        const int e = q >> a.lg_ngrp, g = q & (ngrp - 1);
        const uint32_t vo = (uint32_t)(8 * g * REC + e) * Mp4 + c4;
        f4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = buf_load4(rs_res, vo, (uint32_t)(u * REC) * Mp4);
        *reinterpret_cast<f4*>(p1 + q * IB + i0) = tree8(v);
      } else if (q < n1 + NG) {  // T2: Gramian entry k — the pair kernel's workgroups in order (full groups of eight as a
                                 // tree, the left-over rows in turn) + the instance-independent part
        const int k = q - n1;
        const uint32_t vo = (uint32_t)k * Mp4 + c4;
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int g = 0; g < nwg; g += 16) {
          f4 v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) v[u] = buf_load4(rs_gram, vo, (uint32_t)((g + u < nwg ? g + u : nwg - 1) * NG) * Mp4);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (g + 8 * h + 8 <= nwg) acc += tree8(v + 8 * h);
            else {
#pragma unroll
              for (int u = 0; u < 8; ++u)
                if (g + 8 * h + u < nwg) acc += v[8 * h + u];
            }
          }
        }
        int i = 0, rr = k;
        while (rr >= S - i) {
          rr -= S - i;
          ++i;
        }
        const float g0 = m.jt.diag_g0[i * S + i + rr];
        *reinterpret_cast<f4*>(gv + k * IB + i0) = g0 + acc;
      } else {  // T3: (joint, coordinate) — its moment rows in table order (k_gram_combine_bm: acc += row); the rows
                // behind the joint's last one come back as 0
        const int q3 = q - n1 - NG, j = q3 / 3, c = q3 - 3 * j;
        const uint32_t vo = (uint32_t)c * Mp4 + c4;
        const uint32_t* mj = moff + j * maxn;
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < maxn; k0 += 32) {
          f4 v[32];
#pragma unroll
          for (int h = 0; h < 2; ++h)
            if (k0 + 16 * h < maxn) {
#pragma unroll
              for (int u = 0; u < 16; ++u) v[16 * h + u] = buf_load4(rs_res, mj[k0 + 16 * h + u] + vo, 0);
            }
#pragma unroll
          for (int h = 0; h < 2; ++h)
            if (k0 + 16 * h < maxn) {
#pragma unroll
              for (int u = 0; u < 16; ++u) acc += v[16 * h + u];
            }
        }
        *reinterpret_cast<f4*>(mbs + q3 * IB + i0) = acc;
      }
    };
    const bool early = slot < n1 + NG;  // (not a moment bundle)
    if (early) bundle(slot);
    if (tid < J * maxn) moff[tid] = mrow0 >= 0 ? (uint32_t)mrow0 * Mp4 : kOob;
    if (tid + 64 * NW < J * maxn) moff[tid + 64 * NW] = mrow1 >= 0 ? (uint32_t)mrow1 * Mp4 : kOob;
    for (int t = tid + 2 * 64 * NW; t < J * maxn; t += 64 * NW) {  // (more than 1024 offsets)
      const int row = sv.aux_pad[t];
      moff[t] = row >= 0 ? (uint32_t)row * Mp4 : kOob;
    }
    __syncthreads();  // (plain loads — the staging requests — stay in flight across it)
    for (int q = early ? slot + NSLOT : slot; q < nb; q += NSLOT) bundle(q);
    stage_store();
  }
  __syncthreads();
  // ---------------- phase B: a (task, four instances) per lane, like the lanes of sf::solve_stage
  {
    auto FJ4 = [&](int e, double (&o)[4]) {
      const f4 v = LF4(fj, e);
      o[0] = (double)v.x; o[1] = (double)v.y; o[2] = (double)v.z; o[3] = (double)v.w;
    };
    double W[4];
    FJ4(NE, W);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      W[u] = (double)m.V + W[u];
      if (W[u] == 0.0) W[u] = 1.0;  // w_sum_safe (:1060)
    }
    const int run = (J + NP - 1) / NP;
    constexpr int NT = NP * S + NG + S + 3;  // (128 for ten unknowns: one task per slot)
    for (int t = slot; t < NT; t += NSLOT) {
      if (t < NP * S) {  // r2p[part][i] = sum over the joints of run `part` of T'_j[:, i] . mb_j
        const int i = t % S, part = t / S;
        const int j0 = part * run, j1 = (part + 1) * run < J ? (part + 1) * run : J;
        double r2[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = j0; j < j1; ++j) {
          f4 tv[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) tv[c] = TP4(j, c, i);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const f4 mb = LF4(mbs, j * 3 + c);
            r2[0] += (double)tv[c].x * (double)mb.x;
            r2[1] += (double)tv[c].y * (double)mb.y;
            r2[2] += (double)tv[c].z * (double)mb.z;
            r2[3] += (double)tv[c].w * (double)mb.w;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) r2p[t * IB + i0 + u] = r2[u];
      } else if (t < NP * S + NG) {  // entry (i, j <= i) of the lower triangle: G[j][i] - sum_c SA[c][i] SA[c][j] / W (+ lambda)
        const int k = t - NP * S;
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= k) ++i;
        const int j = k - i * (i + 1) / 2, e = sf::ne_g(S, j, i);
        const f4 gvv = LF4(gv, e), gjv = LF4(fj, e);
        f4 si[3], sj[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          si[c] = LF4(fj, NG + S + c * S + i);
          sj[c] = LF4(fj, NG + S + c * S + j);
        }
        const double lam = i == j ? sf::ridge_weight(m.jt, i, a.beta_reg, a.beta_reg2, a.kid_reg) : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          double g = (double)gvv[u] + (double)gjv[u];
          // (the unit-weight vertex SA is closed form in the joint stage: the vertex record holds 0)
          g -= ((0.0 + (double)si[0][u]) * (0.0 + (double)sj[0][u]) + (0.0 + (double)si[1][u]) * (0.0 + (double)sj[1][u]) +
                (0.0 + (double)si[2][u]) * (0.0 + (double)sj[2][u])) / W[u];
          if (i == j) g += lam;
          Ms[(i * S + j) * IB + i0 + u] = g;
        }
      } else {  // entry e of r1 | Sb: the groups in turn (sum_rows: acc += group), + the joint block
        const int e = t - (NP * S + NG);
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int g = 0; g < ngrp; g += 8) {
          f4 v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = LF4(p1, e * ngrp + (g + u < ngrp ? g + u : 0));
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (g + u < ngrp) acc += v[u];
        }
        double fjd[4];
        FJ4(e < S ? NG + e : NG + 4 * S + (e - S), fjd);
        chd[e * IB + i0 + 0] = (double)acc.x + fjd[0];
        chd[e * IB + i0 + 1] = (double)acc.y + fjd[1];
        chd[e * IB + i0 + 2] = (double)acc.z + fjd[2];
        chd[e * IB + i0 + 3] = (double)acc.w + fjd[3];
      }
    }
    __syncthreads();
    // ---------------- phase B': the right-hand side (and Sb / W) — needs the r2p of every run
    for (int t = slot; t < S + 3 + 3 * S; t += NSLOT) {
      if (t >= S + 3) {  // SA / W
        const int k = t - (S + 3);
        double sa[4];
        FJ4(NG + S + k, sa);
#pragma unroll
        for (int u = 0; u < 4; ++u) saw[k * IB + i0 + u] = (0.0 + sa[u]) / W[u];
        continue;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int col = i0 + u;
        if (t < S) {
          const int i = t;
          double v = chd[i * IB + col];
          double r2 = 0.0;
#pragma unroll
          for (int part = 0; part < NP; ++part) r2 += r2p[(part * S + i) * IB + col];
          v += r2;
          const double s0 = 0.0 + (double)fj[(NG + S + i) * IB + col], s1 = 0.0 + (double)fj[(NG + 2 * S + i) * IB + col],
                       s2 = 0.0 + (double)fj[(NG + 3 * S + i) * IB + col];
          double rr = v - (s0 * chd[S * IB + col] + s1 * chd[(S + 1) * IB + col] + s2 * chd[(S + 2) * IB + col]) / W[u];
          if (a.use_ref) rr += sf::ridge_weight(m.jt, i, a.beta_reg, a.beta_reg2, a.kid_reg) * (double)ws.regref[(size_t)bcl(u) * S + i];
          xs[i * IB + col] = rr;
        } else {
          xs[t * IB + col] = chd[t * IB + col] / W[u];  // Sb[c] / W
        }
      }
    }
  }
  __syncthreads();
  // ---------------- phase C: one lane per instance — L D L^T of the system in its LDS column (sf::ldlt_solve: the same
  // expressions; column by column, a non-positive pivot becomes NaN), substitutions in registers
  if (tid < IB) {
    const int inst = tid, bcol = grp * IB + inst, b = bcol < B ? bcol : B - 1;
    double* Mi = Ms + inst;
    double* rdl = r2p + inst;
    for (int k = 0; k < S; ++k) {
      const double dk = Mi[(k * S + k) * IB];
      const double rdk = dk > 0.0 ? 1.0 / dk : (dk - dk) / (dk - dk);
      rdl[k * IB] = rdk;
      const int n = S - 1 - k;  // trailing rows i2 = k + 1 + a, columns j2 = k + 1 + b2, b2 <= a
      double* Mk = Mi + ((k + 1) * S + k) * IB;  // M[k + 1][k]
      double l[S - 1];
#pragma unroll
      for (int a2 = 0; a2 < S - 1; ++a2) l[a2] = a2 < n ? Mk[(a2 * S) * IB] : 0.0;
#pragma unroll
      for (int a2 = 0; a2 < S - 1; ++a2) {
        if (a2 < n) {
          const double t = l[a2] * rdk;
#pragma unroll
          for (int b2 = 0; b2 <= a2; ++b2) Mk[(a2 * S + 1 + b2) * IB] -= t * l[b2];
        }
      }
    }
    double x[S], rd[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      x[i] = xs[i * IB + inst];
      rd[i] = rdl[i * IB];
    }
#pragma unroll
    for (int k = 0; k < S; ++k) {  // forward: y = L^-1 b
      const double yk = x[k] * rd[k];
#pragma unroll
      for (int i2 = k + 1; i2 < S; ++i2) x[i2] -= Mi[(i2 * S + k) * IB] * yk;
    }
#pragma unroll
    for (int i = 0; i < S; ++i) x[i] *= rd[i];  // z = D^-1 y
#pragma unroll
    for (int k = S - 1; k > 0; --k) {  // back: x = L^-T z
      const double xk = x[k];
#pragma unroll
      for (int i2 = 0; i2 < k; ++i2) x[i2] -= (Mi[(k * S + i2) * IB] * rd[i2]) * xk;
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
      bt[i * IB + inst] = (float)x[i];
      if (bcol < B) ws.beta[(size_t)b * S + i] = (float)x[i];
    }
    for (int c = 0; c < 3; ++c) {  // translation (:1086-1088)
      double v = xs[(S + c) * IB + inst];
#pragma unroll
      for (int i = 0; i < S; ++i) v -= saw[(c * S + i) * IB + inst] * x[i];
      bt[(S + c) * IB + inst] = (float)v;
      if (bcol < B) ws.trans[(size_t)b * 3 + c] = (float)v;
    }
  }
  __syncthreads();
  // ---------------- phase D: joints (:1093-1098) and skinning translations T0 + T' beta (:1099-1101) at the solution
  // (explicit fused multiply-adds: what the compiler makes of sf::solve_stage's loops; left to itself it pairs the
  // products of two items into packed multiplies here and adds them unfused)
  {
    f4 beta[S];
#pragma unroll
    for (int s = 0; s < S; ++s) beta[s] = LF4(bt, s);
    float* jbT = ws.jbT + ((size_t)(c0 >> 6) * J * 4) * 64 + (c0 & 63);
    for (int idx = slot; idx < 3 * J; idx += NSLOT) {  // a (joint, coordinate) for the lane's four instances
      const int j = idx / 3, c = idx - 3 * j;
      f4 tr[S];
#pragma unroll
      for (int s = 0; s < S; ++s) tr[s] = TP4(j, c, s);
      const f4 t0 = TP4(j, c, -1);
      f4 px[S1];  // the FK row of the four instances
      if (a.stage_px && a.pext_t) {
#pragma unroll
        for (int s = 0; s < S1; ++s) px[s] = LF4(pxs, idx * S1 + s);
      } else if (a.stage_px) {
        const int PXP = (3 * J * S1) | 1;
        const float* p0 = pxs + i0 * PXP + idx * S1;
#pragma unroll
        for (int s = 0; s < S1; ++s) {
          px[s].x = p0[s];
          px[s].y = p0[PXP + s];
          px[s].z = p0[2 * PXP + s];
          px[s].w = p0[3 * PXP + s];
        }
      } else if (a.pext_t) {
#pragma unroll
        for (int s = 0; s < S1; ++s) px[s] = *reinterpret_cast<const f4*>(ws.pextT + (size_t)(idx * S1 + s) * Mp + c0);
      } else {
#pragma unroll
        for (int s = 0; s < S1; ++s) {
          px[s].x = ws.pext[((size_t)bcl(0) * J * 3 + idx) * S1 + s];
          px[s].y = ws.pext[((size_t)bcl(1) * J * 3 + idx) * S1 + s];
          px[s].z = ws.pext[((size_t)bcl(2) * J * 3 + idx) * S1 + s];
          px[s].w = ws.pext[((size_t)bcl(3) * J * 3 + idx) * S1 + s];
        }
      }
      f4 tb0 = {0.f, 0.f, 0.f, 0.f}, acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < S; ++s) {
        tb0.x = __builtin_fmaf(tr[s].x, beta[s].x, tb0.x);
        tb0.y = __builtin_fmaf(tr[s].y, beta[s].y, tb0.y);
        tb0.z = __builtin_fmaf(tr[s].z, beta[s].z, tb0.z);
        tb0.w = __builtin_fmaf(tr[s].w, beta[s].w, tb0.w);
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        acc.x = __builtin_fmaf(px[1 + s].x, beta[s].x, acc.x);
        acc.y = __builtin_fmaf(px[1 + s].y, beta[s].y, acc.y);
        acc.z = __builtin_fmaf(px[1 + s].z, beta[s].z, acc.z);
        acc.w = __builtin_fmaf(px[1 + s].w, beta[s].w, acc.w);
      }
      const f4 jbv = t0 + tb0;
      const f4 rjv = px[0] + acc + LF4(bt, S + c);
      const float jbs[4] = {jbv.x, jbv.y, jbv.z, jbv.w}, rjs[4] = {rjv.x, rjv.y, rjv.z, rjv.w};
      if (c0 + 3 < B) *reinterpret_cast<f4*>(jbT + (size_t)(j * 4 + c) * 64) = jbv;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c0 + u < B) {
          if (c0 + 3 >= B) jbT[(size_t)(j * 4 + c) * 64 + u] = jbs[u];
          ws.jb[((size_t)(c0 + u) * J + j) * 4 + c] = jbs[u];
          ws.rjoints[(size_t)(c0 + u) * J * 3 + idx] = rjs[u];
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// fit_with_known_shape on the batch-major path: scale and translation between the target and the posed reference
// (fit_scale_and_translation, bodyfitter.py:1628-1681; what sf::scale_trans_stage does with a workgroup per instance).
//   k_align_partial_bm<PASS, W>  lane = instance, grid (Mp/64, chunks of the V sorted slots): PASS 1 the weighted sums
//                                [W, t (3), r (3)] of a chunk, PASS 2 (scale_fit) the centred second moments about the
//                                means of pass 1 (ws.vextra) — t the centred target (stream - mean), r the posed vertex
//                                the last LBS pass left in ws.vpT; rows [chunk][8][Mp] in ws.resP.
//   k_align_finish               one wave per instance: chunks in lane order + the joints (lane = joint), DPP sum;
//                                mode 1: the means to ws.vextra (scale_fit: pass 2 follows); mode 2: scale, translation
//                                and their substitution into the part sums / joints the refinement reads.
// ------------------------------------------------------------------------------------------------
template <int PASS, bool W>
__global__ __launch_bounds__(64) void k_align_partial_bm(DevModel m, Workspace ws, int B, int Mp, int nchunk) {
  const int lane = threadIdx.x, blk = blockIdx.x, ch = blockIdx.y, V = m.V, Vp = m.Vp;
  const int bcol = blk * 64 + lane, b = bcol < B ? bcol : B - 1;
  const int per = (V + nchunk - 1) / nchunk, v0 = ch * per, v1 = min(V, v0 + per);
  const float* tp = ws.tT + (size_t)blk * 3 * Vp * 64 + lane;
  const float* rp = ws.vpT + (size_t)blk * 3 * Vp * 64 + lane;
  const float* wp = W ? ws.wT + (size_t)blk * Vp * 64 + lane : nullptr;
  const size_t cstr = (size_t)Vp * 64;
  const float mu[3] = {ws.mean[(size_t)b * 3], ws.mean[(size_t)b * 3 + 1], ws.mean[(size_t)b * 3 + 2]};
  float mt[3] = {0.f, 0.f, 0.f}, mr[3] = {0.f, 0.f, 0.f};
  if (PASS == 2) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mt[c] = ws.vextra[(size_t)b * 32 + c];
      mr[c] = ws.vextra[(size_t)b * 32 + 3 + c];
    }
  }
  float a[7] = {0, 0, 0, 0, 0, 0, 0};
  constexpr int U = 4;
  for (int v = v0; v < v1; v += U) {
    float t[U][3], r[U][3], w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = v + u < v1;
      const int vv = in ? v + u : v0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        t[u][c] = ld_stream<1>(tp + (size_t)c * cstr + (size_t)vv * 64);
        r[u][c] = rp[(size_t)c * cstr + (size_t)vv * 64];
      }
      w[u] = W ? ld_stream<1>(wp + (size_t)vv * 64) : 1.f;
      if (!in) w[u] = 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (PASS == 1) {
        a[0] += w[u];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a[1 + c] += w[u] * (t[u][c] - mu[c]);
          a[4 + c] += w[u] * r[u][c];
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float dt = (t[u][c] - mu[c]) - mt[c], dr = r[u][c] - mr[c];
          a[0] += w[u] * dt * dt;
          a[1] += w[u] * dr * dr;
        }
      }
    }
  }
  float* out = ws.resP + (size_t)ch * 8 * Mp + bcol;
#pragma unroll
  for (int k = 0; k < (PASS == 1 ? 7 : 2); ++k) out[(size_t)k * Mp] = a[k];
}

struct AlignArgs {
  const float* tj;   // (B,J,3) centred target joints or null (vertices only)
  const float* jw;   // (B,J) or null
  int with_scale, regressed, mode, nchunk;
  float* scale_out;  // (B) or null
};
__global__ __launch_bounds__(64) void k_align_finish(DevModel m, AlignArgs a, Workspace ws, int B, int Mp) {
  const int b = blockIdx.x, lane = threadIdx.x, J = m.J;
  const float* part = ws.resP + b;
  float* rj = ws.rjoints + (size_t)b * J * 3;
  const float* tj = a.tj ? a.tj + (size_t)b * J * 3 : nullptr;
  const float* jw = a.jw ? a.jw + (size_t)b * J : nullptr;
  float* vx = ws.vextra + (size_t)b * 32;
  float sc = 1.0f, mt[3], mr[3];
  if (a.mode == 1) {  // means
    float s[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int ch = lane; ch < a.nchunk; ch += 64)
#pragma unroll
      for (int k = 0; k < 7; ++k) s[k] += part[((size_t)ch * 8 + k) * Mp];
    if (tj)
      for (int j = lane; j < J; j += 64) {
        const float w = jw ? jw[j] : 1.0f;
        s[0] += w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          s[1 + c] += w * tj[j * 3 + c];
          s[4 + c] += w * rj[j * 3 + c];
        }
      }
    float tot[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) tot[k] = __shfl(wave_sum_last(s[k]), 63, 64);
    const float invW = 1.0f / tot[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mt[c] = tot[1 + c] * invW;
      mr[c] = tot[4 + c] * invW;
    }
    if (a.with_scale) {  // pass 2 follows
      if (lane < 3) {
        vx[lane] = mt[lane];
        vx[3 + lane] = mr[lane];
      }
      return;
    }
  } else {  // scale from the centred second moments (:1665-1672)
    float q[2] = {0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mt[c] = vx[c];
      mr[c] = vx[3 + c];
    }
    for (int ch = lane; ch < a.nchunk; ch += 64) {
      q[0] += part[((size_t)ch * 8) * Mp];
      q[1] += part[((size_t)ch * 8 + 1) * Mp];
    }
    if (tj)
      for (int j = lane; j < J; j += 64) {
        const float w = jw ? jw[j] : 1.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float dt = tj[j * 3 + c] - mt[c], dr = rj[j * 3 + c] - mr[c];
          q[0] += w * dt * dt;
          q[1] += w * dr * dr;
        }
      }
    const float st = __shfl(wave_sum_last(q[0]), 63, 64), sr = __shfl(wave_sum_last(q[1]), 63, 64);
    sc = sqrtf(st / sr);
  }
  // the substitution reference <- scale * reference + trans on the part sums and joints (sf::scale_trans_stage)
  const float tr[3] = {mt[0] - sc * mr[0], mt[1] - sc * mr[1], mt[2] - sc * mr[2]};
  for (int j = lane; j < J; j += 64) {
    float* ps = ws.psum + ((size_t)b * J + j) * sf::kPsum;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) ps[r * 3 + c] = sc * ps[r * 3 + c] + ps[9 + r] * tr[c];
    for (int c = 0; c < 3; ++c) {
      ps[12 + c] = sc * ps[12 + c] + ps[15] * tr[c];
      rj[j * 3 + c] = sc * rj[j * 3 + c] + tr[c];
      if (a.regressed) {
        float* rr = ws.rjreg + (size_t)b * J * 3;
        rr[j * 3 + c] = sc * rr[j * 3 + c] + m.reg_rowsum[j] * tr[c];
      }
    }
  }
  if (lane < 3) ws.trans[(size_t)b * 3 + lane] = tr[lane];
  if (lane == 0) {
    ws.scale[b] = sc;
    if (a.scale_out) a.scale_out[b] = sc;
  }
}

// The two combine kernels for the FINE cell tables (small batches, sf_tables.h): eight times the rows and a handful
// of instance blocks, so the rows of an output are split over the G waves of a workgroup — wave g adds the g-th of G
// contiguous runs of them (eight loads in flight, a fixed tree), the runs are added in order through LDS.
// lane = instance; grid (Mp/64, outputs), block 64 G.
template <int G, class RowFn>
__device__ __forceinline__ float sum_rows_split(const float* __restrict__ buf, int n, int g, size_t col, int Mp, RowFn row) {
  const int i0 = (int)((long)n * g / G), i1 = (int)((long)n * (g + 1) / G);
  float acc = 0.f;
  int i = i0;
  for (; i + 8 <= i1; i += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = buf[row(i + u) * Mp + col];
    acc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  }
  for (; i < i1; ++i) acc += buf[row(i) * Mp + col];
  return acc;
}

// ------------------------------------------------------------------------------------------------
// Vertex weights on the batch-major path (fit(vertex_weights=...), reference bodyfitter.py:1018-1040, _part_sums
// :257-280).
//   k_layout_weights   the (B, V) weights to the instance-innermost stream ws.wT [instance block][Vp][64] at the sorted
//                      slots; the padding slots get weight 0 (an out-of-range step contributes exactly 0).
//                      grid (ceil(V/64) + 1, Mp/64), block 256; the last block of a column zeroes the padding slots.
//   k_accum_w_bm       the weighted vertex block of the normal equations, lane = instance (what k_shape_accum does with
//                      a wave per instance):  per vertex  Jac = Rt S_v + sum_k s_vk T'_k  (3 x S),  b = t - (Rt x + T0),
//                      G += w Jac^T Jac,  r += w Jac^T b,  SA += w Jac,  Sb += w b,  W += w.
//                      One wave per workgroup (the waves share nothing).  The four joints of the current piece live in
//                      registers (PieceJoints) and their T' rows (4 x 3 x jd_row floats per lane) in LDS as float4
//                      columns [joint][c][quad][lane]: a lane reads its own 16 bytes, conflict-free.  Per vertex and
//                      coordinate c the Jacobian row a_c (S values, S/2 register pairs) is formed from the vertex record
//                      (scalar registers) and the T' rows, then the Gramian rows are updated as packed pairs kept from
//                      an even column (30 pairs for S = 10).  ~330 VALU + 30 ds_read_b128 per vertex.  The accumulators
//                      (G 60, r 10, SA 30, Sb 3, W 1) restart at every cell; a cell's record goes to ws.accP
//                      [cell][NE + 1][Mp] in the layout of the solve stage's record, so k_accum_combine is a sum over
//                      cells in table order.  grid (Mp/64, ncells / mult), block 64, dynamic LDS accum_w_lds<S>() = 37 KB.
// ------------------------------------------------------------------------------------------------
// VW_SHARED: vw is ONE (V) row every instance of the batch reads (smplfit_replace_hands_f32), not (B, V)
template <bool VW_SHARED = false>
__global__ __launch_bounds__(256) void k_layout_weights(DevModel m, const float* __restrict__ vw, float* __restrict__ wT,
                                                        int B) {
  __shared__ float tile[64][65];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.y, V = m.V, Vp = m.Vp;
  float* dst = wT + (size_t)blk * Vp * 64 + lane;
  if ((int)blockIdx.x * 64 >= V) {  // the padding slots
    for (int slot = V + wave; slot < Vp; slot += 4) dst[(size_t)slot * 64] = 0.f;
    return;
  }
  const int v0 = blockIdx.x * 64;
  float x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int inst = wave + 4 * i;
    x[i] = (v0 + lane < V && blk * 64 + inst < B) ? (VW_SHARED ? vw[v0 + lane] : ld_stream<4>(vw + (size_t)(blk * 64 + inst) * V + v0 + lane)) : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[wave + 4 * i][lane] = x[i];
  __syncthreads();
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int vl = wave + 4 * i;
    if (v0 + vl >= V) break;
    st_stream<8>(dst + (size_t)m.inv_slot[v0 + vl] * 64, tile[lane][vl]);
  }
}

typedef float f4 __attribute__((ext_vector_type(4)));
template <int S>
struct GramPairs {  // row i of the upper triangle as register pairs from the even column (i & ~1): compile-time indices
  static constexpr int SP = S / 2;
  static constexpr int base(int i) {
    int b = 0;
    for (int r = 0; r < i; ++r) b += SP - (r >> 1);
    return b;
  }
  static constexpr int count = base(S);
};

template <int S>
constexpr size_t accum_w_lds() { return (size_t)4 * 3 * (sf::jd_row(S) / 4) * 64 * 16; }
#ifndef SMPLFIT_ACC_WAVES
#define SMPLFIT_ACC_WAVES 2
#endif
constexpr int kAccWaves = SMPLFIT_ACC_WAVES;  // waves of a k_accum_w_bm workgroup (1 or 2)

// NW = 2: the two waves of a workgroup share the T' rows of the current piece (the same 64 instances) and take its
// vertices alternately — the LDS that limits a CU to four workgroups then feeds EIGHT waves, two per SIMD, which cover
// each other's waits (a lonely wave issues a packed instruction every 5.2 cycles, two waves one every 4.6 each and
// overlapped: tools/ubench/valu_rate).  Each wave keeps its own accumulators; at the end of a cell wave 1 hands its sums
// to wave 0 through the T' area.  Two barriers per piece (fill / release of the T' rows).
// W = false: unit weights (no weight stream).  EXTRAS: also the sums of the scaled shape solve (fit(scale_target /
// scale_fit), sf::scale_extras_vertex: u = sum w Jac^T t, sum w |t|^2, sum w t.b, sum w |b|^2, sum w t) behind the
// record — the last iteration of such a fit runs this kernel (with one wave per workgroup: sixteen more accumulators)
// whatever its weights.
constexpr int kAccExtras = 16;  // S + 6 <= 16 floats behind a cell's record
template <int S, int NW, bool W = true, bool EXTRAS = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW, NW))) void k_accum_w_bm(DevModel m, ShareView sv,
                                                                                                    Workspace ws, int B, int Mp) {
  static_assert(!EXTRAS || NW == 1, "the extra sums are not handed over between waves");
  static_assert(S + 6 <= kAccExtras, "extras record");
  static_assert(S % 2 == 0 && S <= 12, "weighted batch-major accumulate: an even number of unknowns (10)");
  static_assert(NW == 1 || NW == 2, "one or two waves per workgroup");
  static_assert(4 * accum_w_lds<S>() <= 160 * 1024, "four workgroups per CU");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int STRIDE = sf::jd_stride(S), ROW = sf::jd_row(S), RQ = ROW / 4, SP = S / 2;
  constexpr int NG = sf::ne_ng(S), NE = sf::ne_size(S);
  using GP = GramPairs<S>;
  constexpr int NACC = 2 * GP::count + 2 * SP + 6 * SP + 4;  // floats a wave hands over at the end of a cell
  static_assert((size_t)NACC * 64 * 4 <= accum_w_lds<S>(), "the hand-over fits the T' area");
  const int lane = threadIdx.x & 63;
  const int wave = NW == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int share = blockIdx.y, blk = blockIdx.x, J = m.J, Vp = m.Vp;
  const int bcol = blk * 64 + lane;
  const int b = bcol < B ? bcol : B - 1;
  const int Np = (J * STRIDE + 63) / 64 * 64;
  const float* jdb = ws.jdT + (size_t)blk * Np * 64 + lane;
  f4* T4 = reinterpret_cast<f4*>(smem) + lane;  // T' rows: [(k * 3 + c) * RQ + q] * 64
  const float mu0 = ws.mean[(size_t)b * 3], mu1 = ws.mean[(size_t)b * 3 + 1], mu2v = ws.mean[(size_t)b * 3 + 2];
  PieceJoints jr;
  auto load_joints = [&](const_i32_ptr rec) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* row = jdb + (size_t)rec[1 + k] * STRIDE * 64;
      float r[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) r[i] = row[i * 64];
      jr.p[k][0] = mk2(r[0], r[3]);
      jr.p[k][1] = mk2(r[1], r[4]);
      jr.p[k][2] = mk2(r[2], r[5]);
      jr.p[k][3] = mk2(r[6], r[7]);
      jr.p[k][4] = mk2(r[8], r[11]);
      jr.p[k][5] = mk2(r[9], r[10]);
      // T' rows of the joint: 3 x ROW floats (the row padding is zero, sf::joint_stage); with two waves, wave w fills
      // the joints 2 w, 2 w + 1
      if (NW == 2 && (k >> 1) != wave) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        f4 t[RQ];
#pragma unroll
        for (int q = 0; q < RQ; ++q) {
          const float* tr = row + (size_t)(12 + c * ROW + 4 * q) * 64;
          t[q].x = tr[0]; t[q].y = tr[64]; t[q].z = tr[128]; t[q].w = tr[192];
        }
#pragma unroll
        for (int q = 0; q < RQ; ++q) T4[((k * 3 + c) * RQ + q) * 64] = t[q];
      }
    }
  };
  f2 G[GP::count], r1p[SP], SA[3][SP], up[SP];
  float sb[3] = {0.f, 0.f, 0.f}, wsum = 0.f, xq[3] = {0.f, 0.f, 0.f}, xt[3] = {0.f, 0.f, 0.f};
  auto zero_acc = [&]() {
#pragma unroll
    for (int k = 0; k < GP::count; ++k) G[k] = mk2(0, 0);
#pragma unroll
    for (int k = 0; k < SP; ++k) {
      r1p[k] = mk2(0, 0);
      SA[0][k] = mk2(0, 0); SA[1][k] = mk2(0, 0); SA[2][k] = mk2(0, 0);
      up[k] = mk2(0, 0);
    }
    sb[0] = 0.f; sb[1] = 0.f; sb[2] = 0.f;
    wsum = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { xq[c] = 0.f; xt[c] = 0.f; }
  };
  zero_acc();
  const float* vp = ws.vpT + (size_t)blk * 3 * Vp * 64;
  const float* tp = ws.tT + (size_t)blk * 3 * Vp * 64;
  const float* wp = W ? ws.wT + (size_t)blk * Vp * 64 : nullptr;
  const uint32_t ul = (uint32_t)lane;
  const size_t cstr = (size_t)Vp * 64;
  const int ps = sv.piece_start[share * sv.mult], np = sv.piece_start[(share + 1) * sv.mult] - ps;
  if (np <= 0) return;
  const int vpad = m.V;
  const_i32_ptr pc = as_constant(sv.pieces + (size_t)ps * kPieceRec);
  int vb = pc[9], len = pc[0];
  // the wave's vertices of a piece: indices wave, wave + NW, ...; a piece is walked in an even number of steps per wave
  auto vert = [&](int q, int vbase, int plen) {  // the q-th vertex of this wave in a piece (or the padding slot)
    const int idx = q * NW + wave;
    return idx < plen ? vbase + idx : vpad;
  };
  VertexRec<S> recA, recB;
  load_rec<S>(m.brec, vert(0, vb, len), recA);
  struct WBuf { StreamBuf s; float w; };
  auto request = [&](int v, WBuf& sb2) {
    const float* q = vp + (size_t)v * 64;
    const float* r = tp + (size_t)v * 64;
    sb2.s.x01.x = ld_stream<1>(q + ul); sb2.s.x01.y = ld_stream<1>(q + cstr + ul); sb2.s.xt2.x = ld_stream<1>(q + 2 * cstr + ul);
    sb2.s.t01.x = ld_stream<1>(r + ul); sb2.s.t01.y = ld_stream<1>(r + cstr + ul); sb2.s.xt2.y = ld_stream<1>(r + 2 * cstr + ul);
    // (unit weights: the padding slot must still count for nothing — its record is all zero, so its Jacobian and its
    // residual are; only W and the target sums of the extras see it, and those take the weight from here)
    if constexpr (W) sb2.w = ld_stream<1>(wp + (size_t)v * 64 + ul);
    else sb2.w = v == vpad ? 0.f : 1.f;
  };
  WBuf rA, rB;
  request(vert(0, vb, len), rA);
  request(vert(1, vb, len), rB);
  // One step.  The T' rows come from LDS two joints at a time (24 registers): the rows of the next pair / the next
  // coordinate are requested as soon as the buffer is consumed — under the Jacobian row's shapedirs part and under the
  // Gramian update — and the NEXT vertex's record (scalar loads share their counter with LDS reads: a wait for either is
  // a wait for both) behind the last LDS wait of the step.  Scheduling barriers pin these issue points.  (Measured with
  // one wave per workgroup and not kept: the streams AND the records through an LDS ring filled by LDS-DMA four vertices
  // ahead — 576 / 715 us against 566: the lonely wave is bound by its issue rate, not by the latency of its requests.)
  f4 t[2][RQ];
  auto read_t = [&](int c, int h) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int q = 0; q < RQ; ++q) t[k][q] = T4[(((2 * h + k) * 3 + c) * RQ + q) * 64];
  };
  auto step = [&](int vn1, int vn2, WBuf& wb, const VertexRec<S>& rc, VertexRec<S>& rn) {
    asm volatile("" ::"s"(rc.w[0]));  // this vertex's record is here (the only scalar request outstanding)
    __builtin_amdgcn_sched_barrier(0);
    read_t(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    const float (&cw)[4] = rc.w;
    const float (&rec)[3 * S] = rc.sd;
    StreamBuf& buf = wb.s;
    f2 Q[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) Q[i] = mk2(0, 0);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int i = 0; i < 6; ++i) Q[i] += cw[k] * jr.p[k][i];
    const f2 zz = buf.xt2 - mk2(0.f, mu2v);  // (x2, t2 - mean2)
    const f2 pos01 = (Q[0] * buf.x01.x + Q[1] * buf.x01.y) + (Q[2] * zz.x + Q[5]);
    const float pos2 = (Q[3].x * buf.x01.x + Q[3].y * buf.x01.y) + (Q[4].x * zz.x + Q[4].y);
    const f2 b01 = (buf.t01 - mk2(mu0, mu1)) - pos01;
    const float b2 = zz.y - pos2;
    // the vertex weight is needed to the end of the step: copied out of its buffer HERE, by hand (left to the compiler
    // the copy sinks to the loop's back edge together with a wait for every outstanding load), then the buffer is
    // refilled with the wave's vertex two steps ahead
    float wv;
    asm volatile("v_mov_b32 %0, %1" : "=v"(wv) : "v"(wb.w));
    const f2 tc01 = buf.t01 - mk2(mu0, mu1);  // (EXTRAS: the centred target)
    const float tc2 = zz.y;
    request(vn2, wb);
    sb[0] += wv * b01.x; sb[1] += wv * b01.y; sb[2] += wv * b2;
    wsum += wv;
    if constexpr (EXTRAS) {
      xq[0] += wv * ((tc01.x * tc01.x + tc01.y * tc01.y) + tc2 * tc2);
      xq[1] += wv * ((tc01.x * b01.x + tc01.y * b01.y) + tc2 * b2);
      xq[2] += wv * ((b01.x * b01.x + b01.y * b01.y) + b2 * b2);
      xt[0] += wv * tc01.x; xt[1] += wv * tc01.y; xt[2] += wv * tc2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float rc0 = c == 0 ? Q[0].x : c == 1 ? Q[0].y : Q[3].x;
      const float rc1 = c == 0 ? Q[1].x : c == 1 ? Q[1].y : Q[3].y;
      const float rc2 = c == 0 ? Q[2].x : c == 1 ? Q[2].y : Q[4].x;
      const float bc = c == 0 ? b01.x : c == 1 ? b01.y : b2;
      // Jacobian row: the blended T' rows of joints 0, 1 | Rt_c . shapedirs | the T' rows of joints 2, 3
      f2 ap[SP];
#pragma unroll
      for (int jp = 0; jp < SP; ++jp) {
        const f4 t0 = t[0][jp >> 1], t1 = t[1][jp >> 1];
        ap[jp] = cw[0] * ((jp & 1) ? mk2(t0.z, t0.w) : mk2(t0.x, t0.y)) + cw[1] * ((jp & 1) ? mk2(t1.z, t1.w) : mk2(t1.x, t1.y));
      }
      __builtin_amdgcn_sched_barrier(0);
      read_t(c, 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int jp = 0; jp < SP; ++jp)
        ap[jp] += (mk2(rec[2 * jp], rec[2 * jp + 1]) * rc0 + mk2(rec[S + 2 * jp], rec[S + 2 * jp + 1]) * rc1) +
                  mk2(rec[2 * S + 2 * jp], rec[2 * S + 2 * jp + 1]) * rc2;
#pragma unroll
      for (int jp = 0; jp < SP; ++jp) {
        const f4 t0 = t[0][jp >> 1], t1 = t[1][jp >> 1];
        ap[jp] += cw[2] * ((jp & 1) ? mk2(t0.z, t0.w) : mk2(t0.x, t0.y)) + cw[3] * ((jp & 1) ? mk2(t1.z, t1.w) : mk2(t1.x, t1.y));
      }
      __builtin_amdgcn_sched_barrier(0);
      if (c < 2) read_t(c + 1, 0);
      else load_rec<S>(m.brec, vn1, rn);
      __builtin_amdgcn_sched_barrier(0);
      f2 wap[SP];
#pragma unroll
      for (int jp = 0; jp < SP; ++jp) wap[jp] = ap[jp] * wv;
#pragma unroll
      for (int i = 0; i < S; ++i) {
        const float wa = (i & 1) ? wap[i >> 1].y : wap[i >> 1].x;
#pragma unroll
        for (int jp = i >> 1; jp < SP; ++jp) G[GP::base(i) + jp - (i >> 1)] += wa * ap[jp];
      }
#pragma unroll
      for (int jp = 0; jp < SP; ++jp) {
        r1p[jp] += wap[jp] * bc;
        SA[c][jp] += wap[jp];
        if constexpr (EXTRAS) up[jp] += wap[jp] * (c == 0 ? tc01.x : c == 1 ? tc01.y : tc2);
      }
    }
  };
  for (int p = 0; p < np; ++p) {
    const bool more = p + 1 < np;
    const int len_next = more ? pc[kPieceRec] : 0, vn = more ? pc[kPieceRec + 9] : vpad;
    load_joints(pc);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int i = 0; i < 6; ++i) asm volatile("" : "+v"(jr.p[k][i].x), "+v"(jr.p[k][i].y));
    if (NW == 2) __syncthreads();  // the T' rows of the piece are complete
    // steps of this wave in the piece: its share of the vertices, rounded up to an even number (the two stream buffers
    // keep their roles); step q continues into the wave's first vertices of the next piece
    const int nq = (((len + NW - 1) / NW) + 1) & ~1;
    auto at = [&](int q) { return q < nq ? vert(q, vb, len) : vert(q - nq, vn, len_next); };
    for (int q = 0; q < nq; q += 2) {
      step(at(q + 1), at(q + 2), rA, recA, recB);
      step(at(q + 2), at(q + 3), rB, recB, recA);
    }
    if (NW == 2) __syncthreads();  // both waves are done with the T' rows
    const int cell = pc[10] >= 0 ? (pc[11] >> 8) - 1 : -1;
    if (cell >= 0) {  // end of a cell: its record leaves, the sums restart (the rows do not depend on the multiplier)
      if (NW == 2) {  // wave 1 hands its sums to wave 0 (through the T' area: lane-private columns)
        float* hx = smem + lane;
        if (wave == 1) {
          int o = 0;
#pragma unroll
          for (int k = 0; k < GP::count; ++k) { hx[(o++) * 64] = G[k].x; hx[(o++) * 64] = G[k].y; }
#pragma unroll
          for (int k = 0; k < SP; ++k) { hx[(o++) * 64] = r1p[k].x; hx[(o++) * 64] = r1p[k].y; }
#pragma unroll
          for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < SP; ++k) { hx[(o++) * 64] = SA[c][k].x; hx[(o++) * 64] = SA[c][k].y; }
          hx[(o++) * 64] = sb[0]; hx[(o++) * 64] = sb[1]; hx[(o++) * 64] = sb[2]; hx[(o++) * 64] = wsum;
        }
        __syncthreads();
        if (wave == 0) {
          int o = 0;
#pragma unroll
          for (int k = 0; k < GP::count; ++k) { G[k].x += hx[(o++) * 64]; G[k].y += hx[(o++) * 64]; }
#pragma unroll
          for (int k = 0; k < SP; ++k) { r1p[k].x += hx[(o++) * 64]; r1p[k].y += hx[(o++) * 64]; }
#pragma unroll
          for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < SP; ++k) { SA[c][k].x += hx[(o++) * 64]; SA[c][k].y += hx[(o++) * 64]; }
          sb[0] += hx[(o++) * 64]; sb[1] += hx[(o++) * 64]; sb[2] += hx[(o++) * 64]; wsum += hx[(o++) * 64];
        }
        __syncthreads();  // (the hand-over area is the next piece's T' rows)
      }
      if (wave == 0) {
        float* oc = ws.accP + (size_t)cell * (NE + 1 + kAccExtras) * Mp + bcol;
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
          for (int j = i; j < S; ++j) {
            const f2 g = G[GP::base(i) + (j >> 1) - (i >> 1)];
            oc[(size_t)sf::ne_g(S, i, j) * Mp] = (j & 1) ? g.y : g.x;
          }
#pragma unroll
        for (int i = 0; i < S; ++i) {
          oc[(size_t)(NG + i) * Mp] = (i & 1) ? r1p[i >> 1].y : r1p[i >> 1].x;
#pragma unroll
          for (int c = 0; c < 3; ++c) oc[(size_t)(NG + S + c * S + i) * Mp] = (i & 1) ? SA[c][i >> 1].y : SA[c][i >> 1].x;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) oc[(size_t)(NG + 4 * S + c) * Mp] = sb[c];
        oc[(size_t)NE * Mp] = wsum;
        if constexpr (EXTRAS) {
          float* ox = oc + (size_t)(NE + 1) * Mp;
#pragma unroll
          for (int i = 0; i < S; ++i) ox[(size_t)i * Mp] = (i & 1) ? up[i >> 1].y : up[i >> 1].x;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            ox[(size_t)(S + c) * Mp] = xq[c];
            ox[(size_t)(S + 3 + c) * Mp] = xt[c];
          }
        }
      }
      zero_acc();
    }
    vb = vn;
    len = len_next;
    pc += kPieceRec;
  }
}

// cell records of k_accum_w_bm -> the solve stage's record ws.gramv (fp64), cells added in table order
// (sum_rows_split: the rows of an entry over the G waves of a workgroup).  grid (Mp/64, NE + 1 [+ S + 6]), block 64 G.
// unit (the unit-weight form of the kernel, scale fits): SA = 0 and W = V as k_shape_accum leaves them — the joint
// stage evaluates the unit-weight SA in closed form.  Entries behind the record: the extras of the scaled solve, to
// ws.vextra.
template <int S, int G>
__global__ __launch_bounds__(64 * G) void k_accum_combine(DevModel m, ShareView sv, Workspace ws, int B, int Mp, int unit) {
  constexpr int NE = sf::ne_size(S), NG = sf::ne_ng(S), REC = NE + 1 + kAccExtras;
  __shared__ float part[G][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, b = blockIdx.x * 64 + lane, e = blockIdx.y;
  float acc = sum_rows_split<G>(ws.accP, sv.ncells, g, b, Mp, [&](int i) { return (size_t)e + (size_t)i * REC; });
  part[g][lane] = acc;
  __syncthreads();
  if (g != 0 || b >= B) return;
  acc = part[0][lane];
#pragma unroll
  for (int q = 1; q < G; ++q) acc += part[q][lane];
  if (e > NE) {
    ws.vextra[(size_t)b * 32 + (e - NE - 1)] = acc;
    return;
  }
  double v = (double)acc;
  if (unit && e >= NG + S && e < NG + 4 * S) v = 0.0;
  if (unit && e == NE) v = (double)m.V;
  ws.gramv[(size_t)b * (NE + 1) + e] = v;
}

template <int S, int G>
__global__ __launch_bounds__(64 * G) void k_gram_combine_split(DevModel m, ShareView sv, Workspace ws, int B, int Mp) {
  constexpr int kResShareRec = res_share_rec(S);
  constexpr int NG = sf::ne_ng(S), NE = sf::ne_size(S);
  __shared__ float part[G][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, b = blockIdx.x * 64 + lane, e = blockIdx.y, J = m.J;
  float acc;
  int k = 0, j = 0, c = 0;
  if (e < S + 3) {
    acc = sum_rows_split<G>(ws.resP, sv.ncells, g, b, Mp, [&](int i) { return (size_t)e + (size_t)i * kResShareRec; });
  } else if (e < S + 3 + 3 * J) {
    j = (e - S - 3) / 3, c = (e - S - 3) % 3;
    const int a0 = sv.aux_start[j];
    acc = sum_rows_split<G>(ws.resP, sv.aux_start[j + 1] - a0, g, b, Mp, [&](int i) { return (size_t)sv.aux_rows[a0 + i] + c; });
  } else {
    k = e - (S + 3 + 3 * J);
    const int nwg = pair_gram_workgroups(J, m.jt.np);
    acc = sum_rows_split<G>(ws.gramP, nwg, g, b, Mp, [&](int i) { return (size_t)k + (size_t)i * NG; });
  }
  part[g][lane] = acc;
  __syncthreads();
  if (g != 0 || b >= B) return;
  acc = part[0][lane];
#pragma unroll
  for (int q = 1; q < G; ++q) acc += part[q][lane];
  double* out = ws.gramv + (size_t)b * (NE + 1);
  if (e < S + 3) {
    out[e < S ? NG + e : NG + 4 * S + (e - S)] = (double)acc;
    if (e == 0) {
      for (int q = 0; q < 3 * S; ++q) out[NG + S + q] = 0.0;
      out[NE] = (double)m.V;
    }
  } else if (e < S + 3 + 3 * J) {
    ws.mbj[((size_t)b * J + j) * 3 + c] = acc;
  } else {
    int i = 0, r = k;
    while (r >= S - i) {
      r -= S - i;
      ++i;
    }
    out[k] = (double)(m.jt.diag_g0[i * S + i + r] + acc);
  }
}

template <int G>
__global__ __launch_bounds__(64 * G) void k_psum_combine_split(DevModel m, ShareView sv, Workspace ws, int B, int Mp) {
  static_assert(sf::kPsum % G == 0, "a wave finishes kPsum / G entries");
  __shared__ float part[G][sf::kPsum][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, b = blockIdx.x * 64 + lane, prt = blockIdx.y;
  const int a0 = sv.aux_start[prt], n = sv.aux_start[prt + 1] - a0;
  const int i0 = (int)((long)n * g / G), i1 = (int)((long)n * (g + 1) / G);
  float acc[sf::kPsum];
#pragma unroll
  for (int k = 0; k < sf::kPsum; ++k) acc[k] = 0.f;
  for (int i = i0; i < i1; ++i) {
    const float* src = ws.psumP + (size_t)sv.aux_rows[a0 + i] * sf::kPsum * Mp + b;
#pragma unroll
    for (int k = 0; k < sf::kPsum; ++k) acc[k] += src[(size_t)k * Mp];
  }
#pragma unroll
  for (int k = 0; k < sf::kPsum; ++k) part[g][k][lane] = acc[k];
  __syncthreads();
  if (b >= B) return;
#pragma unroll
  for (int kk = 0; kk < sf::kPsum / G; ++kk) {
    const int k = g * (sf::kPsum / G) + kk;
    float t = part[0][k][lane];
#pragma unroll
    for (int q = 1; q < G; ++q) t += part[q][k][lane];
    ws.psum[((size_t)b * m.J + prt) * sf::kPsum + k] = t;
  }
}

// part-sum rows of the shares -> ws.psum[b][part][16] (the rows of one part summed in table order).
// grid (ceil(B/256), J): blockIdx.y = part.
__global__ __launch_bounds__(256) void k_psum_combine(DevModel m, ShareView sv, Workspace ws, int B, int Mp) {
  const int b = blockIdx.x * 256 + threadIdx.x, part = blockIdx.y;
  if (b >= B) return;
  float acc[sf::kPsum];
#pragma unroll
  for (int k = 0; k < sf::kPsum; ++k) acc[k] = 0.f;
  // a part without a row (an unused part; a used part that owns no vertex of a subset; every part but the
  // adjustable ones behind the last pass of a fit) gets zeros: the joint stages read every row
  for (int q = sv.aux_start[part]; q < sv.aux_start[part + 1]; ++q) {
    const float* src = ws.psumP + (size_t)sv.aux_rows[q] * sf::kPsum * Mp + b;
#pragma unroll
    for (int k = 0; k < sf::kPsum; ++k) acc[k] += src[(size_t)k * Mp];
  }
  float4* dst = reinterpret_cast<float4*>(ws.psum + ((size_t)b * m.J + part) * sf::kPsum);
  dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
  dst[2] = make_float4(acc[8], acc[9], acc[10], acc[11]);
  dst[3] = make_float4(acc[12], acc[13], acc[14], acc[15]);
}


// ------------------------------------------------------------------------------------------------
// Topology transfer (BodyConverter.convert_vertices, reference pt/bodyconverter.py:128-149; the matrix is the first
// half of the columns of the official *_deftrafo_setup.pkl files, common.py:425-429): every output vertex is a
// weighted combination of a few (usually 3) input vertices.
//
// k_transfer_bm — the fused form used by smplfit_convert_f32: the input model's posed vertices are read from ITS
// instance-innermost stream (srcT = the input handle's vpT after the forward-only LBS pass, sorted slots of the input
// model) and the result is written straight into the OUTPUT model's target stream tT at the output model's sorted
// slots, together with the per-slab coordinate sums k_mean_finish reads — k_layout_targets and every
// instance-major intermediate disappear from `convert`.  lane = instance: a row of the matrix is wave-uniform
// (scalar loads), every gathered value is one coalesced 256-byte row.  Entries are added in table (CSR) order.
// grid (ceil(V_out / kSlabV), Mp/64), block 256: a workgroup takes kSlabV consecutive ORIGINAL output vertices,
// wave w the vertices w, w + 4, ...; `part` (slab, 3, Mp) as in k_layout_targets.
// NEG (a SMPLFIT_TRANSFER_NEGATE_X matrix, the mirror of smplfit_flip_f32): x -> -x after the row sum, in the stream
// AND in the slab sums, so that k_mean_finish takes the mean of the flipped mesh.  Negation is exact: the values equal
// those of k_transfer_rows<_, true>.
// ------------------------------------------------------------------------------------------------
struct TransferTabs {
  const int32_t* oslot;   // (V_out) sorted slot of the output vertex in the output model
  const int32_t* start;   // (V_out + 1) entry range of the output vertex
  const int32_t* islot;   // (nnz) sorted slot of the entry's input vertex in the input model
  const float* w;         // (nnz)
  int v_out;
};

template <bool NEG>
__global__ __launch_bounds__(256) void k_transfer_bm(TransferTabs tt, const float* __restrict__ srcT, int VpIn,
                                                     float* __restrict__ tT, int VpOut, float* __restrict__ part, int Mp) {
  __shared__ float red[4 * 3 * 64];
  const int slab = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* s = srcT + (size_t)blk * 3 * VpIn * 64 + lane;
  float* d = tT + (size_t)blk * 3 * VpOut * 64 + lane;
  const size_t cin = (size_t)VpIn * 64, cout = (size_t)VpOut * 64;
  const int v0 = slab * kSlabV;
  // the matrix through the constant address space: wave-uniform rows -> scalar loads
  const const_i32_ptr t_start = as_constant(tt.start), t_oslot = as_constant(tt.oslot), t_islot = as_constant(tt.islot);
  const const_f32_ptr t_w = as_constant(tt.w);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  constexpr int U = 4;  // entries requested together (a barycentric row has three)
  for (int k = 0; k < kSlabV / 4; ++k) {
    const int r = v0 + wave + 4 * k;  // wave-uniform
    if (r >= tt.v_out) break;
    const int e0 = t_start[r], e1 = t_start[r + 1], oslot = t_oslot[r];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int e = e0; e < e1; e += U) {
      float x[U][3], w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ee = e + u < e1 ? e + u : e1 - 1;
        const int slot = t_islot[ee];
        w[u] = e + u < e1 ? t_w[ee] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) x[u][c] = s[(size_t)c * cin + (size_t)slot * 64];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a0 += w[u] * x[u][0];
        a1 += w[u] * x[u][1];
        a2 += w[u] * x[u][2];
      }
    }
    if constexpr (NEG) a0 = -a0;
    st_stream<8>(d + (size_t)oslot * 64, a0);
    st_stream<8>(d + cout + (size_t)oslot * 64, a1);
    st_stream<8>(d + 2 * cout + (size_t)oslot * 64, a2);
    s0 += a0; s1 += a1; s2 += a2;
  }
  red[(wave * 3 + 0) * 64 + lane] = s0;
  red[(wave * 3 + 1) * 64 + lane] = s1;
  red[(wave * 3 + 2) * 64 + lane] = s2;
  __syncthreads();
  if (tid < 192) {
    const int c = tid >> 6;
    const float sum = (red[c * 64 + lane] + red[(3 + c) * 64 + lane]) + (red[(6 + c) * 64 + lane] + red[(9 + c) * 64 + lane]);
    part[((size_t)slab * 3 + c) * Mp + blk * 64 + lane] = sum;
  }
}

// k_transfer_rows — the stand-alone form behind smplfit_transfer_f32 (instance-major in and out, what
// convert_vertices returns to a caller): one workgroup per instance stages the instance's (V_in, 3) row in LDS with
// coalesced loads (gathering 12-byte vertices from global memory pulls ~8x the row through the fabric, see K0), then
// every thread forms output vertices from LDS and the rows go out as contiguous 12-byte pieces.
// grid B, block 1024, dynamic LDS 12 V_in bytes; STAGED = false (V_in beyond the LDS): gathers from global memory.
// NEG: x -> -x after the row sum (SMPLFIT_TRANSFER_NEGATE_X).
// smplfit_transfer_backward_f32 runs the same kernel on the CSR form of the transposed matrix (sf::transpose_csr) with
// Vin and Vout swapped: `in` is then the cotangent (B, V_out, 3), a "row" an input vertex, whose entries are added in
// ascending output-row order; a vertex without entries stores its zero accumulators.
template <bool STAGED, bool NEG>
__global__ __launch_bounds__(1024) void k_transfer_rows(const float* __restrict__ in, float* __restrict__ out,
                                                        const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                        const float* __restrict__ values, int Vin, int Vout) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* src = in + (size_t)b * Vin * 3;
  if constexpr (STAGED) {
    const int n = 3 * Vin;
    constexpr int UB = 8;  // requests of a thread in flight before its LDS stores
    for (int i0 = tid; i0 < n; i0 += 1024 * UB) {
      float x[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) x[u] = i0 + 1024 * u < n ? src[i0 + 1024 * u] : 0.f;
#pragma unroll
      for (int u = 0; u < UB; ++u)
        if (i0 + 1024 * u < n) smem[i0 + 1024 * u] = x[u];
    }
    __syncthreads();
  }
  const float* s = STAGED ? smem : src;
  float* dst = out + (size_t)b * Vout * 3;
  for (int r = tid; r < Vout; r += 1024) {
    const int e0 = indptr[r], e1 = indptr[r + 1];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int e = e0; e < e1; ++e) {  // CSR order, as the reference's sparse product adds them
      const int c = indices[e];
      const float w = values[e];
      a0 += w * s[3 * c];
      a1 += w * s[3 * c + 1];
      a2 += w * s[3 * c + 2];
    }
    dst[3 * r] = NEG ? -a0 : a0;
    dst[3 * r + 1] = a1;
    dst[3 * r + 2] = a2;
  }
}

// ------------------------------------------------------------------------------------------------
// k_naive_flip — BodyFlipper.naive_flip_rotvecs (reference pt/bodyflipper.py:121-133): the joints reordered by the
// joint mirror map and every rotation vector multiplied by (1, -1, -1); the warm start of smplfit_flip_f32.  Exact
// (a permutation and sign changes).  lane = instance: grid ceil(B / 256), block 256; perm (J) lies in [0, J) (checked
// when the plan is made).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_naive_flip(const float* __restrict__ pose, const int32_t* __restrict__ perm,
                                                    float* __restrict__ out, int B, int J) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* src = pose + (size_t)b * J * 3;
  float* dst = out + (size_t)b * J * 3;
  for (int j = 0; j < J; ++j) {
    const int k = perm[j];
    dst[3 * j] = src[3 * k];
    dst[3 * j + 1] = -src[3 * k + 1];
    dst[3 * j + 2] = -src[3 * k + 2];
  }
}

// ------------------------------------------------------------------------------------------------
// smplfit_replace_hands_f32 (HandReplacer.replace_hand, reference pt/handreplacer.py:48-74).
//   k_rotvecs_to_mats     once per plan: the n replacement rotation vectors as rotation matrices, by the arithmetic the
//                         forward's joint stage runs on rotation vectors (sf::rotvec2mat on the device).
//   k_replace_rotations   the fitted relative rotations of the joints [j0, j0 + n) of every instance overwritten with those
//                         matrices — the form the forward's joint stage consumes (ForwardArgs::rel), so the edited pose
//                         never goes through (B, 3J) rotation vectors — and, when pose is given, the same joints of the
//                         fit's rotation vectors with the replacement vectors.  One element per thread, consecutive
//                         threads write consecutive floats of an instance's run (9 n / 3 n floats).  grid
//                         ceil(B 9 n / 256), block 256; j0 + n <= J (checked when the plan is made).
//   (the blend itself is the BLEND form of k_unlayout_vertices, above)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rotvecs_to_mats(const float* __restrict__ rv, float* __restrict__ mats, int n) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  const float r[3] = {rv[3 * k], rv[3 * k + 1], rv[3 * k + 2]};
  float m[9];
  sf::rotvec2mat(r, m);
#pragma unroll
  for (int e = 0; e < 9; ++e) mats[9 * k + e] = m[e];
}

__global__ __launch_bounds__(256) void k_replace_rotations(const float* __restrict__ mats, const float* __restrict__ rv,
                                                           float* __restrict__ rel, float* __restrict__ pose, int B, int J,
                                                           int j0, int n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t run = (size_t)9 * n;
  if (i >= (size_t)B * run) return;
  const size_t b = i / run, e = i - b * run;
  rel[(b * J + j0) * 9 + e] = mats[e];
  if (pose && e < (size_t)3 * n) pose[(b * J + j0) * 3 + e] = rv[e];
}
