// libsmplfit_hip.so — HIP kernels (gfx950 / CDNA4) and the C-ABI of include/smplfit.h.
//
// Kernel inventory.  Wave-per-instance kernels (every configuration; grid = instances unless noted):
//   k_center_sort_partsum(_lds)  K0  mean-centre targets, re-order vertices by body part (SoA), part sums against
//                                    the template mesh
//   k_joint_stage          K1  part rotations (SO(3) projections, swing-twist), shape prologue (FK + beta-Jacobian,
//                              pose feature, joint normal equations)
//   k_posedirs_gemm*       K2  v_posed = v_template + pose_feature . posedirs: split-bf16 on the matrix cores
//                              (k_posedirs_gemm_bf16x3, _tiled for K > 208) or fp32 MFMA (_as, generic)
//   k_shape_accum          K3  vertex block of the normal equations (weighted / non-batch-major configurations)
//   k_shape_solve          K4  fp64 centring + Cholesky + translation (share_beta: + k_share_reduce; scale options:
//                              k_scale_extras + k_shape_solve_scaled + k_scale_refs)
//   k_lbs_partsum          K5  vertices at the solved shape fused with the part sums of the next rotation pass
//   k_refine_epilogue      K6  dependent rotation refinement + relative rotations + log map
//   k_forward_joint, k_lbs_partsum<MODE 2>   BodyModel.forward;  k_scale_trans  known-shape alignment
//   k_bwd_vertex, k_bwd_reduce, k_bwd_combine, k_bwd_joint   its backward (kernels_bwd.inc)
//   k_obj_vertex                                           value + gradient of the mesh-distance objective (same file)
//   k_adj_gram, k_adj_apply, k_adj_combine                 adjoint of the shape solve: gradients of fit_with_known_pose
//                                                          (kernels_adj.inc)
//   k_rototranslate, k_rototranslate_backward              BodyModel.rototranslate and its backward: lane = instance,
//                                                          pose rows copied coalesced (kernels_rigid.inc)
// Batch-major kernels (LANE = INSTANCE; the default vertex block where they apply, see route_of): k_layout_targets,
//   k_mean_finish, k_template_partsum_bm, k_residual_bm, k_pair_gram_bm, k_gram_combine_bm, k_lbs_partsum_bm,
//   k_psum_combine, k_regress_joints_bm, k_transpose_targets (joint rows) — grid = (vertex group | unit chunk) x
//   instance blocks of 64; k_transfer_bm / k_transfer_rows: topology transfer (BodyConverter), k_transfer_rows on the
//   transposed matrix: its adjoint (smplfit_transfer_backward_f32).
// Everything is enqueued on the caller's stream; no host synchronisation, no allocation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include <type_traits>

#include "../../include/smplfit.h"
#include "sf_rigid.h"
#include "sf_stages.h"
#include "sf_tables.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define SF_HIP_TRY(expr)                                                                   \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(SMPLFIT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

// ------------------------------------------------------------------------------------------------
// device-side model
// ------------------------------------------------------------------------------------------------
struct DevModel {
  int V, J, S, P, Vp, Kp, KW, n_used, nseg;
  sf::JointTabs jt;
  const int32_t* perm;      // (Vp)
  const int32_t* inv_slot;  // (V) sorted slot of every original vertex
  const int32_t* segments;  // (nseg,3)
  const int32_t* part_seg_start;  // (J+1) first segment of each part (empty range: unused part)
  const float *vt, *dm, *sd, *wval, *pdSw, *j_template, *cpackA, *cpackB, *gblob;
  const uint16_t* pdB;  // split-bf16 tile images of posedirs (Kp == 208), see HostTables::pdB
  const uint16_t* pdB2; // split-bf16 stage images for the tiled GEMM (Kp != 208), HostTables::pdB2
  int kc32;
  int gemm_exclusive;  // the split-bf16 GEMM kernels own whole CUs (smplfit_handle::gemm_vgprs >= 256)
  const int32_t* gtiles;  // (ngt,3) start, count, part
  int ngt;
  const uint32_t* widx;
  const int32_t *reg_start, *reg_slot;
  const float* reg_val;
  const float* reg_rowsum;
  // batch-major vertex kernels (HostTables::vpieces / brec; the share tables travel as ShareView arguments)
  int bm_tables;              // the model has batch-major tables (<= 4 skinning weights per vertex)
  const float* brec;          // (Vp, brec_stride) per-slot records: shapedirs + 4 weights in the piece's joint order
  const float *pair_E, *pair_c2e, *diag_c2e;  // constants of k_pair_gram_bm (HostTables)
  const int32_t *jn_start, *jn;               // neighbours of every joint (HostTables::jn)
  // GENERAL path (more than 16 betas / more than 8 skinning weights per vertex, kernels_gen.inc)
  int general;
  const float* sdg;        // (Vp, 3, S4) shapedirs, vertex-major, rows padded to a multiple of four
  const int32_t* segall;   // (nsegall, 3) part-aligned tiles over every slot
  int nsegall;
  // k_prologue_bm: the ancestors of every joint from the root down (CSR; the joint itself excluded)
  const int32_t *anc_start, *anc;
};

// One cell table on the device (sf::ShareTable) as the kernels take it, with the multiplier a launch picked.
struct ShareView {
  const int32_t* piece_start;  // (ncells + 1)
  const int32_t* pieces;       // (npieces + 1, kPieceRec)
  // LBS tables: rows of every part, CSR (part_row_start (J + 1), part_rows); residual tables: the resP rows holding a
  // joint's residual moments, CSR (mb_start (J + 1), mb_row)
  const int32_t *aux_start, *aux_rows;
  int ncells, nrows;
  int rec;   // ints per piece record: 12, or 24 for pieces of up to eight joints (sf::HostTables::piece_rec)
  int mult;  // cells per wave: share s walks the cells [s * mult, (s + 1) * mult)
  int fine;  // the fine table of its kind (small batches): the combine kernels split the rows over waves
  int max_aux;  // longest CSR run of aux_rows (a joint's moment rows / a part's rows)
  // residual tables: the CSR as rows of aux_pitch (max_aux rounded up to 16) entries per joint, -1 behind a joint's last
  // row (k_solve_bm)
  const int32_t* aux_pad;
  int aux_pitch;
};

// The device arrays of one object (a handle, a transfer matrix, a plan): every one is allocated through it — 16 bytes
// at least — and they are freed together.  A failed call leaves the HIP call and its error in smplfit_last_error().
struct DeviceArrays {
  std::vector<void*> ptrs;
  template <class P>
  int alloc(size_t bytes, P* dst) {  // uninitialised
    void* p = nullptr;
    bytes = std::max<size_t>(bytes, 16);
    SF_HIP_TRY(hipMalloc(&p, bytes));
    ptrs.push_back(p);
    *dst = (P)p;
    return 0;
  }
  template <class T, class P>
  int upload(const T* src, size_t count, P* dst) {
    if (int rc = alloc(count * sizeof(T), dst)) return rc;
    if (count) SF_HIP_TRY(hipMemcpy((void*)*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
  template <class T, class P>
  int upload(const std::vector<T>& src, P* dst) { return upload(src.data(), src.size(), dst); }
  void free_all() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
};

}  // namespace

constexpr int kMaxChunks = 4;  // batch chunks of one fit call run on the caller's stream + 3 side streams

// k_refine_bm: the wave that owns an adjustable part (sf::HostTables::refine_waves)
struct RefGroups { int8_t wave[sf::kRefMaxAdj]; };

struct smplfit_handle {
  sf::HostTables t;
  DevModel d{};
  // the cell tables of the batch-major vertex kernels on the device: views[kind]
  std::vector<ShareView> views;
  DeviceArrays dev;
  bool has_device = false;
  // registers per lane the split-bf16 GEMM kernels were built with (hipFuncGetAttributes at create).  They must own
  // the whole register file of a CU (256 x 8 waves, see k_posedirs_gemm_bf16x3 "exclusive CU"); if a toolchain ever
  // allocates fewer, the fp32-MFMA GEMM is used instead
  int gemm_vgprs = 0;
  // fork/join resources of the chunked fit (see smplfit_fit_f32); guarded by `mu`
  hipStream_t side[kMaxChunks - 1] = {};
  hipEvent_t ev_fork = nullptr, ev_join[kMaxChunks - 1] = {};
  bool have_streams = false;
  mutable std::mutex mu;
};

// Topology-transfer matrix (BodyConverter's vertex_converter_csr, pt/bodyconverter.py:31-47): host + device CSR, and
// the CSR of its transpose (t_*, sf::transpose_csr) for smplfit_transfer_backward_f32.
struct smplfit_transfer {
  int v_in = 0, v_out = 0;
  std::vector<int32_t> indptr, indices, t_indptr, t_indices;
  std::vector<float> values, t_values;
  int32_t *d_indptr = nullptr, *d_indices = nullptr, *d_t_indptr = nullptr, *d_t_indices = nullptr;
  float *d_values = nullptr, *d_t_values = nullptr;
  DeviceArrays dev;
  bool negate_x = false;  // SMPLFIT_TRANSFER_NEGATE_X: x -> -x after the product (the mirror of BodyFlipper)
};

// Fused conversion plan (smplfit_convert_f32): the transfer matrix re-indexed to the sorted slots of the two models.
struct smplfit_convert_plan {
  const smplfit_handle *in = nullptr, *out = nullptr;
  int nslab = 0;
  int32_t *d_oslot = nullptr, *d_start = nullptr, *d_islot = nullptr;
  float* d_w = nullptr;
  DeviceArrays dev;  // (of a plan of its own; the arrays of a flip plan's `conv` are the flip plan's)
  bool negate_x = false;  // the matrix was made with SMPLFIT_TRANSFER_NEGATE_X
};

// Fused flip plan (smplfit_flip_f32): the mirror matrix at the sorted slots of the kid handle (in = out) and the
// joint mirror map.
struct smplfit_flip_plan {
  smplfit_convert_plan conv;
  int32_t* d_perm = nullptr;  // (J)
  DeviceArrays dev;
};

// Fused hand replacement plan (smplfit_replace_hands_f32): the constants of HandReplacer on the device.
struct smplfit_replace_hands_plan {
  const smplfit_handle* h = nullptr;
  int j0 = 0, n = 0;          // the joints [j0, j0 + n) are overwritten
  float* d_fitw = nullptr;    // (V) vertex weights of the fit, one row for the whole batch
  float* d_mix = nullptr;     // (V) blend weight of the new mesh
  float* d_rv = nullptr;      // (3 n) replacement rotation vectors
  float* d_mats = nullptr;    // (n, 9) the same as rotation matrices (k_rotvecs_to_mats)
  DeviceArrays dev;
};

// Segments of a share_beta batch (smplfit_fit_segments_f32 / smplfit_shape_solve_segments_f32): the tables of
// sf::build_share_segments on the host and, unless the plan is host-only, on the device.
struct smplfit_share_segments {
  sf::ShareSegments t;
  int32_t *d_row_seg = nullptr, *d_seg_blk = nullptr, *d_blk_rows = nullptr;
  DeviceArrays dev;
  bool has_device = false;
};

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// DPP wave-64 sum (6 VALU ops, no LDS traffic); the total lands in lane 63.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_step(float v) {
  const int x = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false);
  return v + __builtin_bit_cast(float, x);
}
__device__ __forceinline__ float wave_sum_last(float v) {
  v = dpp_step<0x111, 0xf>(v);  // row_shr:1
  v = dpp_step<0x112, 0xf>(v);  // row_shr:2
  v = dpp_step<0x114, 0xf>(v);  // row_shr:4
  v = dpp_step<0x118, 0xf>(v);  // row_shr:8   -> lane 15 of each row holds the row total
  v = dpp_step<0x142, 0xa>(v);  // row_bcast:15 into rows 1,3
  v = dpp_step<0x143, 0xc>(v);  // row_bcast:31 into rows 2,3 -> lane 63 holds the wave total
  return v;
}

// the per-instance stages of sf_stages.h run with one wave per instance: lane / n / sync / sum_to_last
struct DevCtx {
  int lane, n;
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ float sum_to_last(float v) const { return wave_sum_last(v); }  // (n == 64: one wave)
};

// the same over each half of the wave: the half totals land in lanes 31 and 63
__device__ __forceinline__ float half_sum_last(float v) {
  v = dpp_step<0x111, 0xf>(v);
  v = dpp_step<0x112, 0xf>(v);
  v = dpp_step<0x114, 0xf>(v);
  v = dpp_step<0x118, 0xf>(v);
  v = dpp_step<0x142, 0xa>(v);
  return v;
}

// Small-model form of the per-instance stages (J <= 32): TWO instances per wave, 32 lanes each.  Those stages are
// VALU-issue bound and most of their loops run over the joints, so a 24-joint model leaves 40 of the 64 lanes idle;
// with two instances per wave the same instructions serve both.  The barrier is the workgroup's (both halves run the
// same uniform control flow), the scratch of half h starts at h * <stage scratch>.
struct DevCtxHalf {
  int lane, n;
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ float sum_to_last(float v) const { return half_sum_last(v); }
};
template <int N> struct StageCtx { using type = DevCtx; };
template <> struct StageCtx<32> { using type = DevCtxHalf; };

// Per-call workspace carve (device pointers).
struct Workspace {
  float* tvs;      // (B,3,Vp)   centred targets, sorted slots, SoA
  float* vws;      // (B,Vp)     vertex weights, sorted slots (when given)
  float* vposed;   // (Mp,3*Vp)  GEMM output
  float* rp;       // (Mp,Kp)    pose features (GEMM A)
  float* mean;     // (B,3)
  float* tjc;      // (B,J,3)    centred target joints
  float* psum;     // (B,J,16)
  float* G;        // (B,J,9)
  float* jd;       // (B,J,jd_stride)
  float* jdT;      // (Mp/64, J*jd_stride padded to 64, 64) the same, instance-innermost (pair-Gram kernel)
  float* pext;     // (B,J,3,S+1)
  float* gramj;    // (B,NE+1)
  double* gramv;   // (B,NE+1)
  float* beta;     // (B,S)
  float* trans;    // (B,3)
  float* jb;       // (B,J,4)
  float* jbT;      // (Mp/64, J*4, 64) the same, instance-innermost (batch-major LBS kernel)
  float* rjoints;  // (B,J,3)
  float* rverts;   // (B,3,Vp) re-evaluated vertices (joints-omitted path only)
  float* tjreg;    // (B,J,3) regressed target joints (joints-omitted path)
  float* rjreg;    // (B,J,3) regressed reference joints
  float* mbj;      // (B,J,3) per-joint residual moments (pair-Gram form)
  float* scale;    // (B) scale_corr of the known-shape fit
  float* regref;   // (B,S) ridge reference of the warm-started fit
  double* cen;     // (B, S*S+S) centred regularised systems of a share_beta fit (general path: one chunk of share_chunk() rows)
  double* cenP;    // (partial blocks, S*S+S) partial sums of the rows above (k_share_partial); ceil(B/64) rows here,
                   // a plan of segments brings its own (segments_layout)
  double* censum;  // (segments, S*S+S) their sums per segment; one row here (row B of cen; general path: a row of its
                   // own), a plan of segments brings its own
  double* gvex;    // (B, S+6) general path: extra sums of the scaled solve (target column of k_gen_accum_mfma)
  float* vextra;   // (B,32) extra vertex sums of the scaled solve (scale_extras_vertex)
  float* beta_out; // (B,S) undivided shape of the scaled solve (ws.beta holds the evaluated one)
  float* tjs;      // (B,J,3) target joints times the scale (scale_target refinement)
  // batch-major path: streams with the instance index innermost (lane = instance reads coalesce)
  float* vpT;      // (Mp/64, 3*Vp, 64) v_posed, written by the GEMM
  float* tT;       // (Mp/64, 3*Vp, 64) targets AS GIVEN at their sorted slots (padding slots: the mean); the
                   // consumers subtract ws.mean (k_layout_targets / k_mean_finish)
  float* psumP;    // (rows, 16, Mp) part sums per row of the LBS share table
  float* resP;     // ([share][16] + [segment row][3 kGQ], Mp) residual-pass sums (k_residual_bm); scratch of the layout pass
  float* gramP;    // (workgroups of k_pair_gram_bm, NG, Mp) pair-Gram partial sums
  float* wT;       // (Mp/64, Vp, 64) vertex weights at the sorted slots (padding slots: 0), k_layout_weights
  float* accP;     // (cells, NE+1, Mp) cell records of the weighted accumulate (k_accum_w_bm)
  // general path: the S-sized scratch of the per-instance stages lives here instead of LDS
  float* gT;       // (B,J,3,S+1) T = P - G J_ext of the joint stage (its P is ws.pext)
  float* gsolve;   // (B, gen_solve_scratch_floats(S)) the scratch of stage S / S' (the S x S system)
  // batch-major prologue (k_prologue_bm, round 6)
  float* GT;       // (J*9, Mp) global rotations, instance-innermost (written by k_joint_stage beside ws.G)
  float* pextT;    // (J*3*(S+1), Mp) FK positions with their beta-Jacobian, instance-innermost
  float* gramjP;   // (prologue workgroups per instance block, NE+1, Mp) partial sums of the joint block
  uint16_t* rpP;   // (Mp/32, sf::kPlaneRuns, 64, 8) the pose features as split-bf16 planes in the fragment order of
                   // k_posedirs_gemm_bf16x3 (sf::plane_off), written by k_prologue_bm instead of ws.rp on the route
                   // gemm_planes; Kp == 208 only.  No region of its own: the head of ws.vposed (carve)
};

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The bump allocator of every workspace layout: regions handed out in order from `base`, each starting on a 256-byte
// boundary.  A null base only counts.  off: the bytes taken so far, a multiple of 256 — the size of the layout once
// its function has run.  Nothing else aligns or advances a workspace offset.
struct Arena {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t count) {
    const size_t o = off;
    off = align_up(off + count * sizeof(T), 256);
    return base ? reinterpret_cast<T*>(base + o) : nullptr;
  }
};

// Kernels that may ask for more than 64 KB of dynamic LDS: the attribute is set once per (device, kernel) — a list
// under a mutex, so that every device id has its own entry (round 5 kept 16 flags indexed by id & 15: the ids from 16
// up shared a flag with a lower id and never got the attribute)
void ensure_max_lds(const void* fn) {
  static std::mutex mu;
  static std::vector<std::pair<int, const void*>> done;
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  std::lock_guard<std::mutex> lock(mu);
  for (const auto& e : done)
    if (e.first == dev_id && e.second == fn) return;
  // (a failed call is not recorded: the next launch of the kernel tries again)
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess)
    done.emplace_back(dev_id, fn);
}

// Work units of k_pair_gram_bm (kernels_bm.inc): every joint twice + chunks of kPgPairs joint pairs; a workgroup of
// kPgWaves waves takes kPgWaves units and writes ONE upper triangle to ws.gramP.  Shared by the workspace carve, the
// launch and the combine kernels.
// (3 pairs per chunk: 77 units = 10 workgroups per instance block for the SMPL-shaped model — 640 workgroups at
// B = 4096, one round of the chip at 2.5 resident workgroups per CU; with 2 pairs per chunk (rounds 4 - 5) 832: a second,
// mostly empty round: 27.3 -> 24.7 us, SMPL-X 57 -> 54)
#ifndef SMPLFIT_PG_PAIRS
#define SMPLFIT_PG_PAIRS 3
#endif
constexpr int kPgWaves = 8, kPgPairs = SMPLFIT_PG_PAIRS;
constexpr int pair_gram_units(int J, int npairs) { return 2 * J + (npairs + kPgPairs - 1) / kPgPairs; }
constexpr int pair_gram_workgroups(int J, int npairs) { return (pair_gram_units(J, npairs) + kPgWaves - 1) / kPgWaves; }
constexpr int kProWaves = 8;  // joints (= waves) per workgroup of k_prologue_bm
using sf::kRefWaves, sf::kRotSlots, sf::res_share_rec, sf::kResRowRec;  // (sf_tables.h: the table builder uses them too)
constexpr int prologue_splits(int J) { return (J + kProWaves - 1) / kProWaves; }
constexpr int kAccExtrasHost = 16;  // (= kAccExtras of kernels_bm.inc: the extras of the scaled solve behind a cell record)

#ifndef SMPLFIT_SLAB
#define SMPLFIT_SLAB 32  // original vertices per workgroup of k_layout_targets (kSlabV)
#endif

// fwd_only: the slice a batch-major forward of this model needs (the input side of a fused conversion, see
// smplfit_convert_f32): pose features, joint rows, shape / translation and the instance-innermost v_posed buffer.
// general path: instances per chunk of a share_beta solve (the workspace reserves their S^2 + S doubles)
inline int share_chunk(int B) { return std::min((B + 63) / 64 * 64, 256); }

// LAYOUT fit: the workspace of one fit / forward / shape solve of B instances (smplfit_workspace_bytes: its chunks).
Workspace carve(const sf::HostTables& t, int B, Arena& ar, bool fwd_only = false) {
  const size_t Mp = align_up((size_t)B, 128);
  const size_t Vp = t.Vp, J = t.J, S = t.S, NE1 = t.ne() + 1;
  auto take = [&](size_t bytes, bool fwd = false) {  // fwd: also part of the forward-only slice
    return fwd_only && !fwd ? (char*)nullptr : ar.take<char>(bytes);
  };
  Workspace ws;
  ws.tvs = (float*)take((size_t)B * 3 * Vp * 4);
  ws.vws = (float*)take((size_t)B * Vp * 4);
  // instance-major GEMM output; on the batch-major path of a model with Kp != 208 it holds the split feature
  // images of the tiled GEMM instead (k_split_features: 32 KB per 256-instance tile and 32-k stage)
  ws.vposed = (float*)take(fwd_only ? (t.Kp != 208 ? (Mp + 255) / 256 * (size_t)((t.Kp + 31) / 32) * ((sf::kGemm3 ? 2 : 3) * 256 * 64) : 0)
                                    : Mp * 3 * Vp * 4, true);
  ws.rp = (float*)take(Mp * t.Kp * 4, true);
  ws.mean = (float*)take((size_t)B * 3 * 4);
  ws.tjc = (float*)take((size_t)B * J * 3 * 4);
  ws.psum = (float*)take((size_t)B * J * sf::kPsum * 4);
  ws.G = (float*)take((size_t)B * J * 9 * 4);
  ws.jd = (float*)take((size_t)B * J * sf::jd_stride(S) * 4, true);
  ws.pext = (float*)take((size_t)B * J * 3 * (S + 1) * 4);
  ws.gramj = (float*)take((size_t)B * NE1 * 4);
  ws.gramv = (double*)take((size_t)B * NE1 * 8);
  ws.beta = (float*)take((size_t)B * S * 4, true);
  ws.trans = (float*)take((size_t)B * 3 * 4, true);
  ws.jb = (float*)take((size_t)B * J * 4 * 4, true);
  ws.jbT = (float*)take(Mp * J * 4 * 4, true);
  ws.rjoints = (float*)take((size_t)B * J * 3 * 4, true);
  ws.rverts = (float*)take((size_t)B * 3 * Vp * 4);
  ws.tjreg = (float*)take((size_t)B * J * 3 * 4);
  ws.rjreg = (float*)take((size_t)B * J * 3 * 4);
  ws.mbj = (float*)take((size_t)B * J * 3 * 4);
  ws.scale = (float*)take((size_t)B * 4);
  ws.regref = (float*)take((size_t)B * S * 4, true);
  // (general path: (S^2 + S) doubles per instance — 0.7 MB at S = 300 — are reserved for ONE chunk of the batch; a
  // share_beta solve writes and sums the instances' systems chunk by chunk, in the order of the unchunked sum)
  ws.cen = (double*)take((t.general ? (size_t)share_chunk(B) : (size_t)B + 1) * (S * S + S) * 8);
  ws.cenP = (double*)take(((size_t)B + 63) / 64 * (S * S + S) * 8);
  ws.censum = t.general ? (double*)take((S * S + S) * 8) : (ws.cen ? ws.cen + (size_t)B * (S * S + S) : nullptr);
  ws.gvex = (double*)take(t.general ? (size_t)B * (S + sf::kScaleExtras) * 8 : 0);
  ws.vextra = (float*)take((size_t)B * 32 * 4);
  ws.beta_out = (float*)take((size_t)B * S * 4);
  ws.tjs = (float*)take((size_t)B * J * 3 * 4);
  // (the batch-major streams: never read on the general path)
  ws.vpT = (float*)take(t.general ? 0 : Mp * 3 * Vp * 4, true);
  ws.tT = (float*)take(t.general ? 0 : Mp * 3 * Vp * 4);
  {
    // rows of partial sums: the coarse tables', and the fine tables' as well for a batch that may take them (whatever
    // SMPLFIT_FINE_B says at the time of the call)
    size_t lbs_rows = 0, res_rows = 0;
    for (size_t k = 0; k < t.shares.size(); ++k) {
      if ((int)k >= sf::kShareFine && B > sf::kFineMaxBatch) break;
      if ((int)k % sf::kShareKinds == sf::kShareResidual)
        res_rows = std::max(res_rows, (size_t)t.shares[k].ncells * ((S + 3 + 3) / 4 * 4) + (size_t)t.shares[k].nrows * 3 * sf::kGroupJoints);
      else lbs_rows = std::max(lbs_rows, (size_t)t.shares[k].nrows);
    }
    // (the layout kernel's slab sums use ws.resP as scratch: 3 rows per slab)
    const size_t nslab = ((size_t)t.V + SMPLFIT_SLAB - 1) / SMPLFIT_SLAB;
    ws.psumP = (float*)take(lbs_rows * 16 * Mp * 4);
    ws.resP = (float*)take(std::max(res_rows, 3 * nslab) * Mp * 4);
    // weighted fits on the batch-major path: the weight stream and the cell records of k_accum_w_bm
    size_t acc_cells = 0;
    for (size_t k = sf::kShareResidual; k < t.shares.size(); k += sf::kShareKinds)
      if ((int)k < sf::kShareFine || B <= sf::kFineMaxBatch) acc_cells = std::max(acc_cells, (size_t)t.shares[k].ncells);
    ws.wT = (float*)take(t.shares.empty() ? 0 : Mp * Vp * 4);
    ws.accP = (float*)take(acc_cells * (NE1 + kAccExtrasHost) * Mp * 4);
  }
  {  // k_pair_gram_bm: one upper triangle (NG rows) per workgroup of its launch (pair_gram_workgroups: the same
     // constants as the launch and the combine kernels)
    ws.gramP = (float*)take((size_t)pair_gram_workgroups((int)J, (int)t.pair_c3.size()) * sf::ne_ng((int)S) * Mp * 4);
  }
  ws.jdT = (float*)take(t.general ? 0 : Mp * align_up((size_t)J * sf::jd_stride(S), 64) * 4, true);
  ws.gT = (float*)take(t.general ? (size_t)B * J * 3 * (S + 1) * 4 : 0, true);
  ws.gsolve = (float*)take(t.general ? (size_t)B * align_up((size_t)sf::gen_solve_scratch_floats((int)S), 4) * 4 : 0);
  const bool pro = !t.general && !t.shares.empty();  // (the models the batch-major path can serve)
  ws.GT = (float*)take(pro ? Mp * J * 9 * 4 : 0);
  ws.pextT = (float*)take(pro ? Mp * J * 3 * (S + 1) * 4 : 0);
  ws.gramjP = (float*)take(pro ? (size_t)prologue_splits((int)J) * NE1 * Mp * 4 : 0);
  // the feature planes of the route gemm_planes live in ws.vposed, which only the wave-per-instance vertex kernels
  // read and no batch-major fit touches (as the feature images of the tiled GEMM, launch_gemm): 864 of its 12 Vp bytes
  // per instance.  Every 16 bytes of them are written by k_prologue_bm before the GEMM reads them, the pad instances'
  // as zeros.
  ws.rpP = pro && !fwd_only && sf::kGemm3 && t.Kp == 16 * sf::kPlaneSteps && 12 * Vp >= sf::kPlaneGroupBytes / 32
               ? reinterpret_cast<uint16_t*>(ws.vposed) : nullptr;
  return ws;
}

// Cache policy of the streams.  The per-iteration streams of a fit (v_posed, the targets: 0.34 GB each at B = 4096)
// are written once and read once per pass, and together they are several times the 256 MB Infinity Cache and the
// 32 MB of L2: left to the default policy, the producer's output lingers as dirty lines that the NEXT kernel's reads
// push out — its write-back then competes with those reads (measured, B = 4096: the residual pass takes 178 us behind
// the GEMM, 145 us on its own) — and the streams evict the tables every wave re-reads.  Marked non-temporal, stream
// reads and writes pass through: residual 178 -> 126 us, LBS 142 -> 120, GEMM 106 -> 97, layout 150 -> 126,
// 2.01 -> 2.4 M fits/s, bit-identical results.  SMPLFIT_NT selects which accesses carry the hint (A/B builds):
// 1 stream loads of the batch-major vertex passes, 2 GEMM output stores, 4 target loads of the layout pass (slower:
// 139 us — off), 8 its stores (and the topology transfer's), 16 the streams of the wave-per-instance kernels (K0's
// sorted copy, the reads of K3 / K5).
#ifndef SMPLFIT_NT
#define SMPLFIT_NT 27
#endif
template <int BIT>
__device__ __forceinline__ float ld_stream(const float* p) {
  if constexpr ((SMPLFIT_NT & BIT) != 0) return __builtin_nontemporal_load(p);
  else return *p;
}
template <int BIT>
__device__ __forceinline__ void st_stream(float* p, float v) {
  if constexpr ((SMPLFIT_NT & BIT) != 0) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// the kernels (same anonymous namespace, same translation unit)
#include "kernels_wave.inc"
#include "kernels_bm.inc"
#include "kernels_gen.inc"
#include "kernels_bwd.inc"
#include "kernels_adj.inc"
#include "kernels_rigid.inc"
#include "kernels_robust.inc"
#include "kernels_align.inc"

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// Tuning switches.  Every SMPLFIT_* environment variable the launch code honours is read ONCE (first use) into
// this struct — no getenv on the launch path; smplfit_reload_options() re-reads them (tests and the A/B tools
// switch paths inside one process).  INTEGRATION.md documents each of them.
// ------------------------------------------------------------------------------------------------
struct Tuning {
  bool bm = true;          // SMPLFIT_BM=0: wave-per-instance vertex kernels everywhere
  bool gemm_f32 = false;   // SMPLFIT_GEMM=f32: fp32-MFMA posedirs GEMM instead of the split-bf16 one
  bool pair_form = false;  // SMPLFIT_SHAPE_FORM=pair: pair-Gram form on the wave-per-instance path
  int chunks = 0;          // SMPLFIT_CHUNKS=1..4: concurrent batch chunks of one fit call (0: by model, see chunk_plan)
  int stage_half_b = 2048; // SMPLFIT_STAGE_HALF_B: smallest batch whose per-instance stages run two instances per wave (J <= 32)
  int fine_b = sf::kFineMaxBatch;  // SMPLFIT_FINE_B: largest batch that takes the fine cell tables (0: none; at most sf::kFineMaxBatch)
  bool bm_known_pose = true;  // SMPLFIT_BM_KNOWN_POSE=0: smplfit_shape_solve_ex_f32 on the wave-per-instance kernels (A/B)
  bool bm_forward = true;  // SMPLFIT_BM_FORWARD=0: BodyModel.forward on the wave-per-instance LBS kernel (A/B)
  bool bm_scale = true;    // SMPLFIT_BM_SCALE=0: fit(scale_target / scale_fit) on the wave-per-instance kernels (A/B)
  bool bm_known_shape = true;  // SMPLFIT_BM_KNOWN_SHAPE=0: fit_with_known_shape on the wave-per-instance kernels (A/B)
  bool bm_weighted = true; // SMPLFIT_BM_WEIGHTED=0: fits with vertex weights on the wave-per-instance kernels (A/B)
  int share_slots = 4096;  // SMPLFIT_BM_SLOTS: resident waves a batch-major vertex pass is dealt for (share-count choice)
  bool gen_mfma = true;    // SMPLFIT_GEN_MFMA=0: the general path's vertex block on the vector ALUs (k_gen_accum) instead of the matrix cores (A/B)
  bool rot_bm = true;      // SMPLFIT_ROT_BM=0: the part rotations as the wave-per-instance k_joint_stage behind a part-sum combine instead of k_rotations_bm (A/B)
  bool rot_spread = true;  // SMPLFIT_ROT_SPREAD=0: the part rotations always as k_rotations_bm / k_rotations_bm_rounds (a workgroup per 64 instances, its waves fit several joints each), never as k_rotations_spread (a joint per wave, the joints over the grid's second dimension) (A/B, bit-identical)
  int rot_spread_b = kRotSpreadMaxBatch;  // SMPLFIT_ROT_SPREAD_B: the most instances of a call (all its chunks together) that take k_rotations_spread
  bool refine_bm = true;   // SMPLFIT_REFINE_BM=0: the refinement + epilogue as the wave-per-instance k_refine_epilogue behind a part-sum combine instead of k_refine_bm (A/B)
  bool prologue_bm = true; // SMPLFIT_PROLOGUE_BM=0: the shape prologue inside k_joint_stage + the joint-row transpose instead of k_prologue_bm (A/B)
  bool solve_bm = true;    // SMPLFIT_SOLVE_BM=0: normal-equation combine + wave-per-instance solve as two launches instead of k_solve_bm (A/B)
  bool gemm_planes = true; // SMPLFIT_GEMM_PLANES=0: k_prologue_bm writes the fp32 feature rows and k_posedirs_gemm_bf16x3 splits them itself, instead of the split planes (A/B, bit-identical)
};
// The current options: an immutable snapshot behind an atomic pointer.  smplfit_reload_options() publishes a new
// snapshot; a launch that is reading the old one on another thread keeps a valid object (snapshots are never freed:
// a few hundred bytes per reload).
std::atomic<const Tuning*> g_tune{nullptr};
std::mutex g_tune_mu;
Tuning read_tuning() {
  Tuning t;
  auto env = [](const char* n) { return getenv(n); };
  if (const char* e = env("SMPLFIT_BM")) t.bm = e[0] != '0';
  if (const char* e = env("SMPLFIT_GEMM")) t.gemm_f32 = e[0] == 'f';
  if (const char* e = env("SMPLFIT_SHAPE_FORM")) t.pair_form = std::string(e) == "pair";
  if (const char* e = env("SMPLFIT_CHUNKS")) t.chunks = std::min(std::max(atoi(e), 1), 4);
  if (const char* e = env("SMPLFIT_BM_KNOWN_POSE")) t.bm_known_pose = e[0] != '0';
  if (const char* e = env("SMPLFIT_BM_FORWARD")) t.bm_forward = e[0] != '0';
  if (const char* e = env("SMPLFIT_BM_SCALE")) t.bm_scale = e[0] != '0';
  if (const char* e = env("SMPLFIT_BM_KNOWN_SHAPE")) t.bm_known_shape = e[0] != '0';
  if (const char* e = env("SMPLFIT_BM_WEIGHTED")) t.bm_weighted = e[0] != '0';
  if (const char* e = env("SMPLFIT_FINE_B")) t.fine_b = std::min(std::max(atoi(e), 0), sf::kFineMaxBatch);
  if (const char* e = env("SMPLFIT_STAGE_HALF_B")) t.stage_half_b = std::max(atoi(e), 1);
  if (const char* e = env("SMPLFIT_BM_SLOTS")) t.share_slots = std::min(std::max(atoi(e), 256), 16384);
  if (const char* e = env("SMPLFIT_GEN_MFMA")) t.gen_mfma = e[0] != '0';
  if (const char* e = env("SMPLFIT_SOLVE_BM")) t.solve_bm = e[0] != '0';
  if (const char* e = env("SMPLFIT_GEMM_PLANES")) t.gemm_planes = e[0] != '0';
  if (const char* e = env("SMPLFIT_PROLOGUE_BM")) t.prologue_bm = e[0] != '0';
  if (const char* e = env("SMPLFIT_REFINE_BM")) t.refine_bm = e[0] != '0';
  if (const char* e = env("SMPLFIT_ROT_BM")) t.rot_bm = e[0] != '0';
  if (const char* e = env("SMPLFIT_ROT_SPREAD")) t.rot_spread = e[0] != '0';
  if (const char* e = env("SMPLFIT_ROT_SPREAD_B")) t.rot_spread_b = std::max(atoi(e), 0);
  return t;
}
void load_tuning() {
  std::lock_guard<std::mutex> lock(g_tune_mu);
  g_tune.store(new Tuning(read_tuning()), std::memory_order_release);
}
const Tuning& tune() {
  const Tuning* t = g_tune.load(std::memory_order_acquire);
  if (!t) {
    std::lock_guard<std::mutex> lock(g_tune_mu);
    t = g_tune.load(std::memory_order_acquire);
    if (!t) {
      t = new Tuning(read_tuning());
      g_tune.store(t, std::memory_order_release);
    }
  }
  return *t;
}

// Launches of the stage kernels since the process started, by smplfit_stage_id (smplfit_stage_launches): which stage
// kernels served a call is the route's decision and does not show in the results.  Each count is bumped at the one
// place its kernel is enqueued; host side only.
std::atomic<uint64_t> g_stage_launches[SMPLFIT_STAGE_COUNT] = {};
inline void count_stage(int id) { g_stage_launches[id].fetch_add(1, std::memory_order_relaxed); }

// joint rows of the current rotations, instance-innermost, for k_pair_gram_bm
void launch_jd_transpose(const DevModel& d, const Workspace& ws, int B, hipStream_t st) {
  const int Mp = (int)align_up((size_t)B, 128), Ns = d.J * sf::jd_stride(d.S), Np = (int)align_up((size_t)Ns, 64);
  hipLaunchKernelGGL(k_transpose_targets, dim3(Np / 64, Mp / 64), dim3(256), 0, st, ws.jd, ws.jdT, B, Np, Mp, Ns);
}

// The cell table a batch-major vertex pass of `kind` over B instances runs on, with its multiplier (sf::pick_share_mult).
// the table a launch over B instances walks: the fine one up to SMPLFIT_FINE_B instances (sf_tables.h)
int share_index(int kind, int B) { return kind + (B <= tune().fine_b ? sf::kShareFine : 0); }
ShareView share_view(const smplfit_handle* h, int kind, int B) {
  const int nblocks = (int)align_up((size_t)B, 128) / 64, idx = share_index(kind, B);
  ShareView sv = h->views[idx];
  sv.fine = idx >= sf::kShareFine;
  sv.mult = sf::pick_share_mult(h->t, idx, nblocks, tune().share_slots);
  return sv;
}
dim3 share_grid(const ShareView& sv, int Mp) { return dim3(Mp / 64, sv.ncells / sv.mult / kBW); }
void launch_psum_combine(const DevModel& d, const ShareView& sv, const Workspace& ws, int B, int Mp, hipStream_t st) {
  count_stage(SMPLFIT_STAGE_PSUM_COMBINE);
  if (sv.fine) hipLaunchKernelGGL(k_psum_combine_split<8>, dim3(Mp / 64, d.J), dim3(64 * 8), 0, st, d, sv, ws, B, Mp);
  else hipLaunchKernelGGL(k_psum_combine, dim3((B + 255) / 256, d.J), dim3(256), 0, st, d, sv, ws, B, Mp);
}

// part sums of the centred targets against the template + their combine (the first rotation estimate); combine:
// Route::psum_combine
void launch_template_partsum_bm(const smplfit_handle* h, const Workspace& ws, int B, hipStream_t st, bool weighted,
                                bool combine) {
  const DevModel& d = h->d;
  const int Mp = (int)align_up((size_t)B, 128);
  const ShareView sv = share_view(h, sf::kShareLbsUsed, B);
  if (weighted) hipLaunchKernelGGL(k_template_partsum_bm<true>, share_grid(sv, Mp), dim3(64 * kBW), 0, st, d, sv, ws, B, Mp);
  else hipLaunchKernelGGL(k_template_partsum_bm<false>, share_grid(sv, Mp), dim3(64 * kBW), 0, st, d, sv, ws, B, Mp);
  if (combine) launch_psum_combine(d, sv, ws, B, Mp, st);  // (k_rotations_bm adds the rows itself)
}

// Target layout of the batch-major path (k_layout_weights, k_layout_targets): ws.wT, ws.tT and the slab sums in
// ws.resP (scratch); launch_targets_in finishes them.  -> the slabs
// vw_shared: vw is one (V) row for the whole batch (TargetsIn::vw_shared)
int launch_layout_bm(const DevModel& d, const float* tv, const float* vw, const Workspace& ws, int B, hipStream_t st,
                     bool vw_shared = false) {
  if (vw) {  // vertex weights: their stream first (the template part sums read it)
    const dim3 grid((d.V + 63) / 64 + 1, (int)align_up((size_t)B, 128) / 64);
    if (vw_shared) hipLaunchKernelGGL(k_layout_weights<true>, grid, dim3(256), 0, st, d, vw, ws.wT, B);
    else hipLaunchKernelGGL(k_layout_weights<false>, grid, dim3(256), 0, st, d, vw, ws.wT, B);
  }
  const int Mp = (int)align_up((size_t)B, 128), nslab = (d.V + kSlabV - 1) / kSlabV;
  hipLaunchKernelGGL(k_layout_targets, dim3(nslab, Mp / 64), dim3(256), (size_t)64 * kSlabRow * 4, st, d, tv, ws.tT,
                     ws.resP, B, Mp);
  return nslab;
}

// K3' + K3g + K3c of the batch-major path for 10 betas (S = 10) and 10 betas + the kid unknown (S = 11)
template <int S>
void launch_residual_bm_s(const smplfit_handle* h, const Workspace& ws, int B, hipStream_t st, int which = 7) {
  const DevModel& d = h->d;
  const int Mp = (int)align_up((size_t)B, 128);
  const ShareView sv = share_view(h, sf::kShareResidual, B);
  if ((which & 1) && d.KW == 8)
    hipLaunchKernelGGL((k_residual_bm<S, 8>), share_grid(sv, Mp), dim3(64 * kBW),
                       kResidualLds, st, d, sv, ws, B, Mp);
  else if (which & 1)
    hipLaunchKernelGGL((k_residual_bm<S>), share_grid(sv, Mp), dim3(64 * kBW),
                       kResidualLds, st, d, sv, ws, B, Mp);
  if (which & 2) {
    hipLaunchKernelGGL((k_pair_gram_bm<S>), dim3(pair_gram_workgroups(d.J, d.jt.np), Mp / 64), dim3(64 * kPgWaves), 0, st, d, ws, B, Mp);
  }
  if (which & 4) count_stage(SMPLFIT_STAGE_GRAM_COMBINE);
  if ((which & 4) && sv.fine)
    hipLaunchKernelGGL((k_gram_combine_split<S, 16>), dim3(Mp / 64, S + 3 + 3 * d.J + sf::ne_ng(S)), dim3(64 * 16), 0,
                       st, d, sv, ws, B, Mp);
  else if (which & 4)
    hipLaunchKernelGGL((k_gram_combine_bm<S>), dim3((B + 255) / 256, S + 3 + 3 * d.J + sf::ne_ng(S)), dim3(256), 0,
                       st, d, sv, ws, B, Mp);
}
void launch_residual_bm(const smplfit_handle* h, const Workspace& ws, int B, hipStream_t st, int which = 7) {
  switch (h->d.S) {
    case 11: launch_residual_bm_s<11>(h, ws, B, st, which); break;
    case 16: launch_residual_bm_s<16>(h, ws, B, st, which); break;
    case 17: launch_residual_bm_s<17>(h, ws, B, st, which); break;
    default: launch_residual_bm_s<10>(h, ws, B, st, which);
  }
}

// the vertex block of the normal equations accumulated per vertex on the batch-major path (S = 10): cell records +
// their combine.  weighted: the vertex weights enter (else unit weights); extras: also the sums of the scaled solve
// (the last iteration of a scale_target / scale_fit fit)
void launch_accum_w_bm(const smplfit_handle* h, const Workspace& ws, int B, hipStream_t st, bool weighted = true,
                       bool extras = false) {
  static_assert(kAccExtrasHost == kAccExtras, "record layout");
  const DevModel& d = h->d;
  const int Mp = (int)align_up((size_t)B, 128);
  ShareView sv = share_view(h, sf::kShareResidual, B);
  // four workgroups per CU (their LDS): the multiplier for rounds of 1024 workgroups
  sv.mult = sf::pick_share_mult(h->t, share_index(sf::kShareResidual, B), Mp / 64, 1024, 1);
  const dim3 grid(Mp / 64, sv.ncells / sv.mult);
  const size_t lds = accum_w_lds<10>();
  if (!extras)
    hipLaunchKernelGGL((k_accum_w_bm<10, kAccWaves>), grid, dim3(64 * kAccWaves), lds, st, d, sv, ws, B, Mp);
  else if (weighted)
    hipLaunchKernelGGL((k_accum_w_bm<10, 1, true, true>), grid, dim3(64), lds, st, d, sv, ws, B, Mp);
  else
    hipLaunchKernelGGL((k_accum_w_bm<10, 1, false, true>), grid, dim3(64), lds, st, d, sv, ws, B, Mp);
  constexpr int NE1 = sf::ne_size(10) + 1;
  const int nent = NE1 + (extras ? 10 + 6 : 0), unit = weighted ? 0 : 1;
  if (sv.fine) hipLaunchKernelGGL((k_accum_combine<10, 16>), dim3(Mp / 64, nent), dim3(64 * 16), 0, st, d, sv, ws, B, Mp, unit);
  else hipLaunchKernelGGL((k_accum_combine<10, 4>), dim3(Mp / 64, nent), dim3(64 * 4), 0, st, d, sv, ws, B, Mp, unit);
}

// write_v (joints-omitted fits): every slot, the vertices at the solution written over ws.vpT, then the reference
// joints of the next rotation pass regressed from them into ws.rjreg.  adj_only (the last pass of a fit with target
// joints): the part sums feed the dependent refinement alone, which reads them at the adjustable parts
// (bodyfitter.py:1505-1517) — only those parts' slots are visited, the other rows of ws.psum become zero.
// combine: Route::psum_combine / psum_combine_last.
template <int S, int KW>
void launch_lbs_bm(const smplfit_handle* h, const Workspace& ws, int B, hipStream_t st, bool combine, bool write_v,
                   bool adj_only, bool weighted, bool write_all = false, int regress = -1) {
  const DevModel& d = h->d;
  const int Mp = (int)align_up((size_t)B, 128);
  const ShareView sv = share_view(h, write_v ? sf::kShareLbsAll : adj_only ? sf::kShareLbsAdj : sf::kShareLbsUsed, B);
  if constexpr ((KW == 4 || KW == 8) && sf::bm_shape_count(S)) {  // what route_of admits (10 / 16 betas with or without the kid unknown)
    if (write_v) {
      // (write_all: every posed vertex — the alignment sums of a known-shape fit; else the slots the regressor reads)
      const int wa = write_all ? 1 : 0;
      if (weighted)
        hipLaunchKernelGGL((k_lbs_partsum_bm<S, KW, true, false, true>), share_grid(sv, Mp), dim3(64 * kBW), 0, st, d, sv, ws, B, Mp, wa);
      else
        hipLaunchKernelGGL((k_lbs_partsum_bm<S, KW, true>), share_grid(sv, Mp), dim3(64 * kBW), 0, st, d, sv, ws, B, Mp, wa);
      // regress: the regressed reference joints are consumed (joints-omitted fits).  A known-shape fit WITH target
      // joints keeps the posed mesh for its alignment sums only; and a model without a regressor has none to apply
      const bool do_regress = (regress < 0 ? true : regress != 0) && h->t.has_regressor;
      if (do_regress)
        hipLaunchKernelGGL(k_regress_joints_bm<false>, dim3(Mp / 64, d.J), dim3(64), 0, st, d, ws.vpT, nullptr, ws.rjreg, B);
    } else if (weighted) {
      hipLaunchKernelGGL((k_lbs_partsum_bm<S, KW, false, false, true>), share_grid(sv, Mp), dim3(64 * kBW), 0, st, d, sv, ws, B, Mp);
    } else {
      hipLaunchKernelGGL((k_lbs_partsum_bm<S, KW>), share_grid(sv, Mp), dim3(64 * kBW), 0, st, d, sv, ws, B, Mp);
    }
  }
  if (combine) launch_psum_combine(d, sv, ws, B, Mp, st);
}

// the forward-only variant of the batch-major LBS pass (posed vertices left in ws.vpT): input side of a fused
// conversion, BodyModel.forward, the mesh of a shape solve
int launch_lbs_fwd_bm(const DevModel& d, const ShareView& sv, const Workspace& ws, int B, int Mp, hipStream_t st) {
  const dim3 grid = share_grid(sv, Mp);
#define SF_FWD(S_, KW_) hipLaunchKernelGGL((k_lbs_partsum_bm<S_, KW_, true, true>), grid, dim3(64 * kBW), 0, st, d, sv, ws, B, Mp)
  if (d.KW == 8) {
    switch (d.S) {
      case 11: SF_FWD(11, 8); break;
      case 16: SF_FWD(16, 8); break;
      case 10: SF_FWD(10, 8); break;
      default: return fail(SMPLFIT_ERR_UNSUPPORTED, "forward LBS pass: no batch-major kernel for this (betas, skinning width)");
    }
  } else {
    switch (d.S) {
      case 11: SF_FWD(11, 4); break;
      case 16: SF_FWD(16, 4); break;
      case 17: SF_FWD(17, 4); break;
      case 10: SF_FWD(10, 4); break;
      default: return fail(SMPLFIT_ERR_UNSUPPORTED, "forward LBS pass: no batch-major kernel for this (betas, skinning width)");
    }
  }
#undef SF_FWD
  return 0;
}

// The unit-weight vertex block has two implementations:
//   direct (default): k_shape_accum accumulates G, r, Sb per vertex (VALU-bound);
//   pair  (pair_form, Route::pair_in): k_residual + k_pair_gram — 4x fewer per-vertex FLOPs, parity-tested,
//          but not faster on wave-per-instance kernels (the batch-major path always uses the pair form).
template <int S, int KW>
int launch_shape_accum(const DevModel& d, const Workspace& ws, int B, bool weighted, bool pair_form, hipStream_t st) {
  const dim3 grid((B + kNW - 1) / kNW);
  if (weighted || !pair_form) {
    const size_t lds =
        ((size_t)kNW * d.J * sf::jd_stride(S) + 2 * 64 * sf::cpack_stride(S, KW) + 256 * 12) * 4;
    if (weighted)
      hipLaunchKernelGGL((k_shape_accum<S, KW, true>), grid, dim3(256), lds, st, d, ws, B);
    else
      hipLaunchKernelGGL((k_shape_accum<S, KW, false>), grid, dim3(256), lds, st, d, ws, B);
    return 0;
  }
  const size_t per_wave = ((size_t)d.J * sf::jd_stride(S) + 256 + (d.J + 1) * 4 + 3) / 4 * 4;
  const size_t blob = 64 * sf::cpack_stride(S, KW) + 16 * 64 + 16;
  hipLaunchKernelGGL((k_residual<S, KW>), grid, dim3(256), (kNW * per_wave + 2 * blob) * 4, st, d, ws, B);
  const size_t lds_g = ((size_t)d.J * sf::jd_stride(S) + (size_t)d.jt.np * 9 + (size_t)d.J * 3 * S) * 4;
  hipLaunchKernelGGL(k_pair_gram, dim3(B), dim3(64), lds_g, st, d, ws);
  return 0;
}

template <int S, int KW, int MODE, bool SOLVE>
void launch_lbs(const DevModel& d, const Workspace& ws, int B, bool weighted, int nb,
                const float* beta, const float* trans, float* out, float beta_reg, float beta_reg2,
                hipStream_t st, const float* kid = nullptr) {
  const size_t per_wave =
      ((size_t)d.J * sf::jd_stride(S) + d.J * 4 + 36 + (SOLVE ? sf::solve_scratch_floats(S) : 0) + 3) / 4 * 4;
  const size_t lds = (kNW * per_wave + 2 * 64 * sf::cpack_stride(S, KW)) * 4;
  const dim3 grid((B + kNW - 1) / kNW);
  if (weighted)
    hipLaunchKernelGGL((k_lbs_partsum<S, KW, true, MODE, SOLVE>), grid, dim3(256), lds, st, d, ws, B,
                       nb, beta, trans, kid, out, beta_reg, beta_reg2);
  else
    hipLaunchKernelGGL((k_lbs_partsum<S, KW, false, MODE, SOLVE>), grid, dim3(256), lds, st, d, ws, B,
                       nb, beta, trans, kid, out, beta_reg, beta_reg2);
  if (MODE == 1)
    hipLaunchKernelGGL((k_lbs_rest<S, KW>), dim3(B), dim3(256),
                       ((size_t)d.J * sf::jd_stride(S) + d.J * 4) * 4, st, d, ws);
}

// K0 dispatch: LDS-staged form when the (V,3) row fits in LDS, gather form otherwise.
// vw_shared: vw is one (V) row for the whole batch (TargetsIn::vw_shared)
void launch_center_sort(const DevModel& d, const float* tv, const float* tj, const float* vw,
                        const Workspace& ws, int B, hipStream_t st, bool vw_shared = false) {
  // vertices staged in LDS: the whole row, or — when that leaves room for one workgroup per CU only but
  // an 80 KB slice covers >= 15/16 of the row — the slice that lets two workgroups share the CU
  int VL = d.V;
  {
    const int cap = ((80 * 1024 - 64 * 4) / 12) & ~1;
    if (d.V > cap && d.V - cap <= d.V / 16) VL = cap;
  }
  const size_t lds_row = ((size_t)((3 * VL + 3) & ~3) + 64) * 4;
  if (lds_row <= 160 * 1024) {
    // dynamic LDS above 64 KB has to be opted into once per kernel (and per device: the attribute is
    // set again whenever the current device changes; idempotent, so racing threads are harmless)
    ensure_max_lds(reinterpret_cast<const void*>(&k_center_sort_partsum_lds<true>));
    ensure_max_lds(reinterpret_cast<const void*>(&k_center_sort_partsum_lds<false>));
    if (vw && vw_shared) {
      ensure_max_lds(reinterpret_cast<const void*>(&k_center_sort_partsum_lds<true, true>));
      hipLaunchKernelGGL((k_center_sort_partsum_lds<true, true>), dim3(B), dim3(1024), lds_row, st, d, tv, tj, vw, ws, VL);
    } else if (vw)
      hipLaunchKernelGGL((k_center_sort_partsum_lds<true>), dim3(B), dim3(1024), lds_row, st, d, tv, tj, vw, ws, VL);
    else
      hipLaunchKernelGGL((k_center_sort_partsum_lds<false>), dim3(B), dim3(1024), lds_row, st, d, tv, tj, vw, ws, VL);
    return;
  }
  const size_t lds0 = ((size_t)4 * d.J * sf::kPsum + 20) * 4;
  if (vw && vw_shared)
    hipLaunchKernelGGL((k_center_sort_partsum<true, true>), dim3(B), dim3(256), lds0, st, d, tv, tj, vw, ws);
  else if (vw)
    hipLaunchKernelGGL((k_center_sort_partsum<true>), dim3(B), dim3(256), lds0, st, d, tv, tj, vw, ws);
  else
    hipLaunchKernelGGL((k_center_sort_partsum<false>), dim3(B), dim3(256), lds0, st, d, tv, tj, vw, ws);
}

#define SF_DISPATCH_SKW(d, CALL)                                               \
  do {                                                                         \
    if ((d).S == 10 && (d).KW == 4) { CALL(10, 4); }                           \
    else if ((d).S == 10 && (d).KW == 8) { CALL(10, 8); }                      \
    else if ((d).S == 16 && (d).KW == 4) { CALL(16, 4); }                      \
    else if ((d).S == 16 && (d).KW == 8) { CALL(16, 8); }                      \
    else if ((d).S == 11 && (d).KW == 4) { CALL(11, 4); }                      \
    else if ((d).S == 11 && (d).KW == 8) { CALL(11, 8); }                      \
    else if ((d).S == 17 && (d).KW == 4) { CALL(17, 4); }                      \
    else return fail(SMPLFIT_ERR_UNSUPPORTED,                                  \
                     "unsupported (shape unknowns, skinning width) combination"); \
  } while (0)

// GENERAL path (kernels_gen.inc): the vertex block of the normal equations and the LBS / part-sum pass with run-time
// loops over the unknowns and the skinning weights
// the matrix-core form (k_gen_accum_mfma): (weighted, waves, blocks per wave, staged joint rows) -> instantiation
int launch_gen_accum_mfma(const DevModel& d, const Workspace& ws, int B, bool weighted, double* vextra, const float* tj,
                          const float* jw, hipStream_t st) {
  const size_t lds = gen2_lds(d.J, d.S, d.KW);
  if (lds > 160 * 1024) return fail(SMPLFIT_ERR_UNSUPPORTED, "general path: too many shape unknowns for the accumulate kernel's LDS tile");
  const bool stage = gen2_stage_joints(d.J, d.S, d.KW);
  const int nw = gen2_nw(d.S), nbw = gen2_nbw(d.S);
  const dim3 grid(B, gen2_groups(d.S));
  // blend passes (64 / 128 vertices) between two additions of the fp32 accumulators to the fp64 record: a scaled
  // iteration after every pass, the others after kGenFlushVertices (k_gen_accum_mfma; at S = 300 a flush every 2048
  // vertices cost +2.5 % of its time, every 1024 +5 %)
  const int flush_every = vextra ? 1 : std::max(1, kGenFlushVertices / gen2_sv(d.S));
#define SF_GEN2(W_, NW_, NBW_, ST_)                                                                                   \
  do {                                                                                                                \
    ensure_max_lds(reinterpret_cast<const void*>(&k_gen_accum_mfma<W_, NW_, NBW_, ST_>)); \
    hipLaunchKernelGGL((k_gen_accum_mfma<W_, NW_, NBW_, ST_>), grid, dim3(64 * NW_), lds, st, d, ws, B, vextra, flush_every, tj, jw); \
  } while (0)
#define SF_GEN2_W(NW_, NBW_, ST_)               \
  do {                                          \
    if (weighted) SF_GEN2(true, NW_, NBW_, ST_); \
    else SF_GEN2(false, NW_, NBW_, ST_);        \
  } while (0)
#define SF_GEN2_S(NW_, NBW_)              \
  do {                                    \
    if (stage) SF_GEN2_W(NW_, NBW_, true); \
    else SF_GEN2_W(NW_, NBW_, false);     \
  } while (0)
  if (nw == 4) SF_GEN2_S(4, 1);
  else if (nbw == 1) SF_GEN2_S(16, 1);
  else SF_GEN2_S(8, 7);
#undef SF_GEN2_S
#undef SF_GEN2_W
#undef SF_GEN2
  return 0;
}
// (general path, matrix-core accumulate: the target joints enter as rows of the vertex block's kernel instead of the
// joint block of k_joint_stage)
bool gen_joint_rows(const DevModel& d) { return d.general && tune().gen_mfma; }
int launch_gen_accum(const DevModel& d, const Workspace& ws, int B, bool weighted, hipStream_t st, const float* jrows_tj,
                     const float* jrows_jw, bool extras) {
  if (tune().gen_mfma) return launch_gen_accum_mfma(d, ws, B, weighted, extras ? ws.gvex : nullptr, jrows_tj, jrows_jw, st);
  const size_t lds = gen_accum_lds(d.J, d.S, d.KW);
  if (lds > 160 * 1024) return fail(SMPLFIT_ERR_UNSUPPORTED, "general path: too many shape unknowns for the accumulate kernel's LDS tile");
  const bool stage = gen_accum_stage_joints(d.J, d.S, d.KW);
  const int tv = gen_tile_vertices(d.S), nt = gen_accum_threads(d.S);
  const int flush_tiles = std::max(1, kGenFlushVertices / tv);
  // (weighted, vertices per tile, threads, staged joint rows) -> instantiation
#define SF_GEN(W_, TV_, NT_, ST_)                                                                              \
  do {                                                                                                         \
    ensure_max_lds(reinterpret_cast<const void*>(&k_gen_accum<W_, TV_, NT_, ST_>)); \
    hipLaunchKernelGGL((k_gen_accum<W_, TV_, NT_, ST_>), dim3(B), dim3(NT_), lds, st, d, ws, B, flush_tiles);  \
  } while (0)
#define SF_GEN_W(TV_, NT_, ST_)              \
  do {                                       \
    if (weighted) SF_GEN(true, TV_, NT_, ST_); \
    else SF_GEN(false, TV_, NT_, ST_);       \
  } while (0)
#define SF_GEN_S(TV_, NT_)            \
  do {                                \
    if (stage) SF_GEN_W(TV_, NT_, true); \
    else SF_GEN_W(TV_, NT_, false);   \
  } while (0)
  if (nt == 64) SF_GEN_S(32, 64);
  else if (tv == 32) SF_GEN_S(32, 256);
  else SF_GEN_S(8, 256);
#undef SF_GEN_S
#undef SF_GEN_W
#undef SF_GEN
  return 0;
}
template <int MODE>
void launch_gen_lbs(const DevModel& d, const Workspace& ws, int B, bool weighted, int nb, const float* beta,
                    const float* trans, float* out, hipStream_t st, const float* kid = nullptr) {
  const size_t lds = gen_lbs_lds(d.J, d.S, B);
  const int ni = gen_lbs_ni(d.S, B);
#define SF_GLBS(M_, W_)                                                                                                   \
  do {                                                                                                                    \
    if (ni == 4) {                                                                                                        \
      ensure_max_lds(reinterpret_cast<const void*>(&k_gen_lbs<M_, W_, 4>));   \
      hipLaunchKernelGGL((k_gen_lbs<M_, W_, 4>), dim3((B + 3) / 4), dim3(256), lds, st, d, ws, B, nb, beta, trans, kid, out); \
    } else {                                                                                                              \
      hipLaunchKernelGGL((k_gen_lbs<M_, W_, 1>), dim3(B), dim3(256), lds, st, d, ws, B, nb, beta, trans, kid, out);       \
    }                                                                                                                     \
  } while (0)
  if (weighted && MODE != 2) SF_GLBS((MODE == 2 ? 0 : MODE), true);
  else SF_GLBS(MODE, false);
#undef SF_GLBS
}
// the vertex block / the LBS pass of the wave-per-instance path OR the general one, by model
// jrows_tj / jrows_jw: the centred target joints (and their weights) when gen_joint_rows() moved the joint block here
// extras: also the extra sums of a scale unknown (general path: ws.gvex; the other paths run k_scale_extras)
// pair_form: Route::pair_in (wave-per-instance path)
int launch_accum_any(const DevModel& d, const Workspace& ws, int B, bool weighted, bool pair_form, hipStream_t st,
                     const float* jrows_tj = nullptr, const float* jrows_jw = nullptr, bool extras = false) {
  if (d.general) return launch_gen_accum(d, ws, B, weighted, st, jrows_tj, jrows_jw, extras);
#define SF_CALL_ACCUM(S_, KW_) launch_shape_accum<S_, KW_>(d, ws, B, weighted, pair_form, st)
  SF_DISPATCH_SKW(d, SF_CALL_ACCUM);
#undef SF_CALL_ACCUM
  return 0;
}
template <int MODE>
int launch_lbs_any(const DevModel& d, const Workspace& ws, int B, bool weighted, int nb, const float* beta,
                   const float* trans, float* out, hipStream_t st, const float* kid = nullptr) {
  if (d.general) {
    launch_gen_lbs<MODE>(d, ws, B, weighted, nb, beta, trans, out, st, kid);
    return 0;
  }
#define SF_CALL_LBS(S_, KW_) launch_lbs<S_, KW_, MODE, false>(d, ws, B, weighted, nb, beta, trans, out, 0.f, 0.f, st, kid)
  SF_DISPATCH_SKW(d, SF_CALL_LBS);
#undef SF_CALL_LBS
  return 0;
}

// Handle, batch and workspace of every entry point `who`.  needed: what the entry's workspace query `query` answers
// for this handle and batch (the queries answer 0 for a null handle or a batch <= 0, so they may be asked first).
// check_handle: the handle alone, for the entries without workspace whose empty batch is a call that enqueues nothing
// (smplfit_rototranslate_f32 and its backward).
int check_handle(const char* who, const smplfit_handle* h) {
  if (!h) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null handle");
  if (!h->has_device) return fail(SMPLFIT_ERR_HIP, std::string(who) + ": handle was created host-only (no device)");
  return 0;
}
int check_call(const char* who, const smplfit_handle* h, int batch, const void* workspace, size_t given, size_t needed,
               const char* query) {
  const auto bad = [who](int code, const std::string& what) { return fail(code, std::string(who) + ": " + what); };
  if (int rc = check_handle(who, h)) return rc;
  if (batch <= 0) return bad(SMPLFIT_ERR_BAD_ARG, "batch must be positive");
  if (!workspace || ((uintptr_t)workspace & 255))
    return bad(SMPLFIT_ERR_WORKSPACE, "workspace must be a 256-byte aligned device pointer");
  if (given < needed) return bad(SMPLFIT_ERR_WORKSPACE, std::string("workspace too small (see ") + query + ")");
  return 0;
}

// The scale / share options of a shape solve (smplfit_fit_ex_f32, smplfit_shape_solve_ex_f32)
int check_scale_share(const char* who, int scale_mode, const float* scale_corr, int share_beta,
                      smplfit_share_allreduce_fn share_allreduce) {
  if (scale_mode < 0 || scale_mode > 2)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": scale_mode must be 0, 1 (scale_target) or 2 (scale_fit)");
  if (scale_mode && !scale_corr) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": a scale option needs the scale_corr output");
  if (share_allreduce && !share_beta) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": share_allreduce without share_beta");
  return 0;
}

// The inputs of a forward evaluation as the argument structs of the forward, its backward and both objectives name
// them: one rotation form or none, (B, given) betas, the kid factor.  Read once per call (forward_inputs), checked
// (check_forward_inputs), and the kernels' argument structs are filled from them (forward_args here, JointBwdArgs in
// launch_forward_backward).
struct ForwardInputs {
  const float *pose, *glob, *rel, *betas, *kid;
  int given;
};
template <class A>
ForwardInputs forward_inputs(const A& a) {
  return {a.pose_rotvecs, a.glob_rotmats, a.rel_rotmats, a.shape_betas, a.kid_factor, a.num_betas_given};
}
int check_forward_inputs(const char* who, const DevModel& d, const ForwardInputs& in) {
  if ((in.pose != nullptr) + (in.glob != nullptr) + (in.rel != nullptr) > 1)
    return fail(SMPLFIT_ERR_BAD_ARG, "Only one rotation input may be provided");
  if (in.betas && in.given > d.S - d.jt.n_kid - d.jt.n_pad)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": more betas than the model holds; slice first");
  if (in.kid && !d.jt.n_kid) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": kid_factor given to a handle without kid");
  return 0;
}
// Betas per instance row.  The forward clamps to the model's; the backward family reads the rows as given
// (check_forward_inputs has refused more than the model holds).
int forward_nb(const DevModel& d, const ForwardInputs& in) {
  return in.betas ? std::min(in.given, d.S - d.jt.n_kid - d.jt.n_pad) : 0;
}
int backward_nb(const ForwardInputs& in) { return in.betas ? std::max(0, in.given) : 0; }
ForwardArgs forward_args(const ForwardInputs& in, int nb, const float* trans, float* joints, float* orient) {
  ForwardArgs fa{};
  fa.pose = in.pose;
  fa.glob = in.glob;
  fa.rel = in.rel;
  fa.betas = in.betas;
  fa.nb = nb;
  fa.kid = in.kid;
  fa.trans = trans;
  fa.joints = joints;
  fa.orient = orient;
  return fa;
}

// BodyModel.rototranslate (smplfit_rototranslate_f32 and its backward): the inputs both entries share, checked before
// anything is enqueued (the betas / kid rules are check_forward_inputs'), as the kernels' argument struct.
template <class A>
int rigid_inputs(const char* who, const smplfit_handle* h, const A& a, RigidInputs* out) {
  if (int rc = check_handle(who, h)) return rc;
  if (a.batch < 0) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": batch must not be negative");
  if (!a.R || !a.pose_rotvecs || !a.trans)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": R, pose_rotvecs and trans are required");
  const DevModel& d = h->d;
  const ForwardInputs in{a.pose_rotvecs, nullptr, nullptr, a.shape_betas, a.kid_factor, a.num_betas_given};
  if (int rc = check_forward_inputs(who, d, in)) return rc;
  RigidInputs r{};
  r.j_ext = d.jt.j_ext;
  r.S = d.S;
  r.J3 = 3 * d.J;
  r.R = a.R;
  r.R_stride = a.R_per_instance ? 9 : 0;
  r.t = a.t;
  r.t_stride = a.t_per_instance ? 3 : 0;
  r.pose = a.pose_rotvecs;
  r.betas = in.betas;
  r.nb = backward_nb(in);
  if (!r.nb) r.betas = nullptr;
  r.kid = in.kid;
  r.trans = a.trans;
  r.post = a.post_translate != 0;
  *out = r;
  return 0;
}

// Arithmetic of the posedirs contraction: "bf16x3" (default) runs it on the bf16 matrix cores with every fp32
// operand split error-free into bf16 terms (3 products per k-step + the bias row's third term, fp32 accumulate:
// fp32-class accuracy at the vertex level, see k_posedirs_gemm_bf16x3); "f32" (SMPLFIT_GEMM=f32) uses the fp32 MFMA,
// which on gfx950 shares the vector ALUs with ordinary VALU work.
bool gemm_bf16x3() { return !tune().gemm_f32; }

// Residency rounds of k_posedirs_gemm_bf16x3: its workgroups per CU (256 CUs) over a launch.  1 (default): 16 column
// chunks at B = 4096, every CU starts one workgroup; 2 (up to this round): 32 chunks, every workgroup start — tile
// request, features, first barrier — twice per CU.  A/B builds (-DSMPLFIT_GEMM_ROUNDS=2), measured alternating on one
// box with both front ends: profiles/README.md, profiles/gemm_planes_mi355x.json
#ifndef SMPLFIT_GEMM_ROUNDS
#define SMPLFIT_GEMM_ROUNDS 1
#endif
constexpr int kGemmRounds = SMPLFIT_GEMM_ROUNDS;

// GEMM launches on feature planes since the process started (smplfit_gemm_plane_launches: the route is not otherwise
// visible to a caller, and the results are the same bits either way)
std::atomic<uint64_t> g_gemm_plane_launches{0};

// The models k_posedirs_gemm_bf16x3 serves (route_of asks it for Route::gemm_planes)
bool gemm_bf16x3_stationary(const DevModel& d) { return d.Kp == 208 && gemm_bf16x3() && d.gemm_exclusive; }

// planes: Route::gemm_planes — the features are the split planes ws.rpP (k_prologue_bm wrote them, and not ws.rp)
int launch_gemm(const DevModel& d, const Workspace& ws, int B, hipStream_t st, bool transposed = false, bool planes = false) {
  const int Mp = (int)align_up((size_t)B, 128), N = 3 * d.Vp;
  if (planes && !(sf::kGemm3 && transposed && gemm_bf16x3_stationary(d)))
    return fail(SMPLFIT_ERR_UNSUPPORTED, "posedirs GEMM: no kernel reads feature planes on this route");
  if (gemm_bf16x3_stationary(d)) {
    // Workgroup = 8 waves x 32 instances = one whole CU (see k_posedirs_gemm_bf16x3).  XCD-aware tiling: block
    // id = y * nchunk + x runs on XCD id % 8, so with nchunk a multiple of 8 a tile chunk x lives on ONE XCD,
    // and with nchunk * ny ~ 256 kGemmRounds (one workgroup per CU) the instance blocks y of a chunk walk its tiles
    // together: the 39 KB tile images come out of that XCD's L2 and posedirs is fetched from HBM about twice
    // per launch instead of once per instance block (FETCH_SIZE: 444 -> 72 MB per launch at B = 4096).
    const int ntiles = N / 32, ny = (Mp + 32 * kGemmWaves - 1) / (32 * kGemmWaves);
    const int nchunk = std::min(std::max(8, (kGemmRounds * 256 / ny + 4) / 8 * 8), ntiles);
    const int per = (ntiles + nchunk - 1) / nchunk;  // trailing chunks may be empty (they return at once)
    const size_t lds = (size_t)kGemmRing * kGemmTileBytes;
    if constexpr (sf::kGemm3) {
      if (planes) {
        g_gemm_plane_launches.fetch_add(1, std::memory_order_relaxed);
        ensure_max_lds(reinterpret_cast<const void*>(&k_posedirs_gemm_bf16x3<true, true>));
        hipLaunchKernelGGL((k_posedirs_gemm_bf16x3<true, true>), dim3(nchunk, ny), dim3(64 * kGemmWaves), lds, st, ws.rp,
                           ws.rpP, d.pdB, ws.vpT, N, per, Mp);
        return 0;
      }
    }
    ensure_max_lds(reinterpret_cast<const void*>(&k_posedirs_gemm_bf16x3<true, false>));
    ensure_max_lds(reinterpret_cast<const void*>(&k_posedirs_gemm_bf16x3<false, false>));
    if (transposed)
      hipLaunchKernelGGL((k_posedirs_gemm_bf16x3<true, false>), dim3(nchunk, ny), dim3(64 * kGemmWaves), lds, st, ws.rp,
                         ws.rpP, d.pdB, ws.vpT, N, per, Mp);
    else
      hipLaunchKernelGGL((k_posedirs_gemm_bf16x3<false, false>), dim3(nchunk, ny), dim3(64 * kGemmWaves), lds, st, ws.rp,
                         ws.rpP, d.pdB, ws.vposed, N, per, Mp);
    return 0;
  }
  if (d.Kp != 208 && transposed && d.kc32 > 0 && gemm_bf16x3() && d.gemm_exclusive) {
    // tiled split-bf16 GEMM (SMPL-X): the feature images go to ws.vposed, which the batch-major path does not use
    const int mt = (Mp + 255) / 256, nt256 = N / 256;
    uint16_t* aimg = reinterpret_cast<uint16_t*>(ws.vposed);
    hipLaunchKernelGGL(k_split_features, dim3(mt, d.kc32), dim3(256), 0, st, ws.rp, aimg, Mp, d.Kp, d.kc32);
    ensure_max_lds(reinterpret_cast<const void*>(&k_posedirs_gemm_bf16x3_tiled));
    hipLaunchKernelGGL(k_posedirs_gemm_bf16x3_tiled, dim3(8 * ((mt + 7) / 8) * nt256), dim3(512), (size_t)2 * kTg2Stage, st,
                       aimg, d.pdB2, ws.vpT, N, Mp, mt, d.kc32, sf::rp_pos(d.P, d.Kp) / 16);
    return 0;
  }
  if (d.Kp == 208) {  // SMPL (J = 24): A-stationary kernel, 104 A registers per lane
    constexpr int NK2 = 104;
    const int ntiles = N / 32;
    // ~768 workgroups (measured faster than exactly one 512-workgroup residency wave)
    int nchunk = std::max(1, (3 * 256 + Mp / 128 - 1) / (Mp / 128));
    nchunk = std::min(nchunk, ntiles);
    const int per = (ntiles + nchunk - 1) / nchunk;
    nchunk = (ntiles + per - 1) / per;
    const size_t lds = (size_t)2 * 32 * (2 * NK2 + 4) * 4;
    if (transposed)
      hipLaunchKernelGGL((k_posedirs_gemm_as<NK2, true>), dim3(nchunk, Mp / 128), dim3(256), lds, st,
                         ws.rp, d.pdSw, ws.vpT, N, per, Mp);
    else
      hipLaunchKernelGGL((k_posedirs_gemm_as<NK2, false>), dim3(nchunk, Mp / 128), dim3(256), lds, st,
                         ws.rp, d.pdSw, ws.vposed, N, per, Mp);
    return 0;
  }
  if (transposed)
    hipLaunchKernelGGL(k_posedirs_gemm<true>, dim3((N / 128) * (Mp / 128)), dim3(256), 0, st, ws.rp, d.pdSw,
                       ws.vpT, Mp, N, d.Kp);
  else
    hipLaunchKernelGGL(k_posedirs_gemm<false>, dim3((N / 128) * (Mp / 128)), dim3(256), 0, st, ws.rp, d.pdSw,
                       ws.vposed, Mp, N, d.Kp);
  return 0;
}

// (general path: the S-sized parts of the scratch — P, T, the S x S system — live in the workspace, see gen_joint_scratch)
size_t joint_lds(const DevModel& d, int kind = 0) {
  return (size_t)sf::joint_scratch_floats(d.J, d.general ? 0 : d.S, kind) * 4;
}
// (general path: the stage's scratch is in global memory, LDS holds the panel of the blocked factorisation)
size_t solve_lds(const DevModel& d) {
  return d.general ? (size_t)(sf::kSolvePanel * d.S + sf::kSolvePanel) * 8 : (size_t)sf::solve_scratch_floats(d.S) * 4;
}

// The per-instance stages run two instances per wave (DevCtxHalf) when the model's joints fit 32 lanes and the batch
// fills the chip either way (below ~2 workgroups per CU the one-instance form is the faster one: B = 256 0.416 vs
// 0.403 M fits/s; B = 4096 2.55 -> 2.59, 32768 2.68 -> 2.70).  A half-wave sum adds lanes 0-31 in the order the
// wave sum does; loops longer than 32 split differently (tests/test_gpu_parity.py::test_stage_half runs both forms).
// SMPLFIT_STAGE_HALF (compile time) masks it per stage: 1 joint stage, 2 solve, 4 refinement.
#ifndef SMPLFIT_STAGE_HALF
#define SMPLFIT_STAGE_HALF 7
#endif
inline bool stage_half(const DevModel& d, int bit, int B) {
  return (SMPLFIT_STAGE_HALF & bit) && d.J <= 32 && B >= tune().stage_half_b && !d.general;
}

void launch_forward_joint(const DevModel& d, const ForwardArgs& fa, const Workspace& ws, int B, hipStream_t st) {
  if (d.general) hipLaunchKernelGGL(k_forward_joint<true>, dim3(B), dim3(64), joint_lds(d), st, d, fa, ws);
  else hipLaunchKernelGGL(k_forward_joint<false>, dim3(B), dim3(64), joint_lds(d), st, d, fa, ws);
}
void launch_joint_stage(const DevModel& d, JointStageArgs ja, const Workspace& ws, int B, hipStream_t st) {
  ja.B = B;
  ja.b0 = 0;
  count_stage(SMPLFIT_STAGE_JOINT_STAGE);
  if (stage_half(d, 1, B)) {
    if (B / 2 > 0) hipLaunchKernelGGL(k_joint_stage<32>, dim3(B / 2), dim3(64), 2 * joint_lds(d), st, d, ja, ws);
    if (B & 1) {  // the odd last instance: a launch of its own (no wave works on one instance twice)
      ja.b0 = B - 1;
      hipLaunchKernelGGL(k_joint_stage<64>, dim3(1), dim3(64), joint_lds(d), st, d, ja, ws);
    }
  } else {
    if (d.general) hipLaunchKernelGGL((k_joint_stage<64, true>), dim3(B), dim3(64), joint_lds(d), st, d, ja, ws);
    else hipLaunchKernelGGL(k_joint_stage<64>, dim3(B), dim3(64), joint_lds(d), st, d, ja, ws);
  }
}
void launch_refine(const DevModel& d, RefineArgs ra, const Workspace& ws, int B, hipStream_t st) {
  ra.B = B;
  ra.b0 = 0;
  count_stage(SMPLFIT_STAGE_REFINE_EPILOGUE);
  if (stage_half(d, 4, B)) {
    if (B / 2 > 0) hipLaunchKernelGGL(k_refine_epilogue<32>, dim3(B / 2), dim3(64), 2 * joint_lds(d, 1), st, d, ra, ws);
    if (B & 1) {
      ra.b0 = B - 1;
      hipLaunchKernelGGL(k_refine_epilogue<64>, dim3(1), dim3(64), joint_lds(d, 1), st, d, ra, ws);
    }
  } else {
    hipLaunchKernelGGL(k_refine_epilogue<64>, dim3(B), dim3(64), joint_lds(d, 1), st, d, ra, ws);
  }
}
// first / count / cen_b0: a sub-range of the batch (general path: the chunks of a share_beta solve, see share_sum); the
// other paths always launch the whole batch
void launch_shape_solve(const DevModel& d, const Workspace& ws, int B, hipStream_t st, float beta_reg, float beta_reg2,
                        float kid_reg, int pair_form, int use_ref, int mode = 0, int first = 0, int count = -1,
                        int cen_b0 = 0, const int32_t* row_seg = nullptr) {
  if (count < 0) count = B;
  count_stage(SMPLFIT_STAGE_SHAPE_SOLVE);
  if (d.general) {
    ensure_max_lds(reinterpret_cast<const void*>(&k_shape_solve<64, true>));
    hipLaunchKernelGGL((k_shape_solve<64, true>), dim3(count), dim3(d.S > 128 ? 1024 : d.S > 64 ? 256 : 64), solve_lds(d), st, d,
                       ws, B, beta_reg, beta_reg2, kid_reg, pair_form, use_ref, mode, first, cen_b0, row_seg);
  } else if (stage_half(d, 2, B)) {
    if (B / 2 > 0)
      hipLaunchKernelGGL(k_shape_solve<32>, dim3(B / 2), dim3(64), 2 * solve_lds(d), st, d, ws, B, beta_reg,
                         beta_reg2, kid_reg, pair_form, use_ref, mode, 0, 0, row_seg);
    if (B & 1)
      hipLaunchKernelGGL(k_shape_solve<64>, dim3(1), dim3(64), solve_lds(d), st, d, ws, B, beta_reg, beta_reg2,
                         kid_reg, pair_form, use_ref, mode, B - 1, 0, row_seg);
  } else {
    hipLaunchKernelGGL(k_shape_solve<64>, dim3(B), dim3(64), solve_lds(d), st, d, ws, B, beta_reg, beta_reg2,
                       kid_reg, pair_form, use_ref, mode, 0, 0, row_seg);
  }
}

// K4' (k_solve_bm): the normal-equation combine and the shape solve of the batch-major path as one launch, lane =
// instance.  Applies to the plain per-instance solve on the sums of k_residual_bm + k_pair_gram_bm (unit vertex weights
// in the solve, no share_beta, no scale unknown) for 10 / 11 shape unknowns; everything else keeps k_gram_combine_bm +
// k_shape_solve (route_of).
constexpr int kSolveIB = 16;
// what k_solve_bm needs beyond the model: the longest run of moment rows of a joint in the residual table of this batch
// (rounded up to 8), the sizes of its three buffers (their descriptors take byte offsets below 2^31)
struct SolveBmPlan {
  bool ok = false;
  SolveBmArgs a{};
  ShareView sv{};
  size_t lds = 0;
};
SolveBmPlan solve_bm_plan(const smplfit_handle* h, int B) {
  SolveBmPlan p;
  const DevModel& d = h->d;
  if (d.general || !(d.S == 10 || d.S == 11) || !d.bm_tables) return p;
  const int idx = share_index(sf::kShareResidual, B);
  if (idx >= sf::kShareFine || (size_t)idx >= h->views.size()) return p;  // (small batches: the fine cell tables keep k_gram_combine_split + k_shape_solve)
  const sf::ShareTable& t = h->t.shares[idx];
  const int maxn = h->views[idx].aux_pitch;
  const size_t Mp = align_up((size_t)B, 128);
  const size_t res_rows = (size_t)t.ncells * ((d.S + 3 + 3) / 4 * 4) + (size_t)t.nrows * 3 * sf::kGroupJoints;
  const size_t res_bytes = res_rows * Mp * 4;
  const size_t gram_bytes = (size_t)pair_gram_workgroups(d.J, d.jt.np) * sf::ne_ng(d.S) * Mp * 4;
  const size_t jdt_bytes = Mp * align_up((size_t)d.J * sf::jd_stride(d.S), 64) * 4;
  int lg = 0;
  while ((8 << lg) < t.ncells) ++lg;
  if (maxn > kSolveT3 || (8 << lg) != t.ncells || res_bytes >= (1u << 31) || gram_bytes >= (1u << 31) || jdt_bytes >= (1u << 31) ||
      !h->views[idx].aux_pad)
    return p;
  p.sv = share_view(h, sf::kShareResidual, B);
  const bool stage_px = solve_bm_lds_bytes(d.S, kSolveIB, d.J, t.ncells, maxn, true) <= 156 * 1024;
  p.lds = solve_bm_lds_bytes(d.S, kSolveIB, d.J, t.ncells, maxn, stage_px);
  if (p.lds > 156 * 1024) return p;
  p.a.stage_px = stage_px ? 1 : 0;
  p.a.maxn = maxn;
  p.a.lg_ngrp = lg;
  p.a.res_bytes = (uint32_t)res_bytes;
  p.a.gram_bytes = (uint32_t)gram_bytes;
  p.a.jdt_bytes = (uint32_t)jdt_bytes;
  p.ok = true;
  return p;
}
template <int S>
void launch_solve_bm_s(const smplfit_handle* h, const Workspace& ws, int B, hipStream_t st, SolveBmPlan p) {
  const DevModel& d = h->d;
  const int Mp = (int)align_up((size_t)B, 128);
  const int groups = (int)align_up((size_t)Mp / kSolveIB, 32);
  count_stage(SMPLFIT_STAGE_SOLVE_BM);
  if (p.lds > 64 * 1024) ensure_max_lds(reinterpret_cast<const void*>(&k_solve_bm<S, kSolveIB>));
  hipLaunchKernelGGL((k_solve_bm<S, kSolveIB>), dim3(groups), dim3(64 * kSolveWaves), p.lds, st, d, p.sv, ws, B, Mp, p.a);
}
// p: Route::solve_plan.  pro: the joint block and the FK rows come from k_prologue_bm (ws.gramjP, ws.pextT) instead of
// k_joint_stage
void launch_solve_bm(const smplfit_handle* h, SolveBmPlan p, const Workspace& ws, int B, hipStream_t st, float beta_reg,
                     float beta_reg2, float kid_reg, int use_ref, bool pro) {
  p.a.gj_parts = pro ? prologue_splits(h->d.J) : 0;
  p.a.pext_t = pro ? 1 : 0;
  p.a.beta_reg = beta_reg;
  p.a.beta_reg2 = beta_reg2;
  p.a.kid_reg = kid_reg;
  p.a.use_ref = use_ref;
  if (h->d.S == 11) launch_solve_bm_s<11>(h, ws, B, st, p);
  else launch_solve_bm_s<10>(h, ws, B, st, p);
}

// K1p (k_prologue_bm): the shape prologue of the joint stage on the batch-major path — k_joint_stage then fits the
// rotations only and leaves ws.GT.  Applies when every shape solve of the call is k_solve_bm (the one consumer of its
// ws.gramjP / ws.pextT): route_of.
void launch_prologue_bm(const smplfit_handle* h, const JointStageArgs& ja, const Workspace& ws, int B, hipStream_t st,
                        bool planes) {
  const DevModel& d = h->d;
  const int Mp = (int)align_up((size_t)B, 128);
  PrologueArgs pa{ja.tj, ja.jw, ja.joint_block, ja.joint_block_weighted, ja.vertex_sa_closed_form, B, planes ? 1 : 0};
  const size_t lds = (size_t)(kProWaves / 2) * (sf::ne_size(d.S) + 1) * 64 * 4;
  const dim3 grid(Mp / 64, prologue_splits(d.J));
  count_stage(d.S == 11 ? SMPLFIT_STAGE_PROLOGUE_BM_S11 : SMPLFIT_STAGE_PROLOGUE_BM_S10);
  if (d.S == 11) {
    if (lds > 64 * 1024) ensure_max_lds(reinterpret_cast<const void*>(&k_prologue_bm<11>));
    hipLaunchKernelGGL(k_prologue_bm<11>, grid, dim3(64 * kProWaves), lds, st, d, pa, ws, Mp);
  } else {
    if (lds > 64 * 1024) ensure_max_lds(reinterpret_cast<const void*>(&k_prologue_bm<10>));
    hipLaunchKernelGGL(k_prologue_bm<10>, grid, dim3(64 * kProWaves), lds, st, d, pa, ws, Mp);
  }
}
// the joint stage of a fit on the batch-major path: rotations by k_joint_stage, the prologue by k_prologue_bm (pro), or
// both by k_joint_stage
// K1r (k_rotations_bm): the part rotations with lane = instance, adding the part-sum rows of the pass in front of it
// itself.  rot_kind: the cell table of that pass (its rows), or -1: k_joint_stage fits the rotations.  gprev_mode: where
// the previous rotations come from (0 none, 1 ws.GT, 2 the instance-major ja.Gprev).
// spread: Route::rot_spread, the form with a joint per wave (k_rotations_spread; it has no use for RotArgs::slot); it
// counts under the stage id of the kernel it replaces, and in g_rot_spread_launches.
std::atomic<uint64_t> g_rot_spread_launches{0};
void launch_rotations_bm(const smplfit_handle* h, const JointStageArgs& ja, int rot_kind, int gprev_mode, const Workspace& ws, int B,
                         hipStream_t st, bool spread) {
  const DevModel& d = h->d;
  const int Mp = (int)align_up((size_t)B, 128);
  RotArgs ra{ja.tj, ja.rj, ja.jw, ja.Gprev, ja.rj_shared, gprev_mode, B, {}};
  if (spread) {
    const size_t lds = (size_t)rot_spread_lds_floats(d.J) * 4;
    count_stage(d.J <= kRotJoints * kRefWaves ? SMPLFIT_STAGE_ROTATIONS_BM : SMPLFIT_STAGE_ROTATIONS_BM_ROUNDS);
    g_rot_spread_launches.fetch_add(1, std::memory_order_relaxed);
    if (lds > 64 * 1024) ensure_max_lds(reinterpret_cast<const void*>(&k_rotations_spread));
    hipLaunchKernelGGL(k_rotations_spread, dim3((B + 63) / 64, (d.J + kRefWaves - 1) / kRefWaves), dim3(64 * kRefWaves), lds, st, d, ra,
                       share_view(h, rot_kind, B), ws, Mp);
    return;
  }
  static_assert(sizeof(ra.slot) == sizeof(h->t.rot_slots), "RotArgs::slot holds HostTables::rot_slots");
  std::memcpy(ra.slot, h->t.rot_slots, sizeof(ra.slot));
  const size_t lds = (size_t)rot_bm_lds_floats(d.J) * 4;
  count_stage(d.J <= kRotJoints * kRefWaves ? SMPLFIT_STAGE_ROTATIONS_BM : SMPLFIT_STAGE_ROTATIONS_BM_ROUNDS);
  if (d.J <= kRotJoints * kRefWaves) {
    if (lds > 64 * 1024) ensure_max_lds(reinterpret_cast<const void*>(&k_rotations_bm));
    hipLaunchKernelGGL(k_rotations_bm, dim3((B + 63) / 64), dim3(64 * kRefWaves), lds, st, d, ra, share_view(h, rot_kind, B), ws, Mp);
  } else {
    if (lds > 64 * 1024) ensure_max_lds(reinterpret_cast<const void*>(&k_rotations_bm_rounds));
    hipLaunchKernelGGL(k_rotations_bm_rounds, dim3((B + 63) / 64), dim3(64 * kRefWaves), lds, st, d, ra, share_view(h, rot_kind, B), ws, Mp);
  }
}
// planes: Route::gemm_planes (with pro)
void launch_joint_stage_fit(const smplfit_handle* h, JointStageArgs ja, const Workspace& ws, int B, hipStream_t st, bool pro,
                            int rot_kind = -1, int gprev_mode = 0, bool planes = false, bool rot_spread = false) {
  if (pro && ja.do_prologue) {
    if (rot_kind >= 0) {
      launch_rotations_bm(h, ja, rot_kind, gprev_mode, ws, B, st, rot_spread);
    } else {
      ja.do_prologue = 0;
      ja.gt_pitch = (int)align_up((size_t)B, 128);
      launch_joint_stage(h->d, ja, ws, B, st);
      ja.do_prologue = 1;
    }
    launch_prologue_bm(h, ja, ws, B, st, planes);
  } else {
    launch_joint_stage(h->d, ja, ws, B, st);
  }
}

// K6' (k_refine_bm): the refinement + epilogue with lane = instance, reading the part-sum rows of the last LBS pass
// itself.  Applies where k_prologue_bm ran (pro: ws.GT holds the rotations of the last joint stage, coarse cell tables)
// on models whose joint arrays of 64 instances fit the LDS (at most 32 joints).
// sv: the table of the LBS pass whose rows hold the part sums (unused without final_adjust)
void launch_refine_bm(const smplfit_handle* h, RefineArgs ra, const ShareView& sv, const Workspace& ws, int B, hipStream_t st) {
  const DevModel& d = h->d;
  const int Mp = (int)align_up((size_t)B, 128);
  ra.B = B;
  ra.b0 = 0;
  RefGroups rg;
  std::memcpy(rg.wave, h->t.refine_waves, sizeof(rg.wave));
  const size_t lds = (size_t)refine_bm_lds_floats(d.J) * 4;
  count_stage(SMPLFIT_STAGE_REFINE_BM);
  if (d.S == 11) {
    if (lds > 64 * 1024) ensure_max_lds(reinterpret_cast<const void*>(&k_refine_bm<11>));
    hipLaunchKernelGGL(k_refine_bm<11>, dim3((B + 63) / 64), dim3(64 * kRefWaves), lds, st, d, ra, sv, ws, ws.rjoints, Mp, rg);
  } else {
    if (lds > 64 * 1024) ensure_max_lds(reinterpret_cast<const void*>(&k_refine_bm<10>));
    hipLaunchKernelGGL(k_refine_bm<10>, dim3((B + 63) / 64), dim3(64 * kRefWaves), lds, st, d, ra, sv, ws, ws.rjoints, Mp, rg);
  }
}

// ------------------------------------------------------------------------------------------------
// Kernel route of one call: which kernel family serves its vertex passes and which stage kernels run inside the
// batch-major one, decided once per call by route_of() from the handle, the batch and the call's shape (a fit call cut
// into concurrent chunks: once per chunk, from the chunk's batch; the one rule about what runs side by side on the
// chip, the batch limit of k_rotations_spread, counts the instances of the whole call, CallShape::call_batch).  Nothing
// else reads the routing switches (SMPLFIT_BM, SMPLFIT_BM_*, _ROT_BM, _ROT_SPREAD, _ROT_SPREAD_B, _REFINE_BM, _PROLOGUE_BM,
// _SOLVE_BM, _GEMM_PLANES, _SHAPE_FORM).
//
//   condition                                                      -> kernels
//   <= 8 skinning weights summing to one, 10 / 16 betas +- kid,      -> bm: the batch-major vertex passes; otherwise
//     >= 1024 vertices; not rotations_only; per entry BM_KNOWN_POSE,    the wave-per-instance (or general) kernels
//     BM_FORWARD, BM_KNOWN_SHAPE; vertex weights: BM_WEIGHTED; scale
//     unknown: BM_SCALE; either in the solve: 10 betas, 4 weights
//   bm, no weights in the solve, no share_beta, 10 / 11 unknowns,   -> unscaled solves: k_solve_bm on the partial sums;
//     coarse tables, buffers < 2 GB (solve_bm_plan); SOLVE_BM           else k_gram_combine_bm + k_shape_solve
//   a fit with k_solve_bm, no scale unknown; PROLOGUE_BM             -> k_prologue_bm, which writes ws.jdT: no k_jd_transpose
//   k_prologue_bm, Kp == 208, split-bf16 GEMM on an exclusive CU,     -> gemm_planes: k_prologue_bm writes the features as bf16
//     three products; GEMM_PLANES                                      planes, not as fp32 rows; the GEMM of a shape solve
//                                                                      reads those
//   k_prologue_bm, <= 64 joints; ROT_BM                              -> calls of up to 4096 instances (ROT_SPREAD_B; not with
//                                                                      ROT_SPREAD=0): k_rotations_spread, a joint per
//                                                                      wave; else, where the toe sources fit,
//                                                                      k_rotations_bm / _rounds: no k_psum_combine behind
//                                                                      the passes in front of a rotation pass
//   k_prologue_bm, <= 32 joints, <= 4 adjustable parts a wave; REFINE_BM -> k_refine_bm: no k_psum_combine behind the last
//                                                                      pass; else k_refine_epilogue (+ k_gt_to_g first
//                                                                      when k_rotations_bm ran)
//   no weights in the solve, not general; bm or SHAPE_FORM=pair      -> pair-Gram form (not the scaled solve of bm)
//   forward backward (smplfit_forward_backward_f32)                -> never bm: the instance-major kernels of
//                                                                      kernels_bwd.inc serve every model
//   flip (smplfit_flip_f32): the conversion's entry (kConvert, no    -> bm as a conversion; k_naive_flip, then the source
//     target joints) with warm = true; not bm: no fused call           of the conversion with k_transfer_bm<true> and
//                                                                      no k_template_partsum_bm (the first rotation pass
//                                                                      reads the warm start's LBS rows, kShareLbsAll)
// The route is applied by the STEPS below (launch_targets_in, launch_posed_pass / launch_lbs_pass,
// launch_normal_equations, launch_alignment: bm, general, jd_transpose, psum_combine*, pair_in, solve_bm's residual form),
// by enqueue_solve (solve_bm, pair_in*) and by the stage launches of run_fit (prologue_bm, rot_*, refine_*, gt_to_g).
// ------------------------------------------------------------------------------------------------
enum class Entry { kFit, kConvert, kShapeSolve, kForward, kKnownShape, kForwardBackward };
struct CallShape {
  Entry entry = Entry::kFit;
  bool joints = true;                // target joints given
  bool vw = false, eff_v = false;    // vertex weights given; they enter the shape solve
  int scale_mode = 0;
  bool share_beta = false, rotations_only = false;
  bool warm = false;                 // warm start: the first rotation pass reads the rows of the warm start's LBS pass
  int call_batch = 0;                // a chunk of a fit call: the instances of all its chunks, which run side by side (0: B)
};
struct Route {
  bool bm = false;                   // batch-major vertex kernels
  bool solve_bm = false;             // unscaled, unshared solves are k_solve_bm (on solve_plan)
  SolveBmPlan solve_plan{};
  bool prologue_bm = false;          // k_prologue_bm
  bool gemm_planes = false;          // k_prologue_bm writes the features as split-bf16 planes (ws.rpP) instead of ws.rp
                                     // and the GEMMs behind it (launch_normal_equations) read those
  bool jd_transpose = false;         // k_jd_transpose in front of a fit iteration's vertex passes
  bool rot_bm = false;               // k_rotations_bm, on the rows of the tables rot_kind_first / _next (else -1)
  bool rot_spread = false;           // ... as k_rotations_spread (a joint per wave) instead of k_rotations_bm / _rounds
  int rot_kind_first = -1, rot_kind_next = -1;
  bool refine_bm = false;            // k_refine_bm on the rows of the table refine_kind (else -1); else k_refine_epilogue
  int refine_kind = -1;
  bool gt_to_g = false;              // k_gt_to_g in front of k_refine_epilogue
  bool psum_combine = true, psum_combine_last = true;  // k_psum_combine behind the passes in front of a rotation pass / the last
  int pair_in = 0, pair_in_scaled = 0;  // the unscaled / the scaled solve reads the pair-Gram form
};
Route route_of(const smplfit_handle* h, int B, const CallShape& c) {
  const Tuning& tn = tune();
  const DevModel& d = h->d;
  Route r;
  // Vp > V: the batch-major loops run their out-of-range steps on the first padding slot; small vertex subsets are faster
  // on the wave-per-instance kernels (V = 1024, B = 16384: 4.15 M fits/s batch-major vs 4.63 M).  The residual kernel
  // derives sum_v b_v from the per-joint moments: exact only when every vertex's skinning weights sum to one (wsum_dev).
  const bool model_bm = tn.bm && (d.KW == 4 || d.KW == 8) && sf::bm_shape_count(d.S) && d.bm_tables && d.V >= 1024 &&
                        d.Vp > d.V && h->t.wsum_dev <= 1e-5f;
  const bool accum_w = d.S == 10 && d.KW == 4;  // what k_accum_w_bm is built for
  if (c.entry == Entry::kForwardBackward) return r;
  const bool solves = c.entry != Entry::kForward && c.entry != Entry::kKnownShape;
  if (c.entry == Entry::kForward) r.bm = model_bm && tn.bm_forward;
  else if (c.entry == Entry::kKnownShape) r.bm = model_bm && (!c.vw || tn.bm_weighted) && tn.bm_known_shape;
  else r.bm = model_bm && !c.rotations_only && (c.entry != Entry::kShapeSolve || tn.bm_known_pose) &&
              (!c.vw || (tn.bm_weighted && (!c.eff_v || accum_w))) && (!c.scale_mode || (tn.bm_scale && accum_w));
  if (solves && r.bm && !c.eff_v && !c.share_beta && tn.solve_bm) {
    r.solve_plan = solve_bm_plan(h, B);
    r.solve_bm = r.solve_plan.ok;
  }
  const bool fit = c.entry == Entry::kFit || c.entry == Entry::kConvert;
  r.prologue_bm = fit && r.solve_bm && !c.scale_mode && tn.prologue_bm;
  r.gemm_planes = r.prologue_bm && tn.gemm_planes && sf::kGemm3 && gemm_bf16x3_stationary(d) && 12 * d.Vp >= sf::kPlaneGroupBytes / 32;
  r.jd_transpose = r.bm && !r.prologue_bm;
  // (once k_rotations_bm runs nothing writes the instance-major ws.G any more: a model whose refinement stays on
  // k_refine_epilogue — more than 32 joints — gets it from k_gt_to_g in front of that kernel)
  // (k_rotations_spread needs the joints of 64 instances in LDS and nothing of the toes; the two kernels it replaces
  // also the toe sources in their LDS slots and at most two toes a wave)
  // The spread form for calls of up to kRotSpreadMaxBatch = 4096 instances, all chunks of the call counted since they
  // run side by side (64 blocks of 64: the block form's grid leaves three quarters of the 256 CUs idle).  Its workgroups
  // hold one per CU by their registers; with more blocks they queue behind each other while the block form's grid
  // fills the chip by itself.  Measured (profiles/rot_spread_mi355x.json): a gain at 4096 on both models, none at 8192
  // (the ranges overlap), none at 16384 (0.3 - 0.4 % below the parent, which is also what c4 moves between runs of one
  // build): where no gain was seen the parent's kernels stay.
  const bool spread = tn.rot_spread && std::max(B, c.call_batch) <= tn.rot_spread_b;
  const bool rot_fits = spread ? (size_t)rot_spread_lds_floats(d.J) * 4 <= 160 * 1024
                               : h->t.rot_nslots <= kRotSlots && h->t.rot_toes_per_wave <= 2 &&
                                     (size_t)rot_bm_lds_floats(d.J) * 4 <= 160 * 1024;
  r.rot_bm = r.prologue_bm && tn.rot_bm && d.J <= kRotMaxJ && rot_fits;
  r.rot_spread = r.rot_bm && spread;
  r.refine_bm = r.prologue_bm && tn.refine_bm && d.J <= 32 && h->t.refine_group_max <= kRefParts &&
                (size_t)refine_bm_lds_floats(d.J) * 4 <= 160 * 1024;
  r.gt_to_g = r.rot_bm && !r.refine_bm;
  r.psum_combine = !r.rot_bm;
  r.psum_combine_last = !r.refine_bm;
  // the tables of the passes in front (launch_lbs_bm): without target joints every slot, else the used parts — the
  // last pass of a fit with target joints the adjustable ones
  r.rot_kind_first = !r.rot_bm ? -1 : c.warm && !c.joints ? sf::kShareLbsAll : sf::kShareLbsUsed;
  r.rot_kind_next = !r.rot_bm ? -1 : !c.joints ? sf::kShareLbsAll : sf::kShareLbsUsed;
  r.refine_kind = !r.refine_bm ? -1 : !c.joints ? sf::kShareLbsAll : sf::kShareLbsAdj;
  // (weights in the solve, and the scaled solve of the bm path: the accumulate kernel leaves the complete record)
  r.pair_in = (!c.eff_v && !d.general && (r.bm || tn.pair_form)) ? 1 : 0;
  r.pair_in_scaled = (!c.eff_v && !d.general && !r.bm && tn.pair_form) ? 1 : 0;
  return r;
}

int post_launch_check() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(SMPLFIT_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// STEPS.  The launch sequences the entry points are made of.  Each is written once and is the one place that applies
// the route (Route::bm, DevModel::general) to its sequence; the drivers below only put them in order.
//   launch_targets_in         targets (+ weights) into the workspace, their mean, first part sums, regressed target joints
//   launch_posed_pass         the model at the current parameters: forward joint stage, GEMM, joint-row transpose, then
//   launch_lbs_pass           the LBS pass: part sums against the targets / the mesh alone (also to the caller: mesh out)
//   launch_mesh_error         the model at forward inputs against the caller's targets: mesh, joints and the distance of
//                             every vertex and joint to its target, any subset
//   launch_normal_equations   GEMM, joint-row transpose, the vertex block of one shape solve
//   launch_alignment          scale and translation of a known-shape fit
//   launch_forward_backward   the forward's vector-Jacobian product (below, behind the layouts it runs in)
//   RotationSweep             what the adjoints of both differentiable fits share: centring, part sums, rotation passes and
//                             their adjoints, output stage, vertex pass, mesh cotangent (below, behind its layout)
// and the rules that fill their arguments: solve_weights, set_joint_block, refine_args; in the sweep against_mesh /
// against_template (the reference joints of a stage) and rot_adjoint (which of Gbar / Gbar2 is current).
// ------------------------------------------------------------------------------------------------

// Which weights enter the shape solve and the alignment: both kinds only if both are given (with target joints), the
// vertex weights alone without target joints (bodyfitter.py:1018-1028, :1640-1661)
struct SolveWeights {
  bool v, j;
};
SolveWeights solve_weights(bool joints, const float* vw, const float* jw) {
  return {joints ? (vw && jw) : (vw != nullptr), joints && vw && jw};
}

// the joint block of the normal equations as the joint stage (or k_prologue_bm) takes it
void set_joint_block(JointStageArgs* ja, const DevModel& d, bool joints, SolveWeights w) {
  const bool gjr = gen_joint_rows(d) && joints;  // (the joints are rows of the vertex block: launch_normal_equations)
  ja->joint_block = (joints && !gjr) ? 1 : 0;
  ja->joint_block_weighted = w.j ? 1 : 0;
  ja->vertex_sa_closed_form = (w.v || d.general) ? 0 : 1;  // (the general accumulate sums SA itself)
}

// the refinement + epilogue of a fit: the joints it aligns and the caller's outputs (betas / kid: null for a known shape)
RefineArgs refine_args(const float* tj_rot, bool joints, const float* jw, int final_adjust, const Workspace& ws, float* pose,
                       float* betas, float* trans, float* kid, float* orient, float* rel) {
  RefineArgs ra{};
  ra.tj = tj_rot;
  ra.rj_term = joints ? ws.rjoints : ws.rjreg;
  ra.jw = jw;
  ra.final_adjust = final_adjust;
  ra.pose = pose;
  ra.betas = betas;
  ra.trans = trans;
  ra.kid = kid;
  ra.orient = orient;
  ra.rel = rel;
  return ra;
}

struct ConvertSource {
  const smplfit_convert_plan* plan;
  const float *pose, *betas, *trans;  // this chunk's rows of the input parameters; betas (B, nb) / trans may be null
  const float* kid;                   // (B) kid factor of the input mesh (the flip) or null (the conversion: none)
  int nb;
  Workspace wsi;  // forward-only workspace slice of the input model (carve(..., fwd_only))
};
int launch_convert_source(const ConvertSource& src, const Workspace& ws, int B, hipStream_t st);

// STEP targets in.  The targets of a call in the form its route reads: centred and sorted by part (ws.tvs, ws.vws; the
// template part sums come with them), or the batch-major streams (ws.tT, ws.wT) with their mean and — template_sums —
// the template part sums behind them; regress: the target joints regressed from the centred vertices when none are
// given (bodyfitter.py:1342-1344).  The joints the rotation stage then reads: rotation_targets().
struct TargetsIn {
  const float *tv, *tj;                  // (B,V,3); (B,J,3) or null
  const float* vw;                       // (B,V) or null
  const float* vw_stream;                // what the batch-major kernels of the call read of them: vw, or null where they
                                         // take no part sums and the weights do not enter the solve
  const ConvertSource* source = nullptr; // fused conversion: the third producer of the batch-major streams, instead of tv
  bool template_sums = false;            // (a warm-started fit takes its first part sums against the posed initial model)
  bool regress = false;
  bool vw_shared = false;                // vw is ONE (V) row every instance reads (smplfit_replace_hands_f32), not (B,V)
};
const float* rotation_targets(const Workspace& ws, bool joints) { return joints ? ws.tjc : ws.tjreg; }
int launch_targets_in(const smplfit_handle* h, const Route& r, const TargetsIn& t, const Workspace& ws, int B, hipStream_t st) {
  const DevModel& d = h->d;
  if (t.regress && !t.tj && !h->t.has_regressor)
    return fail(SMPLFIT_ERR_BAD_ARG, "target_joints omitted but the model has no J_regressor_post_lbs over its vertices");
  if (!r.bm) {
    launch_center_sort(d, t.tv, t.tj, t.vw, ws, B, st, t.vw_shared);
    if (t.regress && !t.tj) hipLaunchKernelGGL(k_regress_joints, dim3(B), dim3(64), 0, st, d, ws.tvs, ws.tjreg);
    return 0;
  }
  const int Mp = (int)align_up((size_t)B, 128);
  int nslab;  // ws.resP holds the slab sums of either producer
  if (t.source) {
    if (int rc = launch_convert_source(*t.source, ws, B, st)) return rc;
    nslab = t.source->plan->nslab;
  } else {
    nslab = launch_layout_bm(d, t.tv, t.vw_stream, ws, B, st, t.vw_shared);
  }
  hipLaunchKernelGGL(k_mean_finish, dim3(Mp / 64), dim3(64 * kMeanWaves), 0, st, d, t.tj, ws.resP, ws, B, Mp, nslab);
  if (t.template_sums) launch_template_partsum_bm(h, ws, B, st, t.vw_stream != nullptr, r.psum_combine);
  if (t.regress && !t.tj)
    hipLaunchKernelGGL(k_regress_joints_bm<true>, dim3(Mp / 64, d.J), dim3(64), 0, st, d, ws.tT, ws.mean, ws.tjreg, B);
  return 0;
}

// STEP LBS pass.  The mesh at the shape, translation and joint rows in the workspace, in one of two forms.
//   kPartSums  the part sums of the next rotation pass (or of the refinement) against the targets; without target joints
//              also the reference joints regressed from the posed mesh (ws.rjreg)
//   kForward   the mesh alone: to the caller's (B, V, 3) — mesh out —, or left in ws.vpT (batch-major only)
enum class Lbs { kNone, kPartSums, kForward };
struct LbsPass {
  Lbs form = Lbs::kNone;
  // kPartSums
  bool joints = true;         // target joints given
  bool weighted = false;      // vertex weights enter the part sums
  bool keep_mesh = false;     // the posed mesh stays in the workspace: the wave-per-instance pass in its MODE 1 (ws.rverts);
                              // the batch-major pass writes it (ws.vpT) only where it is read: regressed joints, mesh_all
  bool mesh_all = false;      // every posed vertex is read behind the pass (the alignment sums of a known-shape fit)
  bool feeds_refine = false;  // the last pass of a fit: with target joints the refinement reads the adjustable parts
                              // alone (launch_lbs_bm adj_only); Route::psum_combine_last
  // kForward
  const ForwardArgs* shape = nullptr;  // null: at ws.beta / ws.trans; else at the caller's betas / nb / kid / trans, which
                                       // the batch-major path copies there first (launch_posed_pass)
  float* out = nullptr;
  // kForward to the caller, blended: out = blend_in + (mesh - blend_in) * blend_mix[v] (batch-major only; k_unlayout_vertices<true>)
  const float* blend_in = nullptr;   // (B,V,3), may be `out`
  const float* blend_mix = nullptr;  // (V)
};
LbsPass part_sums(bool joints, bool weighted, bool keep_mesh, bool mesh_all = false, bool feeds_refine = false) {
  return {Lbs::kPartSums, joints, weighted, keep_mesh, mesh_all, feeds_refine};
}
LbsPass mesh_alone(const ForwardArgs* shape, float* out) { return {Lbs::kForward, true, false, false, false, false, shape, out}; }
LbsPass mesh_blended(const ForwardArgs* shape, float* out, const float* in, const float* mix) {
  LbsPass p = mesh_alone(shape, out);
  p.blend_in = in;
  p.blend_mix = mix;
  return p;
}
int launch_lbs_pass(const smplfit_handle* h, const Route& r, const LbsPass& p, const Workspace& ws, int B, hipStream_t st) {
  const DevModel& d = h->d;
  const int Mp = (int)align_up((size_t)B, 128);
  if (p.form == Lbs::kNone) return 0;
  if (p.form == Lbs::kForward) {
    if (r.bm) {  // forward-only pass over every slot, then the inverse of the target layout
      if (int rc = launch_lbs_fwd_bm(d, share_view(h, sf::kShareLbsAll, B), ws, B, Mp, st)) return rc;
      const dim3 grid((d.V + kSlabV - 1) / kSlabV, Mp / 64);
      if (p.out && p.blend_in)
        hipLaunchKernelGGL(k_unlayout_vertices<true>, grid, dim3(256), (size_t)64 * kSlabRow * 4, st, d, ws.vpT, p.out, B, p.blend_in,
                           p.blend_mix);
      else if (p.out)
        hipLaunchKernelGGL(k_unlayout_vertices<false>, grid, dim3(256), (size_t)64 * kSlabRow * 4, st, d, ws.vpT, p.out, B,
                           (const float*)nullptr, (const float*)nullptr);
      return 0;
    }
    if (p.blend_in) return fail(SMPLFIT_ERR_UNSUPPORTED, "forward LBS pass: the blended output is written on the batch-major path only");
    if (!p.out) return fail(SMPLFIT_ERR_UNSUPPORTED, "forward LBS pass: the mesh stays in the workspace on the batch-major path only");
    if (p.shape) return launch_lbs_any<2>(d, ws, B, false, p.shape->nb, p.shape->betas, p.shape->trans, p.out, st, p.shape->kid);
    return launch_lbs_any<2>(d, ws, B, false, d.S, ws.beta, ws.trans, p.out, st);
  }
  if (r.bm) {
    const bool write_v = p.keep_mesh && (!p.joints || p.mesh_all);
#define SF_CALL_LBS(S_, KW_)                                                                                          \
  launch_lbs_bm<S_, KW_>(h, ws, B, st, p.feeds_refine ? r.psum_combine_last : r.psum_combine, write_v, p.feeds_refine && p.joints, \
                         p.weighted, p.mesh_all, p.joints ? 0 : 1)
    SF_DISPATCH_SKW(d, SF_CALL_LBS);
#undef SF_CALL_LBS
    return 0;
  }
  if (int rc = p.keep_mesh ? launch_lbs_any<1>(d, ws, B, p.weighted, d.S, ws.beta, ws.trans, nullptr, st)
                           : launch_lbs_any<0>(d, ws, B, p.weighted, d.S, ws.beta, ws.trans, nullptr, st))
    return rc;
  if (!p.joints) hipLaunchKernelGGL(k_regress_joints, dim3(B), dim3(64), 0, st, d, ws.rverts, ws.rjreg);
  return 0;
}

// STEP posed pass.  The model posed at the current parameters: the forward joint stage (fa; null: the joint rows the
// last joint stage left), v_posed by the GEMM in the route's layout, the joint rows instance-innermost where the
// batch-major kernels read them and an instance-major kernel wrote them (k_forward_joint; k_joint_stage without
// k_prologue_bm: Route::jd_transpose), the LBS pass.
struct PosedPass {
  const ForwardArgs* fa = nullptr;
  LbsPass lbs;
};
int launch_posed_pass(const smplfit_handle* h, const Route& r, const PosedPass& p, const Workspace& ws, int B, hipStream_t st) {
  const DevModel& d = h->d;
  if (p.fa) launch_forward_joint(d, *p.fa, ws, B, st);
  if (r.bm && p.lbs.shape)  // the shape / translation rows the batch-major LBS kernel reads
    hipLaunchKernelGGL(k_fill_shape, dim3((B + 255) / 256), dim3(256), 0, st, ws, B, d.S, d.jt.n_kid, p.lbs.shape->betas,
                       p.lbs.shape->nb, p.lbs.shape->kid, p.lbs.shape->trans);
  if (int rc = launch_gemm(d, ws, B, st, r.bm)) return rc;
  if (r.bm && (p.fa || r.jd_transpose)) launch_jd_transpose(d, ws, B, st);
  return launch_lbs_pass(h, r, p.lbs, ws, B, st);
}

// STEP mesh error.  The model at forward inputs, measured against the caller's targets: any of the mesh (B, V, 3), the
// joints (fa.joints: the caller's (B, J, 3), or ws.rjoints where they are not asked for), the distance of every vertex
// to its target (B, V) and of every joint to its (B, J).  Unweighted; no sums, no atomics: every element has one writer.
// r: the forward's route (Entry::kForward).  Batch-major: the forward pass leaves the mesh in ws.vpT and
// k_unlayout_error turns it, measures it and writes it only where it is asked for — no (B, V, 3) otherwise.  The other
// routes: the forward pass writes the mesh to the caller's or, where it is not asked for, to ws.tvs (B, 3, Vp; the
// sorted targets of a fit, which no forward reads), and k_point_error measures it.
struct MeshError {
  ForwardArgs fa;                  // joints set
  const float *tv = nullptr, *tj = nullptr;  // targets: (B,V,3), needed with verr; (B,J,3), needed with jerr
  float *vertices = nullptr, *verr = nullptr, *jerr = nullptr;  // each may be null
};
int launch_mesh_error(const smplfit_handle* h, const Route& r, const MeshError& p, const Workspace& ws, int B, hipStream_t st) {
  const DevModel& d = h->d;
  launch_forward_joint(d, p.fa, ws, B, st);
  if (p.jerr) {
    const size_t n = (size_t)B * d.J;
    hipLaunchKernelGGL(k_point_error, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p.fa.joints, p.tj, p.jerr, n);
  }
  if (!p.vertices && !p.verr) return 0;
  if (r.bm && p.verr) {
    if (int rc = launch_posed_pass(h, r, {nullptr, mesh_alone(&p.fa, nullptr)}, ws, B, st)) return rc;
    const int Mp = (int)align_up((size_t)B, 128);
    const dim3 grid((d.V + kSlabV - 1) / kSlabV, Mp / 64);
    if (p.vertices)
      hipLaunchKernelGGL(k_unlayout_error<true>, grid, dim3(256), (size_t)64 * kSlabRow * 4, st, d, ws.vpT, p.vertices, p.tv, p.verr, B);
    else
      hipLaunchKernelGGL(k_unlayout_error<false>, grid, dim3(256), (size_t)64 * kSlabRow * 4, st, d, ws.vpT, (float*)nullptr, p.tv,
                         p.verr, B);
    return 0;
  }
  float* mesh = p.vertices ? p.vertices : ws.tvs;
  if (int rc = launch_posed_pass(h, r, {nullptr, mesh_alone(&p.fa, mesh)}, ws, B, st)) return rc;
  if (p.verr) {
    const size_t n = (size_t)B * d.V;
    hipLaunchKernelGGL(k_point_error, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mesh, p.tv, p.verr, n);
  }
  return 0;
}

// STEP normal equations of one shape solve (its vertex block; the joint block comes from the joint stage, see
// set_joint_block).  Batch-major: one transposed GEMM feeds the residual pass and, after the solve, the LBS / part-sum
// pass of the same iteration; residual pass + pair-Gram (unit weights; k_solve_bm adds the partial sums itself), or
// the accumulate kernel (w.v: vertex weights in the solve; scaled: the solve has a scale unknown and needs the extra
// sums).  Otherwise k_shape_accum / the general accumulate, which takes the target joints as rows (tj, jw).
int launch_normal_equations(const smplfit_handle* h, const Route& r, bool joints, SolveWeights w, const float* tj, const float* jw,
                            bool scaled, const Workspace& ws, int B, hipStream_t st) {
  const DevModel& d = h->d;
  // (the features of a shape solve are those of the joint stage in front of it: k_prologue_bm's planes where it ran)
  if (int rc = launch_gemm(d, ws, B, st, r.bm, r.gemm_planes)) return rc;
  if (!r.bm) {
    const bool gjr = gen_joint_rows(d) && joints;
    return launch_accum_any(d, ws, B, w.v, r.pair_in, st, gjr ? tj : nullptr, gjr && w.j ? jw : nullptr, scaled);
  }
  // joint rows instance-innermost for the kernels below; AFTER the GEMM: in front of it the chunk's GEMM starts later
  // and the chunks overlap worse (1.37 vs 1.40 M fits/s).  (Measured and not kept: k_joint_stage writing ws.jdT itself
  // — 64 waves of one XCD completing every 256-byte row with one float each — instead of this 8 us launch: 2.54 ->
  // 2.50 M fits/s, SMPL-X 1.31 -> 1.24: the scattered stores cost the latency-bound stage more than the transpose.)
  if (r.jd_transpose) launch_jd_transpose(d, ws, B, st);
  if (scaled) launch_accum_w_bm(h, ws, B, st, w.v, true);
  else if (w.v) launch_accum_w_bm(h, ws, B, st);
  else launch_residual_bm(h, ws, B, st, r.solve_bm ? 3 : 7);
  return 0;
}

// STEP alignment of a known-shape fit (fit_scale_and_translation): k_scale_trans, or on the batch-major streams the
// alignment sums + their finish, once for the translation (mode 1) and once more for the scale (mode 2).
template <int MODE>
void launch_align_partial(const DevModel& d, bool weighted, int nchunk, const Workspace& ws, int B, int Mp, hipStream_t st) {
  const dim3 grid(Mp / 64, nchunk);
  if (weighted) hipLaunchKernelGGL((k_align_partial_bm<MODE, true>), grid, dim3(64), 0, st, d, ws, B, Mp, nchunk);
  else hipLaunchKernelGGL((k_align_partial_bm<MODE, false>), grid, dim3(64), 0, st, d, ws, B, Mp, nchunk);
}
void launch_alignment(const smplfit_handle* h, const Route& r, const ScaleTransArgs& sa, const Workspace& ws, int B, hipStream_t st) {
  const DevModel& d = h->d;
  if (!r.bm) {
    hipLaunchKernelGGL(k_scale_trans, dim3(B), dim3(256), 0, st, d, sa, ws);
    return;
  }
  const int Mp = (int)align_up((size_t)B, 128);
  AlignArgs aa{};
  aa.tj = sa.tj;
  aa.jw = sa.jw;
  aa.with_scale = sa.with_scale;
  aa.regressed = sa.regressed;
  aa.scale_out = sa.scale_out;
  aa.nchunk = B <= sf::kFineMaxBatch ? 256 : 64;
  for (aa.mode = 1; aa.mode <= (sa.with_scale ? 2 : 1); ++aa.mode) {
    if (aa.mode == 1) launch_align_partial<1>(d, sa.weighted_v, aa.nchunk, ws, B, Mp, st);
    else launch_align_partial<2>(d, sa.weighted_v, aa.nchunk, ws, B, Mp, st);
    hipLaunchKernelGGL(k_align_finish, dim3(B), dim3(64), 0, st, d, aa, ws, B, Mp);
  }
}

// The options of the shape solves of one call (enqueue_solve) and of the fit around them.
struct FitOptions {
  int num_iter;
  float beta_reg, beta_reg2, kid_reg;
  int final_adjust;
  int rotations_only;  // stop after the first rotation pass, write G to the orientations
  int share_beta = 0;                 // one shape for the whole batch (pt/lstsq.py:24-26)
  smplfit_share_allreduce_fn share_allreduce = nullptr;  // completes the sum over the ranks of a sharded batch
  void* share_user = nullptr;
  const smplfit_share_segments* segments = nullptr;  // share_beta: one shape per segment of the batch (null: one segment)
  int scale_mode = 0;                 // 1 scale_target, 2 scale_fit: the last solve has a scale unknown
  float scale_reg = 0.f;
};
FitOptions fit_options(const smplfit_fit_args& a, bool rotations_only) {
  FitOptions o{a.num_iter, a.beta_regularizer, a.beta_regularizer2, a.kid_regularizer, a.final_adjust_rots ? 1 : 0,
               rotations_only ? 1 : 0};
  o.share_beta = a.share_beta ? 1 : 0;
  o.share_allreduce = a.share_allreduce;
  o.share_user = a.share_user;
  o.scale_mode = a.scale_mode;
  o.scale_reg = a.scale_regularizer;
  return o;
}

// The solve of one shape pass on the sums already in the workspace: the plain per-instance solve, the
// scaled solve (one more unknown; extra vertex sums first) or the shared solve (assemble, sum over the
// batch [and the ranks], solve the sum).  The all-shared branch of the reference's lstsq_partial_share
// drops the ridge reference (pt/lstsq.py:45-47): so does this.
// the sums of the instances' systems of a share_beta solve, one per segment of the batch, into the rows of ws.censum:
// `assemble(first, count, cen_b0)` launches the kernel that writes the systems of the instances [first, first + count)
// to the rows [first - cen_b0, ...) of ws.cen.  The partial sums are those of the segments' blocks (sf::ShareSegments;
// without a plan the blocks of the single segment [B]) whatever the grouping of the launches — the general path, whose
// workspace holds share_chunk(B) rows, walks the block list in groups of whole blocks that fit them — so the sums
// depend on the segment sizes alone.
ShareSegs share_segs(const smplfit_share_segments* p, int B) {
  if (p) return {p->d_row_seg, p->d_seg_blk, p->d_blk_rows, p->t.nseg(), p->t.nblk()};
  return {nullptr, nullptr, nullptr, 1, (B + sf::kShareBlock - 1) / sf::kShareBlock};
}
template <class Assemble>
int share_sum(const DevModel& d, const Workspace& ws, int B, const FitOptions& o, hipStream_t st, Assemble assemble) {
  const int NC = d.S * d.S + d.S, ey = (NC + 511) / 512;
  const ShareSegs sg = share_segs(o.segments, B);
  const int room = d.general ? share_chunk(B) : B;  // rows of ws.cen (>= one block)
  const auto rows_of = [&](int p) {
    return o.segments ? o.segments->t.blk_rows[2 * p + 1] : std::min(sf::kShareBlock, B - p * sf::kShareBlock);
  };
  for (int p0 = 0, first = 0; p0 < sg.nblk;) {
    int p1 = p0, cnt = 0;
    while (p1 < sg.nblk && cnt + rows_of(p1) <= room) cnt += rows_of(p1++);
    assemble(first, cnt, d.general ? first : 0);
    hipLaunchKernelGGL(k_share_partial, dim3(p1 - p0, ey), dim3(512), 0, st, ws, sg, B, NC, p0, d.general ? first : 0);
    p0 = p1;
    first += cnt;
  }
  hipLaunchKernelGGL(k_share_reduce, dim3(sg.nseg, ey), dim3(512), 0, st, ws, sg, NC);
  if (o.share_allreduce && o.share_allreduce(o.share_user, ws.censum, NC, (void*)st) != 0)
    return fail(SMPLFIT_ERR_HIP, "the share_allreduce callback failed");
  return 0;
}

// An unscaled solve on the bm path with r.solve_bm finds the PARTIAL sums of k_residual_bm + k_pair_gram_bm in the
// workspace (the combine was not launched) and k_solve_bm takes them from there; otherwise the record is in ws.gramv.
// The scaled solve of the bm path finds the extra sums of k_accum_w_bm in ws.vextra.
int enqueue_solve(const smplfit_handle* h, const Route& r, const Workspace& ws, int B, const FitOptions& o, bool joints,
                  SolveWeights w, const float* jw, int use_ref, bool scaled, hipStream_t st) {
  const DevModel& d = h->d;
  const int pair_in = scaled ? r.pair_in_scaled : r.pair_in;
  const bool extras_done = r.bm && scaled;
  if (d.general && scaled && !tune().gen_mfma)
    return fail(SMPLFIT_ERR_UNSUPPORTED, "general path with SMPLFIT_GEN_MFMA=0: the scale unknown's extra sums come from the "
                                         "matrix-core accumulate kernel only");
  if (scaled) {
    // (extras_done: the batch-major accumulate of this iteration has left the extra sums in ws.vextra; general path:
    // they are entries of the accumulate kernel's rank-k update — its target column — in ws.gvex, joints included)
#define SF_CALL_EXTRAS(S_, KW_)                                                                       \
  hipLaunchKernelGGL((k_scale_extras<S_, KW_>), dim3(B), dim3(64),                                    \
                     (size_t)d.J * sf::jd_stride(S_) * 4, st, d, ws, w.v ? 1 : 0)
    if (!extras_done && !d.general) SF_DISPATCH_SKW(d, SF_CALL_EXTRAS);
#undef SF_CALL_EXTRAS
    ScaledSolveArgs sa{};
    const bool joint_rows = gen_joint_rows(d) && joints;  // the joints' terms are in the records already
    sa.tj = (joints && !joint_rows) ? ws.tjc : nullptr;
    sa.jw = w.j ? jw : nullptr;
    sa.joint_block = (joints && !joint_rows) ? 1 : 0;
    sa.mode = o.scale_mode;
    sa.pair_form = pair_in;
    sa.use_ref = use_ref;
    sa.beta_reg = o.beta_reg; sa.beta_reg2 = o.beta_reg2; sa.kid_reg = o.kid_reg; sa.scale_reg = o.scale_reg;
    sa.B = B;
    const size_t lds = d.general ? (size_t)(sf::kSolvePanel * (d.S + 1) + sf::kSolvePanel) * 8 : (size_t)sf::scaled_solve_scratch_floats(d.S) * 4;
    const int threads = d.general ? (d.S > 128 ? 1024 : d.S > 64 ? 256 : 64) : 64;
    auto launch = [&](int first, int count, int cen_b0) {
      sa.b0 = first;
      sa.cen_b0 = cen_b0;
      if (d.general) {
        ensure_max_lds(reinterpret_cast<const void*>(&k_shape_solve_scaled<true>));
        hipLaunchKernelGGL(k_shape_solve_scaled<true>, dim3(count), dim3(threads), lds, st, d, ws, sa);
      } else {
        hipLaunchKernelGGL(k_shape_solve_scaled<false>, dim3(count), dim3(64), lds, st, d, ws, sa);
      }
    };
    if (o.share_beta) {  // shared shape, own scale: reduced systems, their sum, solve (pt/lstsq.py:50-90)
      sa.row_seg = o.segments ? o.segments->d_row_seg : nullptr;
      sa.share = 1;
      if (int rc = share_sum(d, ws, B, o, st, launch)) return rc;
      sa.share = 2;
    }
    launch(0, B, 0);
  } else if (o.share_beta) {  // assemble per instance, sum over the batch, solve the sum + own translation
    auto assemble = [&](int first, int count, int cen_b0) {
      launch_shape_solve(d, ws, B, st, o.beta_reg, o.beta_reg2, o.kid_reg, pair_in, 0, 1, first, count, cen_b0);
    };
    if (int rc = share_sum(d, ws, B, o, st, assemble)) return rc;
    launch_shape_solve(d, ws, B, st, o.beta_reg, o.beta_reg2, o.kid_reg, pair_in, 0, 2, 0, -1, 0,
                       o.segments ? o.segments->d_row_seg : nullptr);
  } else if (r.solve_bm) {
    launch_solve_bm(h, r.solve_plan, ws, B, st, o.beta_reg, o.beta_reg2, o.kid_reg, use_ref, r.prologue_bm);
  } else {
    launch_shape_solve(d, ws, B, st, o.beta_reg, o.beta_reg2, o.kid_reg, pair_in, use_ref);
  }
  return 0;
}

// Shared driver of fit / part_rotations, on one chunk of the batch: `a` holds the chunk's rows (chunk_view), source
// the chunk's input side of a fused conversion (smplfit_convert_f32: the targets are produced on the device — forward
// of the input model on the batch-major kernels, topology transfer straight into this fit's target stream — instead
// of being read from target_vertices).
int run_fit(const smplfit_handle* h, const smplfit_fit_args& a, bool rotations_only, const ConvertSource* source,
            const Workspace& ws, hipStream_t st, int ph_lo = 0, int ph_hi = 1 << 30, bool vw_shared = false,
            const smplfit_share_segments* segments = nullptr, int call_batch = 0) {  // call_batch: CallShape::call_batch
  // PHASES.  The launches of a fit are numbered in phases — 0: the prologue up to the first rotation pass; 1 + 2 it:
  // the vertex block of iteration `it` up to the normal equations; 2 + 2 it: solve, vertices at the solution, next
  // rotation pass; 1 + 2 num_iter: refinement and epilogue — and a call enqueues the phases [ph_lo, ph_hi) only (the
  // host-side state is rebuilt every time): a chunked fit enqueues its chunks phase by phase, alternating between
  // their streams, instead of one whole chunk after the other (fit_impl).
  const auto on = [&](int ph) { return ph >= ph_lo && ph < ph_hi; };
  const DevModel& d = h->d;
  const int B = a.batch;
  const float *tj = a.target_joints, *vw = a.vertex_weights, *jw = a.joint_weights;
  const bool joints = tj != nullptr;
  const bool vweighted = vw != nullptr;
  const SolveWeights w = solve_weights(joints, vw, jw);
  FitOptions o = fit_options(a, rotations_only);
  o.segments = segments;  // (fit_impl has set a.share_beta)
  // warm start (bodyfitter.py:363-382): the first rotation pass runs against the model posed with the initial values
  // instead of the template — only when a pose or a shape is given —; the ridge references reach EVERY shape solve
  // whenever they are given — also an initial_kid_factor on its own (:413-414, :448-449)
  const bool warm = a.initial_pose_rotvecs || a.initial_shape_betas;
  const int use_ref = (a.initial_shape_betas || a.initial_kid_factor) ? 1 : 0;
  // vertex weights on the batch-major path: the weight stream, weighted part sums, and — when the weights enter the
  // shape solve — the weighted accumulate.  scale_target / scale_fit: the LAST iteration's solve has one more unknown
  // and needs extra vertex sums — that iteration runs the accumulate kernel (with or without weights) in its EXTRAS form
  const Route r = route_of(h, B, {source ? Entry::kConvert : Entry::kFit, joints, vweighted, w.v, o.scale_mode,
                                  o.share_beta != 0, o.rotations_only != 0, warm, call_batch});
  if (source && !r.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "fused conversion: the batch-major path does not apply");
  if (on(0)) {
    TargetsIn t{a.target_vertices, tj, vw, vw, source, !warm, true, vw_shared};
    if (int rc = launch_targets_in(h, r, t, ws, B, st)) return rc;
  }
  const float* tj_rot = rotation_targets(ws, joints);
  JointStageArgs ja{};
  ja.tj = tj_rot;
  ja.jw = jw;
  set_joint_block(&ja, d, joints, w);
  ja.do_prologue = o.rotations_only ? 0 : 1;
  ja.fit_rotations = 1;
  ja.Gprev = nullptr;
  if (on(0) && (warm || use_ref))
    hipLaunchKernelGGL(k_fill_shape, dim3((B + 255) / 256), dim3(256), 0, st, ws, B, d.S, d.jt.n_kid, a.initial_shape_betas,
                       std::min(a.initial_shape_betas ? a.num_initial_betas : 0, d.S - d.jt.n_kid - d.jt.n_pad),
                       a.initial_kid_factor);
  if (warm) {
    // the first part sums against the posed initial model (the wave-per-instance pass has always kept the mesh here,
    // with target joints as well)
    ForwardArgs fa{};
    fa.pose = a.initial_pose_rotvecs;  // null: rest pose
    fa.betas = ws.beta;                // (B,S) incl. the kid column
    fa.nb = d.S;
    fa.joints = ws.rjoints;
    fa.orient = ws.G;
    if (on(0))
      if (int rc = launch_posed_pass(h, r, {&fa, part_sums(joints, vweighted, true)}, ws, B, st)) return rc;
    ja.rj = joints ? ws.rjoints : ws.rjreg;
    ja.rj_shared = 0;
    ja.Gprev = ws.G;  // compose with the initial orientations
  } else if (joints) {
    ja.rj = d.j_template;
    ja.rj_shared = 1;
  } else {  // template joints regressed from the default mesh: same regressor on a (1,3,Vp) source
    if (on(0)) hipLaunchKernelGGL(k_regress_joints, dim3(1), dim3(64), 0, st, d, d.dm, ws.rjreg);
    ja.rj = ws.rjreg;
    ja.rj_shared = 1;
  }
  // (first rotations: the rows of the template pass — or of the warm start's LBS pass —; previous rotations: the
  // instance-major ws.G of the warm start's forward stage, if any)
  if (on(0))
    launch_joint_stage_fit(h, ja, ws, B, st, r.prologue_bm, r.rot_kind_first, ja.Gprev ? 2 : 0, r.gemm_planes, r.rot_spread);
  if (o.rotations_only) {
    if (on(0)) hipLaunchKernelGGL(k_copy, dim3(256), dim3(256), 0, st, ws.G, a.orientations, (size_t)B * d.J * 9);
    return post_launch_check();
  }
  for (int it = 0; it < o.num_iter; ++it) {
    const bool pb = on(2 + 2 * it), last = it + 1 == o.num_iter;
    const bool scaled_now = o.scale_mode && last;  // only the last solve (:434-455)
    if (on(1 + 2 * it))
      if (int rc = launch_normal_equations(h, r, joints, w, tj_rot, jw, scaled_now, ws, B, st)) return rc;
    // K4 stays its own launch: fused into the prologue of the LBS kernel (template flag SOLVE) its
    // ~40 serial barriers stall all four waves of the workgroup and the kernel ran 230 us longer
    if (pb)
      if (int rc = enqueue_solve(h, r, ws, B, o, joints, w, jw, use_ref, scaled_now, st)) return rc;
    if (last && !o.final_adjust) break;  // nothing consumes the re-evaluated mesh
    if (pb)
      if (int rc = launch_lbs_pass(h, r, part_sums(joints, vweighted, !joints, false, last), ws, B, st)) return rc;
    if (last) break;
    ja.rj = joints ? ws.rjoints : ws.rjreg;
    ja.rj_shared = 0;
    ja.Gprev = ws.G;
    if (pb) launch_joint_stage_fit(h, ja, ws, B, st, r.prologue_bm, r.rot_kind_next, 1, r.gemm_planes, r.rot_spread);
  }
  if (!on(1 + 2 * o.num_iter)) return post_launch_check();
  RefineArgs ra = refine_args(tj_rot, joints, jw, o.final_adjust, ws, a.pose_rotvecs, a.shape_betas, a.trans, a.kid_factor,
                              a.orientations, a.relative_orientations);
  if (o.scale_mode) {
    hipLaunchKernelGGL(k_scale_refs, dim3(B), dim3(64), 0, st, d, ws, tj_rot, o.scale_mode,
                       o.final_adjust ? 1 : 0, joints ? 0 : 1);
    if (o.scale_mode == 1 && o.final_adjust) ra.tj = ws.tjs;  // target joints times the scale
    ra.scaled = o.scale_mode == 2 ? 1 : 0;                      // rest joints times the scale (:1449-1450)
    if (a.scale_corr)
      hipLaunchKernelGGL(k_copy, dim3(16), dim3(256), 0, st, ws.scale, a.scale_corr, (size_t)B);
  }
  if (r.refine_bm) {
    launch_refine_bm(h, ra, share_view(h, r.refine_kind, B), ws, B, st);
  } else {
    if (r.gt_to_g) {  // (k_rotations_bm left the rotations instance-innermost only)
      count_stage(SMPLFIT_STAGE_GT_TO_G);
      hipLaunchKernelGGL(k_gt_to_g, dim3((B + 63) / 64, (d.J + 15) / 16), dim3(256), 0, st, ws, d.J, B, (int)align_up((size_t)B, 128));
    }
    launch_refine(d, ra, ws, B, st);
  }
  return post_launch_check();
}

// fit_with_known_shape (bodyfitter.py:655-838): pose and translation (optionally a scale) for given
// shape parameters.  Alternates the posed pass at the current rotations (forward joint stage, GEMM, the
// part sums against the target) with the part-rotation stage; then the alignment stage
// and the dependent refinement.  num_iter rotation passes, num_iter + 1 posed passes.
struct KnownShapeOptions {
  int num_iter, final_adjust, scale_fit;
};

int run_fit_known_shape(const smplfit_handle* h, const float* betas, int nb, const float* kid,
                        const float* init_pose, const float* tv, const float* tj, const float* vw,
                        const float* jw, int B, const KnownShapeOptions& o, float* pose, float* trans,
                        float* scale_out, float* orient, float* rel, const Workspace& ws, hipStream_t st) {
  const DevModel& d = h->d;
  const bool joints = tj != nullptr;
  const bool vweighted = vw != nullptr;
  const Route r = route_of(h, B, {Entry::kKnownShape, joints, vweighted});
  if (int rc = launch_targets_in(h, r, {tv, tj, vw, vw, nullptr, false, true}, ws, B, st)) return rc;
  const float* tj_rot = rotation_targets(ws, joints);
  hipLaunchKernelGGL(k_fill_shape, dim3((B + 255) / 256), dim3(256), 0, st, ws, B, d.S, d.jt.n_kid, betas,
                     std::min(nb, d.S - d.jt.n_kid - d.jt.n_pad), kid);
  ForwardArgs fa{};
  fa.pose = init_pose;  // null -> rest pose
  fa.betas = ws.beta;   // (B,S) incl. the kid column: j_ext's last column is kid_J_shapedir
  fa.nb = d.S;
  fa.joints = ws.rjoints;
  fa.orient = ws.G;
  JointStageArgs ja{};
  ja.tj = tj_rot;
  ja.jw = jw;
  ja.fit_rotations = 1;
  ja.do_prologue = 0;
  ja.rj_shared = 0;
  ja.Gprev = ws.G;
  // the posed mesh is kept where it is read: regressed joints, and the alignment sums behind the last pass
  for (int it = 0; it <= o.num_iter; ++it) {
    if (int rc = launch_posed_pass(h, r, {&fa, part_sums(joints, vweighted, true, it == o.num_iter)}, ws, B, st)) return rc;
    if (it == o.num_iter) break;
    ja.rj = joints ? ws.rjoints : ws.rjreg;
    launch_joint_stage(d, ja, ws, B, st);
    fa.pose = nullptr;
    fa.glob = ws.G;
  }
  const SolveWeights w = solve_weights(joints, vw, jw);
  ScaleTransArgs sa{};
  sa.tj = joints ? ws.tjc : nullptr;
  sa.weighted_v = w.v;
  sa.jw = w.j ? jw : nullptr;
  sa.with_scale = o.scale_fit;
  sa.regressed = joints ? 0 : 1;
  sa.scale_out = o.scale_fit ? scale_out : nullptr;
  launch_alignment(h, r, sa, ws, B, st);
  RefineArgs ra = refine_args(tj_rot, joints, jw, o.final_adjust, ws, pose, nullptr, trans, nullptr, orient, rel);
  ra.scaled = o.scale_fit;
  launch_refine(d, ra, ws, B, st);
  return post_launch_check();
}

// The target stream of a fused conversion (smplfit_convert_f32), per chunk:
//   the posed pass of the INPUT model on the batch-major kernels, forward only (the posed vertices stay in the input
//   model's instance-innermost buffer), then k_transfer_bm into the OUTPUT model's target stream + slab sums;
//   launch_targets_in finishes them as it does the layout pass's.
// src.kid: the flip's input mesh is evaluated with the kid factor (the input handle is then the kid handle); the
// conversion passes none.
int launch_convert_source(const ConvertSource& src, const Workspace& ws, int B, hipStream_t st) {
  const smplfit_convert_plan& pl = *src.plan;
  const DevModel& d = pl.out->d;
  const DevModel& di = pl.in->d;
  const Workspace& wi = src.wsi;
  const int Mp = (int)align_up((size_t)B, 128);
  hipLaunchKernelGGL(k_fill_shape, dim3((B + 255) / 256), dim3(256), 0, st, wi, B, di.S, di.jt.n_kid, src.betas,
                     src.betas ? std::min(src.nb, di.S - di.jt.n_kid - di.jt.n_pad) : 0, src.kid, src.trans);
  ForwardArgs fa{};
  fa.pose = src.pose;
  fa.betas = wi.beta;  // (B,S) rows, zero beyond the given betas
  fa.nb = di.S;
  fa.joints = wi.rjoints;
  Route ri;  // (the entry points have checked that the batch-major path serves the input model)
  ri.bm = true;
  if (int rc = launch_posed_pass(pl.in, ri, {&fa, mesh_alone(nullptr, nullptr)}, wi, B, st)) return rc;
  TransferTabs tt{pl.d_oslot, pl.d_start, pl.d_islot, pl.d_w, d.V};
  if (pl.negate_x)
    hipLaunchKernelGGL(k_transfer_bm<true>, dim3(pl.nslab, Mp / 64), dim3(256), 0, st, tt, wi.vpT, di.Vp, ws.tT, d.Vp, ws.resP, Mp);
  else
    hipLaunchKernelGGL(k_transfer_bm<false>, dim3(pl.nslab, Mp / 64), dim3(256), 0, st, tt, wi.vpT, di.Vp, ws.tT, d.Vp, ws.resP, Mp);
  return 0;
}

// Chunk plan of one fit call: a large batch may be split into chunks (SMPLFIT_CHUNKS=1..4) that run concurrently on
// the caller's stream and the handle's side streams, so that the small latency-bound kernels of one chunk run beside
// the heavy kernels of the other (the GEMM itself never shares a CU).  Default, measured at B = 4096 in round 4 (the
// streams non-temporal, the vertex passes one balanced round): the SMPL-shaped model 2.40 M fits/s in one chunk,
// 2.37 in two, 2.21 in three; the SMPL-X-shaped one 1.13 M in one, 1.20 in two — its per-instance stages (55 joints)
// are a larger share of the fit: two chunks for models with more than 32 joints, one otherwise.
// Chunk sizes are multiples of 128 (the GEMM's instance tile).
int chunk_count(const sf::HostTables& t) {
  const int c = tune().chunks;
  return std::min(c > 0 ? c : (t.J > 32 ? 2 : 1), kMaxChunks);
}
int chunk_plan_n(int n, int batch, int* sizes) {
  // every chunk at least 896 instances (128 above sf::kFineMaxBatch): the chunks of a call all walk the coarse cell
  // tables, and which tables a call takes depends on its batch alone (sf_tables.h).  Chunks are multiples of 128
  // instances, the last one takes the remainder.
  constexpr int kMinChunk = (sf::kFineMaxBatch / 128 + 1) * 128;
  static_assert(kMinChunk > sf::kFineMaxBatch && kMinChunk % 128 == 0, "chunks stay on the coarse tables");
  while (n > 1 && batch < n * kMinChunk) --n;
  const int per = batch / n / 128 * 128;
  for (int k = 0; k + 1 < n; ++k) sizes[k] = per;
  sizes[n - 1] = batch - (n - 1) * per;
  return n;
}
int chunk_plan(const sf::HostTables& t, int batch, int* sizes) { return chunk_plan_n(chunk_count(t), batch, sizes); }

// LAYOUT one chunk of a fit call: the fit's workspace, then — `tin`, the input model of a fused conversion — that
// model's forward-only slice
struct ChunkLayout {
  Workspace ws, wsi;
};
ChunkLayout chunk_layout(const sf::HostTables& t, const sf::HostTables* tin, int nb, Arena& ar) {
  ChunkLayout l{};
  l.ws = carve(t, nb, ar);
  if (tin) l.wsi = carve(*tin, nb, ar, true);
  return l;
}

// The chunks of a call one behind the other (fit_impl).  Sized for every chunk count a call may pick (the tuning
// options can be reloaded between the two calls).
size_t chunked_workspace_bytes(const sf::HostTables& t, int batch, const sf::HostTables* tin = nullptr) {
  size_t need = 0;
  for (int n = 1; n <= kMaxChunks; ++n) {
    int sizes[kMaxChunks];
    const int k = chunk_plan_n(n, batch, sizes);
    Arena ar{nullptr};
    for (int i = 0; i < k; ++i) chunk_layout(t, tin, sizes[i], ar);
    need = std::max(need, ar.off);
  }
  return need;
}

// the input side of a fused conversion, whole batch (fit_impl cuts it into the chunks' ConvertSource)
struct ConvertJob {
  const smplfit_convert_plan* plan;
  const float *pose, *betas, *trans;
  int nb;
  const float* kid;  // (B) or null
};

// The rows [b0, b0 + nb) of a fit call as a call of their own: every per-instance array offset, batch = nb.
smplfit_fit_args chunk_view(const smplfit_fit_args& a, const sf::HostTables& t, int b0, int nb) {
  smplfit_fit_args v = a;
  const auto rows = [b0](auto*& p, size_t width) {
    if (p) p += (size_t)b0 * width;
  };
  const size_t J = t.J, V = t.V;
  rows(v.target_vertices, V * 3);
  rows(v.target_joints, J * 3);
  rows(v.vertex_weights, V);
  rows(v.joint_weights, J);
  rows(v.initial_pose_rotvecs, J * 3);
  rows(v.initial_shape_betas, (size_t)a.num_initial_betas);
  rows(v.initial_kid_factor, 1);
  rows(v.pose_rotvecs, J * 3);
  rows(v.shape_betas, (size_t)t.num_betas());
  rows(v.trans, 3);
  rows(v.kid_factor, 1);
  rows(v.orientations, J * 9);
  rows(v.relative_orientations, J * 9);
  rows(v.scale_corr, 1);
  v.batch = nb;
  return v;
}

// LAYOUT segments: behind the workspace of a call with a plan of segments (its own query's size), the plan's partial
// rows and per-segment sums; point_segments hands them to the call's Workspace in place of the single segment's
struct SegmentsLayout {
  double *cenP, *censum;
};
SegmentsLayout segments_layout(const sf::HostTables& t, const smplfit_share_segments& p, Arena& ar) {
  const size_t NC = (size_t)t.S * t.S + t.S;
  SegmentsLayout l{};
  l.cenP = ar.take<double>((size_t)p.t.nblk() * NC);
  l.censum = ar.take<double>((size_t)p.t.nseg() * NC);
  return l;
}
size_t segments_workspace_bytes(const smplfit_handle* h, const smplfit_share_segments& p) {
  Arena ar{nullptr};
  ar.take<char>(chunked_workspace_bytes(h->t, p.t.batch));
  segments_layout(h->t, p, ar);
  return ar.off;
}
Workspace point_segments(Workspace ws, const smplfit_handle* h, const smplfit_share_segments& p, void* workspace) {
  Arena ar{(char*)workspace};
  ar.take<char>(chunked_workspace_bytes(h->t, p.t.batch));
  const SegmentsLayout l = segments_layout(h->t, p, ar);
  ws.cenP = l.cenP;
  ws.censum = l.censum;
  return ws;
}
// What the two entry points with a plan of segments check before anything else (NULL plan: nothing)
int check_segments(const char* who, const smplfit_share_segments* p, int batch, smplfit_share_allreduce_fn share_allreduce) {
  if (!p) return 0;
  if (batch != p->t.batch)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": batch " + std::to_string(batch) + " is not the plan's " + std::to_string(p->t.batch));
  if (share_allreduce) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": share_allreduce cannot be combined with segments");
  if (!p->has_device) return fail(SMPLFIT_ERR_HIP, std::string(who) + ": the plan of segments is host-only");
  return 0;
}

// vw_shared: args->vertex_weights is one (V) row for the whole batch (smplfit_replace_hands_f32).  The entry has run
// check_call against its own query, which holds chunked_workspace_bytes from a.workspace on: a.workspace_bytes is not
// read here.
// segments: the plan of smplfit_fit_segments_f32 (a.share_beta set; a.workspace holds segments_workspace_bytes).
int fit_impl(const smplfit_handle* h, const smplfit_fit_args* args, const ConvertJob* job, bool vw_shared = false,
             const smplfit_share_segments* segments = nullptr) {
  const smplfit_fit_args& a = *args;
  const int batch = a.batch;
  int rc = 0;
  if ((!a.target_vertices && !job) || !a.pose_rotvecs || !a.shape_betas || !a.trans)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_f32: null input/output pointer");
  if (a.num_iter < 1) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_f32: num_iter must be >= 1");
  if (a.initial_kid_factor && !h->t.n_kid)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_warm_f32: initial_kid_factor given to a handle without kid");
  if (a.initial_shape_betas && (a.num_initial_betas < 0 || a.num_initial_betas > h->t.num_betas()))
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_warm_f32: num_initial_betas must lie in [0, the model's betas]; slice first");
  if ((rc = check_scale_share("smplfit_fit_ex_f32", a.scale_mode, a.scale_corr, a.share_beta, a.share_allreduce))) return rc;
  hipStream_t st = (hipStream_t)a.hip_stream;
  int sizes[kMaxChunks] = {batch};
  // share_beta couples all instances in every shape solve: one chunk
  const int nchunk = (h->have_streams && !a.share_beta) ? chunk_plan(h->t, batch, sizes) : 1;
  const int Jin = job ? job->plan->in->t.J : 0;
  int b0s[kMaxChunks];
  ChunkLayout lay[kMaxChunks];  // every chunk's slice of the workspace, one behind the other
  {
    Arena ar{(char*)a.workspace};
    int b0 = 0;
    for (int c = 0; c < nchunk; ++c) {
      b0s[c] = b0;
      lay[c] = chunk_layout(h->t, job ? &job->plan->in->t : nullptr, sizes[c], ar);
      b0 += sizes[c];
    }
  }
  auto run_chunk = [&](int c, hipStream_t cs, int ph_lo, int ph_hi) -> int {
    const int b0 = b0s[c], nb = sizes[c];
    ConvertSource src{};
    if (job) {
      src.plan = job->plan;
      src.pose = job->pose + (size_t)b0 * Jin * 3;
      src.betas = job->betas ? job->betas + (size_t)b0 * job->nb : nullptr;
      src.trans = job->trans ? job->trans + (size_t)b0 * 3 : nullptr;
      src.nb = job->nb;
      src.kid = job->kid ? job->kid + b0 : nullptr;
      src.wsi = lay[c].wsi;
    }
    smplfit_fit_args v = chunk_view(a, h->t, b0, nb);
    if (vw_shared) v.vertex_weights = a.vertex_weights;  // (every chunk reads the one row)
    // (a plan of segments: share_beta, so the one chunk)
    const Workspace ws = segments ? point_segments(lay[c].ws, h, *segments, a.workspace) : lay[c].ws;
    return run_fit(h, v, false, job ? &src : nullptr, ws, cs, ph_lo, ph_hi, vw_shared, segments, batch);
  };
  if (nchunk <= 1) return run_chunk(0, st, 0, 1 << 30);
  // fork: every chunk is an independent fit with its own workspace slice; chunk 0 stays on the
  // caller's stream, the others go to the handle's side streams and are joined back by events
  // (stream-ordered with respect to the caller, hipGraph-capturable).  The handle's streams and
  // events are shared state: concurrent fit calls on one handle serialise their ENQUEUE here.
  // The chunks are enqueued PHASE BY PHASE (run_fit), alternating between their streams: enqueued one whole chunk
  // after the other, the second chunk's first kernel waits for the host to get through the ~30 launches of the
  // first.  (Measured and not kept, round 4: a deliberate offset between the chunks — chunk c starting when chunk
  // c - 1 has finished k phases, so that the bandwidth-bound kernels of one meet the latency-bound ones of the other:
  // 2.37 M fits/s without, 2.23 / 2.19 / 2.10 with k = 1 / 2 / 3: the offset is paid again at the join of every call.
  // Nor an enforced anti-phase: a "bandwidth token" of events that orders the vertex sections (layout, GEMM + residual,
  // LBS) of all chunks into one sequence, so that a chunk's per-instance stages run beside another chunk's vertex
  // section: 2.56 -> 2.15 M fits/s with two chunks, 1.75 / 1.51 with three / four (SMPL-X 1.34 -> 1.19): every
  // cross-queue event wait costs ~25 us of idle queue, twelve of them per fit.)
  std::lock_guard<std::mutex> lock(h->mu);
  SF_HIP_TRY(hipEventRecord(h->ev_fork, st));
  const int nphase = 2 + 2 * a.num_iter;
  int first_error = 0;
  std::string first_msg;
  bool forked[kMaxChunks] = {true, false, false, false};
  auto note = [&](int rc2) {
    if (rc2 && !first_error) {
      first_error = rc2;
      first_msg = g_last_error;
    }
  };
  for (int ph = 0; ph < nphase && !first_error; ++ph)
    for (int c = 0; c < nchunk && !first_error; ++c) {
      hipStream_t cs = c == 0 ? st : h->side[c - 1];
      if (ph == 0 && c > 0) {
        // a failed fork is an error like any other: the chunks forked before it are still joined below
        const hipError_t fe = hipStreamWaitEvent(cs, h->ev_fork, 0);
        if (fe != hipSuccess) {
          note(fail(SMPLFIT_ERR_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(fe)));
          break;
        }
        forked[c] = true;
      }
      note(run_chunk(c, cs, ph, ph + 1));
    }
  // a chunk that was forked is always joined back, also after an error: an unjoined fork would
  // invalidate a stream capture and leave work in flight that the caller's stream does not wait for
  for (int c = 1; c < nchunk; ++c)
    if (forked[c]) {
      (void)hipEventRecord(h->ev_join[c - 1], h->side[c - 1]);
      (void)hipStreamWaitEvent(st, h->ev_join[c - 1], 0);
    }
  if (first_error) return fail(first_error, first_msg);
  return SMPLFIT_OK;
}

// the fit behind a fused conversion / flip: its options and outputs (A: smplfit_convert_args, smplfit_flip_args)
template <class A>
smplfit_fit_args fused_fit_args(const A& a) {
  smplfit_fit_args f{};
  f.batch = a.batch;
  f.num_iter = a.num_iter;
  f.beta_regularizer = a.beta_regularizer;
  f.beta_regularizer2 = a.beta_regularizer2;
  f.kid_regularizer = a.kid_regularizer;
  f.final_adjust_rots = a.final_adjust_rots;
  f.pose_rotvecs = a.out_pose_rotvecs;
  f.shape_betas = a.out_shape_betas;
  f.trans = a.out_trans;
  f.kid_factor = a.out_kid_factor;
  f.orientations = a.out_orientations;
  f.relative_orientations = a.out_relative_orientations;
  f.hip_stream = a.hip_stream;
  return f;
}

// smplfit_transfer_f32 / smplfit_transfer_backward_f32: out (B,Vout,3) = A in (B,Vin,3) with the (Vout x Vin) device CSR
// A — the matrix, or its transpose with the two vertex counts swapped; the staged form where the input rows fit the LDS
template <bool NEG>
void launch_transfer_rows(const int32_t* d_indptr, const int32_t* d_indices, const float* d_values, int Vin, int Vout,
                          const float* in, int batch, float* out, hipStream_t st) {
  const size_t lds = (size_t)Vin * 12;
  if (lds <= 160 * 1024) {
    ensure_max_lds(reinterpret_cast<const void*>(&k_transfer_rows<true, NEG>));
    hipLaunchKernelGGL((k_transfer_rows<true, NEG>), dim3(batch), dim3(1024), lds, st, in, out, d_indptr, d_indices,
                       d_values, Vin, Vout);
  } else {
    hipLaunchKernelGGL((k_transfer_rows<false, NEG>), dim3(batch), dim3(1024), 0, st, in, out, d_indptr, d_indices,
                       d_values, Vin, Vout);
  }
}

// The tables of k_transfer_bm in `p` (models p->in / p->out set): the matrix (NULL = identity) re-indexed to the sorted
// slots of the two models, uploaded to the current device as arrays of `dev`.  Shared by the conversion and the flip plans.
int upload_slot_transfer(smplfit_convert_plan* p, DeviceArrays& dev, const smplfit_transfer* transfer, const char* who) {
  const std::vector<int32_t>& inv_in = p->in->t.inv_slot;
  const int Vo = p->out->t.V;
  std::vector<int32_t> start(Vo + 1, 0), islot;
  std::vector<float> w;
  for (int r = 0; r < Vo; ++r) {
    if (transfer) {
      for (int e = transfer->indptr[r]; e < transfer->indptr[r + 1]; ++e) {
        islot.push_back(inv_in[transfer->indices[e]]);
        w.push_back(transfer->values[e]);
      }
    } else {  // same topology: the identity
      islot.push_back(inv_in[r]);
      w.push_back(1.f);
    }
    start[r + 1] = (int32_t)islot.size();
  }
  p->nslab = (Vo + kSlabV - 1) / kSlabV;
  p->negate_x = transfer && transfer->negate_x;
  if (dev.upload(p->out->t.inv_slot, &p->d_oslot) || dev.upload(start, &p->d_start) || dev.upload(islot, &p->d_islot) ||
      dev.upload(w, &p->d_w))
    return fail(SMPLFIT_ERR_HIP, std::string(who) + ": device upload failed");
  return 0;
}

// ------------------------------------------------------------------------------------------------
// LAYOUTS.  One function per entry point: it takes the entry's regions from an Arena in order and leaves the total in
// it.  The entry's workspace query runs it on a null base, the entry itself on the caller's pointer; a layout that
// begins with another one calls it.  (carve and chunk_layout, above, are the fit's.)
// ------------------------------------------------------------------------------------------------
Workspace fit_workspace(const smplfit_handle* h, int B, void* base) {
  Arena ar{(char*)base};
  return carve(h->t, B, ar);
}

// LAYOUT forward-backward: the fit's workspace (the backward recomputes the posed pass in it), then BwdWorkspace
struct BackwardLayout {
  Workspace ws;
  BwdWorkspace bw;
};
BackwardLayout backward_layout(const sf::HostTables& t, int B, Arena& ar) {
  BackwardLayout l;
  l.ws = carve(t, B, ar);
  const size_t NC = (size_t)t.P + t.S;
  l.bw.dvp = ar.take<float>((size_t)B * 3 * t.Vp);
  l.bw.dA = ar.take<float>((size_t)B * t.J * 12);
  l.bw.dtv = ar.take<float>((size_t)B * 3);
  l.bw.part = ar.take<float>((size_t)bwd_nsplit(t.Vp) * B * NC);
  l.bw.dfeat = ar.take<float>((size_t)B * NC);
  l.bw.jscr = ar.take<float>((size_t)B * sf::joint_bwd_scratch_floats(t.J));
  return l;
}

// LAYOUT fit objective: the backward's, then the (B, J, 3) joint cotangent of k_obj_joint.  (The mesh objective takes
// the backward's own: its loss sums live in LDS, k_obj_vertex.)
struct ObjectiveLayout {
  BackwardLayout fb;
  float* gjoints;
};
ObjectiveLayout objective_layout(const sf::HostTables& t, int B, Arena& ar) {
  ObjectiveLayout l;
  l.fb = backward_layout(t, B, ar);
  l.gjoints = ar.take<float>((size_t)B * t.J * 3);
  return l;
}

// LAYOUT adjoint of the shape solve: the backward's (the three vector-Jacobian products run in it), then AdjWorkspace
struct AdjointLayout {
  BackwardLayout fb;
  AdjWorkspace aw;
};
AdjointLayout adjoint_layout(const sf::HostTables& t, int B, Arena& ar) {
  AdjointLayout l;
  l.fb = backward_layout(t, B, ar);
  l.aw.lam = ar.take<float>((size_t)B * (t.S + 3));
  l.aw.lamb = ar.take<float>((size_t)B * std::max(1, t.num_betas()));
  l.aw.lamk = ar.take<float>((size_t)B);
  l.aw.c1 = ar.take<float>((size_t)B * t.V * 3);
  l.aw.c2 = ar.take<float>((size_t)B * t.V * 3);
  l.aw.c1j = ar.take<float>((size_t)B * t.J * 3);
  l.aw.c2j = ar.take<float>((size_t)B * t.J * 3);
  l.aw.g1 = ar.take<float>((size_t)B * t.J * 9);
  l.aw.g2 = ar.take<float>((size_t)B * t.J * 9);
  l.aw.g3 = ar.take<float>((size_t)B * t.J * 9);
  return l;
}

// LAYOUT rotation sweep: what the adjoints of both differentiable fits share.  One region for the calls
// they are made of (each lays out its own workspace in it, one after the other on the stream; sub_bytes: the largest
// of them, the caller's), the rotations of every iteration, and the streams of the reverse sweep
struct SweepLayout {
  char* sub;
  size_t sub_bytes;
  float* G;  // (num_iter, B, J, 9) rotations of every iteration
  float *ctv, *ctj, *mesh, *joints, *rjreg;
  double *psum, *scr;
  FaJointCot jc;
  float *acc_tv, *acc_tj, *meshbar, *jointsbar;
  float *Gbar, *Gbar2, *Gtmp, *xb, *kb, *tb, *xb2, *kb2;
};
SweepLayout sweep_layout(const sf::HostTables& t, int B, int num_iter, size_t sub_bytes, Arena& ar) {
  SweepLayout l;
  l.sub_bytes = sub_bytes;
  l.sub = ar.take<char>(sub_bytes);
  const size_t n = (size_t)std::max(num_iter, 1), BJ = (size_t)B * t.J, BV = (size_t)B * t.V;
  const size_t nb = (size_t)std::max(1, t.num_betas());
  l.G = ar.take<float>(n * BJ * 9);
  l.ctv = ar.take<float>(BV * 3);
  l.ctj = ar.take<float>(BJ * 3);
  l.mesh = ar.take<float>(BV * 3);
  l.joints = ar.take<float>(BJ * 3);
  l.rjreg = ar.take<float>(BJ * 3);
  l.psum = ar.take<double>(BJ * sf::kPsum);
  l.scr = ar.take<double>((size_t)B * sf::fit_tail_adjoint_scratch(t.J));
  l.jc.pbar = ar.take<float>(BJ * sf::kPsum);
  l.jc.tjbar = ar.take<float>(BJ * 3);
  l.jc.rjtbar = ar.take<float>(BJ * 3);
  l.jc.rjbar = ar.take<float>(BJ * 3);
  l.jc.jwbar = ar.take<float>(BJ);
  l.acc_tv = ar.take<float>(BV * 3);
  l.acc_tj = ar.take<float>(BJ * 3);
  l.meshbar = ar.take<float>(BV * 3);
  l.jointsbar = ar.take<float>(BJ * 3);
  l.Gbar = ar.take<float>(BJ * 9);
  l.Gbar2 = ar.take<float>(BJ * 9);
  l.Gtmp = ar.take<float>(BJ * 9);
  l.xb = ar.take<float>(B * nb);
  l.kb = ar.take<float>((size_t)B);
  l.tb = ar.take<float>((size_t)B * 3);
  l.xb2 = ar.take<float>(B * nb);
  l.kb2 = ar.take<float>((size_t)B);
  return l;
}

// LAYOUT adjoint of the fit: the sweep's (in its region: the shape solve, the forward's backward and the shape solve's
// adjoint), then the solution of every iteration, the template's regressed joints, the second translation cotangent
// and the shape-solve adjoint's target and weight gradients
struct FitBackwardLayout {
  SweepLayout sw;
  float *betas, *kid, *trans;  // (num_iter, B, ...) solution of every iteration
  float *rj0, *tb2;
  float *tmp_tv, *tmp_tj, *tmp_vw, *tmp_jw;
};
FitBackwardLayout fit_backward_layout(const sf::HostTables& t, int B, int num_iter, Arena& ar) {
  FitBackwardLayout l;
  Arena sub{nullptr};
  adjoint_layout(t, B, sub);
  l.sw = sweep_layout(t, B, num_iter, std::max(sub.off, chunked_workspace_bytes(t, B)), ar);
  const size_t n = (size_t)std::max(num_iter, 1), BJ = (size_t)B * t.J, BV = (size_t)B * t.V;
  l.betas = ar.take<float>(n * B * std::max(1, t.num_betas()));
  l.kid = ar.take<float>(n * B);
  l.trans = ar.take<float>(n * B * 3);
  l.rj0 = ar.take<float>((size_t)t.J * 3);
  l.tb2 = ar.take<float>((size_t)B * 3);
  l.tmp_tv = ar.take<float>(BV * 3);
  l.tmp_tj = ar.take<float>(BJ * 3);
  l.tmp_vw = ar.take<float>(BV);
  l.tmp_jw = ar.take<float>(BJ);
  return l;
}

// LAYOUT adjoint of the known-shape fit: the sweep's (in its region: the forward and the forward's backward), then the
// alignment's translation
struct KnownShapeBackwardLayout {
  SweepLayout sw;
  float* trans;  // (B, 3)
};
KnownShapeBackwardLayout known_shape_backward_layout(const sf::HostTables& t, int B, int num_iter, Arena& ar) {
  KnownShapeBackwardLayout l;
  Arena sub{nullptr};
  backward_layout(t, B, sub);
  l.sw = sweep_layout(t, B, num_iter, std::max(sub.off, chunked_workspace_bytes(t, B)), ar);
  l.trans = ar.take<float>((size_t)B * 3);
  return l;
}

// LAYOUT flip: the naively flipped pose (B,3J) the warm start reads, then the chunks of the fused conversion's fit
struct FlipLayout {
  float* init_pose;
  char* fit;
};
FlipLayout flip_layout(const smplfit_convert_plan& conv, int B, Arena& ar) {
  FlipLayout l;
  l.init_pose = ar.take<float>((size_t)B * conv.out->t.J * 3);
  l.fit = ar.take<char>(chunked_workspace_bytes(conv.out->t, B, &conv.in->t));
  return l;
}

// LAYOUT hand replacement: the per-instance results of its fit — relative rotations (B,J,9), rotation vectors (B,3J),
// betas (B,S), translation (B,3): the last three stand in for parameter outputs the caller left NULL —, then the
// chunks of the fit (the forward behind it runs in the same bytes, as one fit workspace)
struct ReplaceLayout {
  float *rel, *pose, *betas, *trans;
  char* fit;
};
ReplaceLayout replace_layout(const sf::HostTables& t, int B, Arena& ar) {
  ReplaceLayout l;
  l.rel = ar.take<float>((size_t)B * t.J * 9);
  l.pose = ar.take<float>((size_t)B * t.J * 3);
  l.betas = ar.take<float>((size_t)B * t.num_betas());
  l.trans = ar.take<float>((size_t)B * 3);
  l.fit = ar.take<char>(chunked_workspace_bytes(t, B));
  return l;
}

// LAYOUT fit with reconstruction: the fit's global rotations (B,J,9) and kid factors (B), which stand in for outputs
// the caller left NULL (the mesh-error step reads them), then the fit's own workspace — its chunks, or with a plan of
// segments that call's —, in which the step then runs as one fit workspace
struct ReconLayout {
  float *orient, *kid;
  char* fit;
  size_t fit_bytes;
};
// What the two entries with the mesh-error step check of its four optional outputs before anything is enqueued
int check_recon_outputs(const char* who, const float* vertices, const float* joints, const float* verr, const float* jerr,
                        const float* tv, const float* tj) {
  if (!vertices && !joints && !verr && !jerr)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": at least one of vertices, joints, vertex_error, joint_error is required");
  if (!tv) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": target_vertices is required");
  if (jerr && !tj) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": joint_error needs target_joints");
  return 0;
}
ReconLayout recon_layout(const smplfit_handle* h, int B, const smplfit_share_segments* segments, Arena& ar) {
  ReconLayout l;
  l.orient = ar.take<float>((size_t)B * h->t.J * 9);
  l.kid = ar.take<float>((size_t)B);
  l.fit_bytes = segments ? segments_workspace_bytes(h, *segments) : chunked_workspace_bytes(h->t, B);
  l.fit = ar.take<char>(l.fit_bytes);
  return l;
}

// LAYOUT robust fit: the fit with reconstruction's (the rounds' fits and mesh-error steps run in its fit region), then
// what a round hands to the next: the errors at the previous results (B,V) + (B,J), the weights (B,V) + (B,J) and the
// scales (B) — each of the three only where the caller gave no output buffer for it —, and the previous round's pose
// (B,3J), which the warm fit reads while it writes the caller's
struct RobustLayout {
  ReconLayout rc;
  float *verr, *jerr, *wv, *wj, *sigma, *pose;
};
RobustLayout robust_layout(const smplfit_handle* h, int B, const smplfit_share_segments* segments, bool own_wv, bool own_wj,
                           bool own_sigma, Arena& ar) {
  RobustLayout l{};
  l.rc = recon_layout(h, B, segments, ar);
  const size_t BV = (size_t)B * h->t.V, BJ = (size_t)B * h->t.J;
  l.verr = ar.take<float>(BV);
  l.jerr = ar.take<float>(BJ);
  if (own_wv) l.wv = ar.take<float>(BV);
  if (own_wj) l.wj = ar.take<float>(BJ);
  if (own_sigma) l.sigma = ar.take<float>((size_t)B);
  l.pose = ar.take<float>(BJ * 3);
  return l;
}

// [dfeat | dshape] = dv_posed . [posedirs | shapedirs]^T: the split-K partial products, then their sum in chunk order
void launch_bwd_reduce(const DevModel& d, const BwdWorkspace& bw, int B, hipStream_t st) {
  const int NC = d.P + d.S, nsplit = bwd_nsplit(d.Vp);
  hipLaunchKernelGGL(k_bwd_reduce, dim3((NC + kBwdTile - 1) / kBwdTile, (B + kBwdTile - 1) / kBwdTile, nsplit),
                     dim3(256), 0, st, d, bw, B);
  hipLaunchKernelGGL(k_bwd_combine, dim3((unsigned)(((size_t)B * NC + 255) / 256)), dim3(256), 0, st, bw, B, NC, nsplit);
}

// STEP forward backward.  The vector-Jacobian product of the forward at `in` (nb betas per row), in a laid-out
// BackwardLayout.  With a vertex cotangent: the posed pass recomputed without trans (the joint block (G | t) and
// v_posed), the vertex kernel, the pose-feature / shape reduction; then the joint backward, which writes `out`.
// Where the cotangents come from is all that varies between the callers:
struct Cotangents {
  // from memory (smplfit_forward_backward_f32, the adjoint), each may be null:
  const float *vertices = nullptr, *joints = nullptr, *orient = nullptr;
  // or formed from the objective: the vertex's in registers by k_obj_vertex in place of k_bwd_vertex (trans added
  // there), and — joint term — the joints' by k_obj_joint into its gjoints, loss added behind k_obj_vertex's (stream order)
  const ObjArgs* obj = nullptr;
  const ObjJointArgs* obj_joints = nullptr;
};
struct GradOutputs {
  float *pose, *glob, *rel, *betas, *trans, *kid;  // each may be null; pose / glob / rel: that of the form given
};
template <class A>
GradOutputs grad_outputs(const A& a) {
  return {a.grad_pose_rotvecs, a.grad_glob_rotmats, a.grad_rel_rotmats, a.grad_shape_betas, a.grad_trans, a.grad_kid_factor};
}
int launch_forward_backward(const smplfit_handle* h, const ForwardInputs& in, int nb, const Cotangents& ct,
                            const GradOutputs& out, const BackwardLayout& l, int B, hipStream_t st) {
  const DevModel& d = h->d;
  const Workspace& ws = l.ws;
  const BwdWorkspace& bw = l.bw;
  const bool vertex = ct.vertices || ct.obj;
  if (vertex) {
    // (route_of: Entry::kForwardBackward is never batch-major; these kernels serve every model)
    const ForwardArgs fa = forward_args(in, nb, nullptr, ws.rjoints, nullptr);
    if (int rc = launch_posed_pass(h, route_of(h, B, {Entry::kForwardBackward}), {&fa, {}}, ws, B, st)) return rc;
    if (ct.obj)
      hipLaunchKernelGGL(k_obj_vertex, dim3(B), dim3(256), bwd_vertex_lds_bytes(d, true), st, d, ws, bw, B, nb, in.betas,
                         in.kid, *ct.obj);
    else
      hipLaunchKernelGGL(k_bwd_vertex, dim3(B), dim3(256), bwd_vertex_lds_bytes(d, false), st, d, ws, bw, B, nb, in.betas,
                         in.kid, ct.vertices);
    launch_bwd_reduce(d, bw, B, st);
  }
  if (ct.obj_joints) hipLaunchKernelGGL(k_obj_joint, dim3((B + 63) / 64), dim3(64), 0, st, *ct.obj_joints, B, d.J);
  JointBwdArgs ja{};
  ja.pose = in.pose;
  ja.glob = in.glob;
  ja.rel = in.rel;
  ja.betas = in.betas;
  ja.kid = in.kid;
  ja.nb = nb;
  ja.gjoints = ct.obj_joints ? ct.obj_joints->gjoints : ct.joints;
  ja.gorient = ct.orient;
  ja.vertex = vertex;
  ja.g_pose = out.pose;
  ja.g_glob = out.glob;
  ja.g_rel = out.rel;
  ja.g_betas = out.betas;
  ja.g_trans = out.trans;
  ja.g_kid = out.kid;
  hipLaunchKernelGGL(k_bwd_joint, dim3((B + 63) / 64), dim3(64), 0, st, d, bw, ja, B);
  return 0;
}

// Both objective entry points (A: either argument struct).  jt: the joint term's fields, which only
// smplfit_fit_objective_args has — null for smplfit_mesh_objective_f32, whose workspace is the backward's; the term
// itself runs when target_joints is given.
struct JointTerm {
  const float *target, *weights;
  float scale;
};
template <class A>
int objective_impl(const char* who, const smplfit_handle* h, const A& a, const JointTerm* jt, size_t needed,
                          const char* query) {
  const int B = a.batch;
  if (int rc = check_call(who, h, B, a.workspace, a.workspace_bytes, needed, query)) return rc;
  const DevModel& d = h->d;
  const ForwardInputs in = forward_inputs(a);
  if (int rc = check_forward_inputs(who, d, in)) return rc;
  if (!a.target_vertices) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": target_vertices is required");
  if (jt && jt->weights && !jt->target)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": joint_weights without target_joints");
  if (!a.loss) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": loss output is required");
  Arena ar{(char*)a.workspace};
  ObjectiveLayout l{};
  if (jt) l = objective_layout(h->t, B, ar);
  else l.fb = backward_layout(h->t, B, ar);
  const ObjArgs oa{a.target_vertices, a.vertex_weights, a.trans, a.scale, a.loss};
  ObjJointArgs oj{};
  Cotangents ct;
  ct.obj = &oa;
  if (jt && jt->target) {
    oj = {l.fb.ws.rjoints, a.trans, jt->target, jt->weights, jt->scale, l.gjoints, a.loss};
    ct.obj_joints = &oj;
  }
  if (int rc = launch_forward_backward(h, in, backward_nb(in), ct, grad_outputs(a), l.fb, B, (hipStream_t)a.hip_stream)) return rc;
  return post_launch_check();
}

// STEP rotation sweep, in a laid-out SweepLayout.  tj / vw / jw: the call's target joints and weights, each
// may be null; acc_vw / acc_jw: the caller's weight-gradient outputs or null, accumulated in place.
struct OutputCotangents {
  const float *pose, *orient, *rel, *betas, *kid, *trans;  // the caller's, each may be null
};
struct RotationSweep {
  const smplfit_handle* h;
  SweepLayout l;
  hipStream_t st;
  int B;
  const float *tj, *vw, *jw;
  float *acc_vw, *acc_jw;

  bool joints() const { return tj != nullptr; }
  size_t BJ() const { return (size_t)B * h->d.J; }
  size_t BV() const { return (size_t)B * h->d.V; }
  dim3 lanes() const { return dim3((unsigned)((B + 63) / 64)); }  // the joint-level kernels: one lane per instance
  float* Gk(int k) const { return l.G + (size_t)k * BJ() * 9; }
  void add(float* dst, const float* src, size_t cnt) const {
    hipLaunchKernelGGL(k_fa_add, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, dst, src, cnt);
  }
  // the joints regressed from `rows` meshes (null: the template)
  void regress(int rows, const float* verts, float* out) const {
    hipLaunchKernelGGL(k_fa_regress, dim3(rows), dim3(64), 0, st, h->d, verts, out);
  }
  // the four accumulators zeroed and the targets centred; without target joints they are regressed from the centred
  // vertices, and — rj0 given — the template's once, for against_template
  int begin(const float* tv, float* rj0) const {
    SF_HIP_TRY(hipMemsetAsync(l.acc_tv, 0, BV() * 3 * 4, st));
    SF_HIP_TRY(hipMemsetAsync(l.acc_tj, 0, BJ() * 3 * 4, st));
    if (acc_vw) SF_HIP_TRY(hipMemsetAsync(acc_vw, 0, BV() * 4, st));
    if (acc_jw) SF_HIP_TRY(hipMemsetAsync(acc_jw, 0, BJ() * 4, st));
    hipLaunchKernelGGL(k_fa_center, dim3(B), dim3(256), 0, st, h->d, tv, tj, l.ctv, l.ctj);
    if (!joints()) regress(B, l.ctv, l.ctj);
    if (!joints() && rj0) regress(1, nullptr, rj0);
    return 0;
  }
  // the fp64 part sums of a stage and its reference joints (regressed without target joints): against l.mesh / l.joints, or
  // against the template (rj0: its regressed joints)
  FaJoints part_sums(const float* mesh, const FaJoints& jn) const {
    hipLaunchKernelGGL(k_fa_partsums, dim3(B), dim3(256), 0, st, h->d, (const float*)l.ctv, mesh, vw, l.psum);
    return jn;
  }
  FaJoints against_mesh() const {
    if (!joints()) regress(B, l.mesh, l.rjreg);
    return part_sums(l.mesh, {l.ctj, joints() ? l.joints : l.rjreg, 0, jw});
  }
  FaJoints against_template(const float* rj0) const { return part_sums(nullptr, {l.ctj, joints() ? h->d.j_template : rj0, 1, jw}); }
  // the part-sum adjoint of the records the last joint-level adjoint left; with_mesh: the stage ran against l.mesh, whose
  // cotangent and its joints' go to meshbar / jointsbar
  void vertex_pass(bool with_mesh) const {
    FaVertexArgs va{l.ctv, with_mesh ? l.mesh : nullptr, vw, joints() ? 0 : 1, l.acc_tv, l.acc_tj, acc_vw, acc_jw,
                    with_mesh ? l.meshbar : nullptr, with_mesh ? l.jointsbar : nullptr};
    hipLaunchKernelGGL(k_fa_vertex, dim3(B), dim3(256), 0, st, h->d, va, l.jc);
  }
  // G_k = Rot(stage) G_{k-1} (k = 0: the first pass), and its adjoint: Gbar in; k > 0: G_{k-1}'s written to Gbar2, and the
  // two trade places — Gbar is the cotangent of the rotations the reverse sweep stands at
  void rot_forward(int k, const FaJoints& jn) const {
    hipLaunchKernelGGL(k_fa_rot_fwd, lanes(), dim3(64), 0, st, h->d, (const double*)l.psum, jn,
                       k ? (const float*)Gk(k - 1) : (const float*)nullptr, Gk(k), B);
  }
  void rot_adjoint(int k, const FaJoints& jn) {
    hipLaunchKernelGGL(k_fa_rot_adj, lanes(), dim3(64), 0, st, h->d, (const double*)l.psum, jn,
                       k ? (const float*)Gk(k - 1) : (const float*)nullptr, (const float*)l.Gbar, k ? l.Gbar2 : (float*)nullptr, l.scr, l.jc, B);
    if (k) std::swap(l.Gbar, l.Gbar2);
  }
  // output stage and — refine — refinement at (G_k, betas, kid, trans) against l.mesh / l.joints: Gbar, xb, kb, tb written
  void tail(int k, bool refine, int nb, const float* betas, const float* kid, const float* trans, const OutputCotangents& g) const {
    const FaJoints jn = refine ? against_mesh() : FaJoints{l.ctj, l.ctj, 0, jw};
    FaTailArgs ta{Gk(k), betas, kid, trans, l.joints, refine ? 1 : 0, nb, g.pose, g.orient, g.rel, g.betas, g.kid, g.trans,
                  l.Gbar, l.xb, l.kb, l.tb};
    hipLaunchKernelGGL(k_fa_tail, lanes(), dim3(64), 0, st, h->d, (const double*)l.psum, jn, ta, l.scr, l.jc, B);
    if (refine) vertex_pass(true);
  }
  // meshbar / jointsbar through the forward at (glob or the rest pose, betas, kid) in a laid-out BackwardLayout.  out: the
  // products wanted (Gtmp, xb2, kb2, a second tb of the caller's) or null; each is added to Gbar / xb / kb / tb, the
  // rotations' in front of the others (glob_first) or behind them
  int mesh_cotangent(const float* glob, const float* betas, const float* kid, int nb, const GradOutputs& out, bool glob_first,
                     const BackwardLayout& bl) const {
    const ForwardInputs in{nullptr, glob, nullptr, nb ? betas : nullptr, kid, nb};
    Cotangents ct;
    ct.vertices = l.meshbar;
    ct.joints = l.jointsbar;
    if (int rc = launch_forward_backward(h, in, nb, ct, out, bl, B, st)) return rc;
    if (out.glob && glob_first) add(l.Gbar, out.glob, BJ() * 9);
    if (out.betas) add(l.xb, out.betas, (size_t)B * nb);
    if (out.kid) add(l.kb, out.kid, (size_t)B);
    if (out.trans) add(l.tb, out.trans, (size_t)B * 3);
    if (out.glob && !glob_first) add(l.Gbar, out.glob, BJ() * 9);
    return 0;
  }
  // the accumulated target cotangents back through the centring, into the caller's outputs
  void finish(const float* g_trans, float* g_tv, float* g_tj) const {
    hipLaunchKernelGGL(k_fa_uncenter, dim3(B), dim3(256), 0, st, h->d, (const float*)l.acc_tv,
                       joints() ? (const float*)l.acc_tj : nullptr, g_trans, g_tv, g_tj);
  }
};

// What smplfit_fit_backward_f32 and smplfit_fit_known_shape_backward_f32 both refuse (behind check_call)
int check_sweep_call(const char* who, const smplfit_handle* h, int num_iter, const float* tj, const float* vw, const float* jw,
                     const float* grad_tj, const float* grad_vw, const float* grad_jw) {
  const auto bad = [who](int code, const char* what) { return fail(code, std::string(who) + ": " + what); };
  if (num_iter <= 0) return bad(SMPLFIT_ERR_BAD_ARG, "num_iter must be positive");
  if (h->d.S > sf::kAdjMaxUnknowns) return bad(SMPLFIT_ERR_UNSUPPORTED, "more than 17 shape unknowns");
  if (!tj && !h->t.has_regressor)
    return bad(SMPLFIT_ERR_BAD_ARG, "target_joints omitted but the model has no J_regressor_post_lbs over its vertices");
  if (grad_tj && !tj) return bad(SMPLFIT_ERR_BAD_ARG, "grad_target_joints without target_joints");
  if (grad_vw && !vw) return bad(SMPLFIT_ERR_BAD_ARG, "grad_vertex_weights without vertex_weights");
  if (grad_jw && !jw) return bad(SMPLFIT_ERR_BAD_ARG, "grad_joint_weights without joint_weights");
  return 0;
}

// The adjoint of the fit: the sweep's steps around the shape solve of every iteration and its adjoint
int run_fit_backward(const smplfit_handle* h, const smplfit_fit_backward_args& a) {
  const DevModel& d = h->d;
  const int B = a.batch, n = a.num_iter, nb = h->t.num_betas();
  const float *tj = a.target_joints, *vw = a.vertex_weights, *jw = a.joint_weights;
  const bool joints = tj != nullptr, refine = a.final_adjust_rots != 0, kid = d.jt.n_kid != 0;
  hipStream_t st = (hipStream_t)a.hip_stream;
  Arena ar{(char*)a.workspace};
  const FitBackwardLayout l = fit_backward_layout(h->t, B, n, ar);
  RotationSweep sw{h, l.sw, st, B, tj, vw, jw, a.grad_vertex_weights, a.grad_joint_weights};
  const size_t BJ = sw.BJ(), BV = sw.BV(), nbs = (size_t)std::max(1, nb);
  const auto bk = [&](int k) { return l.betas + (size_t)k * B * nbs; };
  const auto kk = [&](int k) { return kid ? l.kid + (size_t)k * B : nullptr; };
  const auto tk = [&](int k) { return l.trans + (size_t)k * B * 3; };
  // the shape solve at the rotations of iteration k in the frame of the centred targets, as the solve (with the fitted mesh
  // and joints) and its adjoint name it
  const auto at_iteration = [&](auto& s, int k) {
    s.glob_rotmats = sw.Gk(k);
    s.target_vertices = sw.l.ctv;
    s.target_joints = joints ? sw.l.ctj : nullptr;
    s.vertex_weights = vw;
    s.joint_weights = joints ? jw : nullptr;
    s.batch = B;
    s.beta_regularizer = a.beta_regularizer;
    s.beta_regularizer2 = a.beta_regularizer2;
    s.kid_regularizer = a.kid_regularizer;
    s.shape_betas = bk(k);
    s.trans = tk(k);
    s.kid_factor = kk(k);
    s.workspace = sw.l.sub;
    s.workspace_bytes = sw.l.sub_bytes;
    s.hip_stream = a.hip_stream;
  };
  const auto solve = [&](int k, bool mesh) {
    smplfit_shape_solve_args sa{};
    at_iteration(sa, k);
    sa.vertices_out = mesh ? sw.l.mesh : nullptr;
    sa.joints_out = mesh ? sw.l.joints : nullptr;
    return smplfit_shape_solve_ex_f32(h, &sa);
  };
  // ---- forward sweep: the rotations and the solution of every iteration
  if (int rc = sw.begin(a.target_vertices, l.rj0)) return rc;
  sw.rot_forward(0, sw.against_template(l.rj0));
  for (int k = 0; k < n; ++k) {
    if (int rc = solve(k, k + 1 < n)) return rc;
    if (k + 1 < n) sw.rot_forward(k + 1, sw.against_mesh());
  }
  // ---- reverse sweep.  Output stage and refinement at the last iteration ...
  if (refine)
    if (int rc = solve(n - 1, true)) return rc;
  sw.tail(n - 1, refine, nb, bk(n - 1), kk(n - 1), tk(n - 1),
          {a.grad_pose_rotvecs, a.grad_orientations, a.grad_relative_orientations, a.grad_shape_betas,
           kid ? a.grad_kid_factor : nullptr, a.grad_trans});
  Arena sub{sw.l.sub};
  const AdjointLayout al = adjoint_layout(h->t, B, sub);
  bool mesh_cot = refine;
  for (int k = n - 1; k >= 0; --k) {
    // ... the mesh cotangent through the forward at (G_k, x_k, t_k) ...
    if (mesh_cot) {
      GradOutputs out{};
      out.glob = sw.l.Gtmp;
      out.betas = nb ? sw.l.xb2 : nullptr;
      out.trans = l.tb2;
      out.kid = kid ? sw.l.kb2 : nullptr;
      if (int rc = sw.mesh_cotangent(sw.Gk(k), bk(k), kk(k), nb, out, true, al.fb)) return rc;
    }
    // ... the adjoint of the shape solve: the targets' and weights' gradients and its share of the rotations' ...
    smplfit_shape_solve_backward_args sb{};
    at_iteration(sb, k);
    sb.grad_shape_betas = sw.l.xb;
    sb.grad_trans = sw.l.tb;
    sb.grad_kid_factor = kid ? sw.l.kb : nullptr;
    sb.grad_target_vertices = l.tmp_tv;
    sb.grad_target_joints = joints ? l.tmp_tj : nullptr;
    sb.grad_vertex_weights = sw.acc_vw ? l.tmp_vw : nullptr;
    sb.grad_joint_weights = (sw.acc_jw && joints) ? l.tmp_jw : nullptr;
    sb.grad_glob_rotmats = sw.l.Gtmp;
    if (int rc = smplfit_shape_solve_backward_f32(h, &sb)) return rc;
    sw.add(sw.l.acc_tv, l.tmp_tv, BV * 3);
    if (joints) sw.add(sw.l.acc_tj, l.tmp_tj, BJ * 3);
    if (sb.grad_vertex_weights) sw.add(sw.acc_vw, l.tmp_vw, BV);
    if (sb.grad_joint_weights) sw.add(sw.acc_jw, l.tmp_jw, BJ);
    sw.add(sw.l.Gbar, sw.l.Gtmp, BJ * 9);
    // ... and the rotation pass that made G_k: against the template (k = 0), or against the mesh of iteration k - 1
    if (k == 0) {
      sw.rot_adjoint(0, sw.against_template(l.rj0));
      sw.vertex_pass(false);
    } else {
      if (int rc = solve(k - 1, true)) return rc;
      sw.rot_adjoint(k, sw.against_mesh());
      sw.vertex_pass(true);
      SF_HIP_TRY(hipMemsetAsync(sw.l.xb, 0, (size_t)B * nbs * 4, st));
      SF_HIP_TRY(hipMemsetAsync(sw.l.kb, 0, (size_t)B * 4, st));
      SF_HIP_TRY(hipMemsetAsync(sw.l.tb, 0, (size_t)B * 3 * 4, st));
      mesh_cot = true;
    }
  }
  sw.finish(a.grad_trans, a.grad_target_vertices, a.grad_target_joints);
  return post_launch_check();
}

// The adjoint of the known-shape fit: the sweep's steps around the forward at the given shape, the
// alignment with its adjoint, and the copy-out of the shape gradient
int run_known_shape_backward(const smplfit_handle* h, const smplfit_fit_known_shape_backward_args& a) {
  const DevModel& d = h->d;
  const int B = a.batch, n = a.num_iter, nb = a.num_betas_given;
  const float *tj = a.target_joints, *vw = a.vertex_weights, *jw = a.joint_weights, *kid = a.kid_factor;
  const bool joints = tj != nullptr, refine = a.final_adjust_rots != 0;
  const bool shape_grads = (a.grad_shape_betas && nb) || a.grad_kid_factor;
  hipStream_t st = (hipStream_t)a.hip_stream;
  Arena ar{(char*)a.workspace};
  const KnownShapeBackwardLayout l = known_shape_backward_layout(h->t, B, n, ar);
  RotationSweep sw{h, l.sw, st, B, tj, vw, jw, a.grad_vertex_weights, a.grad_joint_weights};
  // the model at the given shape and the rotations of iteration k (k < 0: the rest pose), without trans: mesh and joints
  const auto forward = [&](int k) {
    smplfit_forward_args fa{};
    fa.glob_rotmats = k < 0 ? nullptr : sw.Gk(k);
    fa.shape_betas = a.shape_betas;
    fa.num_betas_given = nb;
    fa.kid_factor = kid;
    fa.batch = B;
    fa.vertices = sw.l.mesh;
    fa.joints = sw.l.joints;
    fa.workspace = sw.l.sub;
    fa.workspace_bytes = sw.l.sub_bytes;
    fa.hip_stream = a.hip_stream;
    return smplfit_forward_ex_f32(h, &fa);
  };
  // the cotangents of the mesh and its joints through that forward: Gbar += (with rotations), xb +=, kb +=
  Arena sub{sw.l.sub};
  const BackwardLayout bl = backward_layout(h->t, B, sub);
  const auto mesh_cotangent = [&](int k) {
    GradOutputs out{};
    out.glob = k < 0 ? nullptr : sw.l.Gtmp;
    out.betas = (shape_grads && nb) ? sw.l.xb2 : nullptr;
    out.kid = (shape_grads && kid) ? sw.l.kb2 : nullptr;
    return sw.mesh_cotangent(k < 0 ? nullptr : sw.Gk(k), a.shape_betas, kid, nb, out, false, bl);
  };
  // ---- forward sweep: the rotations of every iteration, then the alignment at the last mesh
  if (int rc = sw.begin(a.target_vertices, nullptr)) return rc;
  for (int k = 0; k < n; ++k) {
    if (int rc = forward(k - 1)) return rc;
    sw.rot_forward(k, sw.against_mesh());
  }
  if (int rc = forward(n - 1)) return rc;
  const SolveWeights w = solve_weights(joints, vw, jw);
  const FaAlign al{sw.l.ctv, joints ? sw.l.ctj : nullptr, w.v ? vw : nullptr, w.j ? jw : nullptr};
  hipLaunchKernelGGL(k_fa_align, dim3(B), dim3(256), 0, st, d, al, sw.l.mesh, sw.l.joints, l.trans);
  // ---- reverse sweep.  Output stage and refinement against the aligned mesh (without it its cotangent is zero) ...
  sw.tail(n - 1, refine, nb, a.shape_betas, kid, l.trans,
          {a.grad_pose_rotvecs, a.grad_orientations, a.grad_relative_orientations, nullptr, nullptr, a.grad_trans});
  if (!refine) {
    SF_HIP_TRY(hipMemsetAsync(sw.l.meshbar, 0, sw.BV() * 3 * 4, st));
    SF_HIP_TRY(hipMemsetAsync(sw.l.jointsbar, 0, sw.BJ() * 3 * 4, st));
  }
  // ... the alignment: the complete tbar, its share of the targets, the weights and the mesh ...
  const FaAlignAdj aa{al, sw.l.mesh, sw.l.joints, sw.l.meshbar, sw.l.jointsbar, sw.l.tb, sw.l.acc_tv, sw.l.acc_tj,
                      w.v ? sw.acc_vw : nullptr, w.j ? sw.acc_jw : nullptr};
  hipLaunchKernelGGL(k_fa_align_adj, dim3(B), dim3(256), 0, st, d, aa);
  // ... the whole cotangent of the last mesh through the forward at (G_{n-1}, betas) ...
  if (int rc = mesh_cotangent(n - 1)) return rc;
  // ... and the rotation passes: G_k = Rot(targets, mesh_k) G_{k-1}, mesh_k the forward at G_{k-1} (k = 0: the rest pose)
  for (int k = n - 1; k >= 0; --k) {
    if (int rc = forward(k - 1)) return rc;
    sw.rot_adjoint(k, sw.against_mesh());
    sw.vertex_pass(true);
    if (k == 0 && !shape_grads) break;  // (the cotangent of mesh_0 reaches the shape alone)
    if (int rc = mesh_cotangent(k - 1)) return rc;
  }
  if (a.grad_shape_betas && nb)
    SF_HIP_TRY(hipMemcpyAsync(a.grad_shape_betas, sw.l.xb, (size_t)B * nb * 4, hipMemcpyDeviceToDevice, st));
  if (a.grad_kid_factor) SF_HIP_TRY(hipMemcpyAsync(a.grad_kid_factor, sw.l.kb, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  sw.finish(a.grad_trans, a.grad_target_vertices, a.grad_target_joints);
  return post_launch_check();
}

}  // namespace

// ================================================================================================
// C-ABI
// ================================================================================================
extern "C" {

const char* smplfit_last_error(void) { return g_last_error.c_str(); }
#ifndef SMPLFIT_BUILD_ID
#define SMPLFIT_BUILD_ID "unknown"
#endif
const char* smplfit_version(void) { return "smplfit-hip 0.4 (gfx950) build " SMPLFIT_BUILD_ID; }
int smplfit_abi_version(void) { return SMPLFIT_ABI_VERSION; }

int smplfit_create(const smplfit_model_desc* desc, int flags, smplfit_handle** out) {
  if (!desc || !out) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_create: null argument");
  *out = nullptr;
  smplfit_handle* h = new smplfit_handle();
  bool unsupported = false;
  std::string err = sf::build_tables(*desc, h->t, &unsupported);
  if (!err.empty()) {
    delete h;
    return fail(unsupported ? SMPLFIT_ERR_UNSUPPORTED : SMPLFIT_ERR_BAD_ARG, err);
  }
  if (!h->t.general && h->t.S + 3 > 3 * h->t.J) {
    delete h;
    return fail(SMPLFIT_ERR_UNSUPPORTED, "smplfit_create: num_betas too large for this joint count");
  }
  if (flags & SMPLFIT_CREATE_HOST_ONLY) {
    *out = h;
    return SMPLFIT_OK;
  }
  // stage images of the tiled split-bf16 GEMM (94 MB for SMPL-X): only for a model whose fits can take the
  // batch-major path (the only launches that read them; the structural part of route_of's batch-major rule)
  if ((h->t.KW == 4 || h->t.KW == 8) && sf::bm_shape_count(h->t.S) && h->t.wsum_dev <= 1e-5f)
    sf::build_tiled_gemm_images(h->t);
  const sf::HostTables& t = h->t;
  DevModel& d = h->d;
  d.V = t.V; d.J = t.J; d.S = t.S; d.P = t.P; d.Vp = t.Vp; d.Kp = t.Kp; d.KW = t.KW;
  d.n_used = t.n_used;
  d.nseg = (int)t.segments.size();
  d.nsegall = (int)t.segments_all.size();
  d.ngt = (int)t.gtiles.size();
  d.kc32 = t.kc32;
  d.general = t.general ? 1 : 0;
  d.bm_tables = t.shares.empty() ? 0 : 1;
  // every table the kernels read, as sf_tables.cpp made it: the first failed upload is the call's error
  int rc = 0;
  auto up = [&](const auto& vec, auto* dst) {
    if (rc == 0) rc = h->dev.upload(vec, dst);
  };
  up(sf::flatten(t.segments_all), &d.segall);
  up(t.sdg, &d.sdg);
  up(t.perm, &d.perm);
  up(sf::flatten(t.segments), &d.segments);
  up(t.part_seg_start, &d.part_seg_start);
  up(t.vt, &d.vt);
  up(t.dm, &d.dm);
  up(t.sd, &d.sd);
  up(t.wval, &d.wval);
  up(t.widx, &d.widx);
  up(t.pdSw, &d.pdSw);
  up(t.pdB, &d.pdB);
  up(t.pdB2, &d.pdB2);
  std::vector<uint16_t>().swap(h->t.pdB2);  // the host copy of the stage images is not needed any more
  up(t.cpackA, &d.cpackA);
  up(t.cpackB, &d.cpackB);
  up(t.gblob, &d.gblob);
  up(sf::flatten(t.gtiles), &d.gtiles);
  up(t.j_template, &d.j_template);
  up(t.reg_start, &d.reg_start);
  up(t.reg_slot, &d.reg_slot);
  up(t.reg_val, &d.reg_val);
  up(t.reg_rowsum, &d.reg_rowsum);
  up(t.inv_slot, &d.inv_slot);
  h->views.assign(t.shares.size(), ShareView{});  // the share tables of the batch-major vertex kernels: (coarse, fine) x kinds
  for (size_t i = 0; i < t.shares.size(); ++i) {
    const sf::ShareTable& stb = t.shares[i];
    ShareView& sv = h->views[i];
    sv.ncells = stb.ncells;
    sv.nrows = stb.nrows;
    sv.rec = stb.rec;
    sv.mult = 1;
    sv.max_aux = stb.max_aux;
    sv.aux_pitch = stb.aux_pitch;
    up(stb.piece_start, &sv.piece_start);
    up(stb.pieces, &sv.pieces);
    up(stb.aux_start, &sv.aux_start);
    up(stb.aux_rows, &sv.aux_rows);
    if (!stb.aux_pad.empty()) up(stb.aux_pad, &sv.aux_pad);  // (residual tables only)
  }
  up(t.brec, &d.brec);
  up(t.pair_E, &d.pair_E);
  up(t.jn_start, &d.jn_start);
  up(t.jn, &d.jn);
  up(t.anc_start, &d.anc_start);
  up(t.anc, &d.anc);
  up(t.pair_c2e, &d.pair_c2e);
  up(t.diag_c2e, &d.diag_c2e);
  d.jt = sf::bind_joint_tabs(t, [&](const auto& vec) {
    decltype(vec.data()) p = nullptr;
    up(vec, &p);
    return p;
  });
  if (rc != 0) {
    smplfit_destroy(h);
    return rc;
  }
  {
    int regs = 1 << 20;
    std::vector<const void*> fns{reinterpret_cast<const void*>(&k_posedirs_gemm_bf16x3<true, false>),
                                 reinterpret_cast<const void*>(&k_posedirs_gemm_bf16x3<false, false>),
                                 reinterpret_cast<const void*>(&k_posedirs_gemm_bf16x3_tiled)};
    if constexpr (sf::kGemm3) fns.push_back(reinterpret_cast<const void*>(&k_posedirs_gemm_bf16x3<true, true>));
    for (const void* fn : fns) {
      hipFuncAttributes fa{};
      regs = std::min(regs, hipFuncGetAttributes(&fa, fn) == hipSuccess ? fa.numRegs : 0);
    }
    h->gemm_vgprs = regs;
    d.gemm_exclusive = regs >= 256 ? 1 : 0;
    // the A-stationary split kernel (Kp == 208) gives the bias row its third term in the LAST k-step, where SMPL's
    // 207 pose features put it; a model with Kp == 208 whose bias row sits elsewhere takes the fp32-MFMA GEMM
    if (sf::kGemm3 && t.Kp == 208 && sf::rp_pos(t.P, t.Kp) / 16 != kGemmKS - 1) d.gemm_exclusive = 0;
    if (!d.gemm_exclusive && !tune().gemm_f32) {  // said once per process: every fit of this handle takes the ~3x slower GEMM
      static std::once_flag warned;
      const int regs_now = regs;
      std::call_once(warned, [regs_now] {
        std::fprintf(stderr, "smplfit: the split-bf16 posedirs GEMM is disabled for this model (kernel registers %d < 256 or a "
                             "bias row outside the last k-step): using the fp32-MFMA GEMM (smplfit_info.gemm_vgprs)\n", regs_now);
      });
    }
  }
  // side streams + events of the chunked fit
  for (int i = 0; i < kMaxChunks - 1; ++i) {
    if (hipStreamCreateWithFlags(&h->side[i], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming) != hipSuccess) {
      smplfit_destroy(h);
      return fail(SMPLFIT_ERR_HIP, "smplfit_create: could not create side streams");
    }
  }
  if (hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) {
    smplfit_destroy(h);
    return fail(SMPLFIT_ERR_HIP, "smplfit_create: could not create events");
  }
  h->have_streams = true;
  h->has_device = true;
  *out = h;
  return SMPLFIT_OK;
}

void smplfit_destroy(smplfit_handle* h) {
  if (!h) return;
  for (int i = 0; i < kMaxChunks - 1; ++i) {
    if (h->side[i]) {
      (void)hipStreamSynchronize(h->side[i]);
      (void)hipStreamDestroy(h->side[i]);
    }
    if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  h->dev.free_all();
  delete h;
}

int smplfit_get_info(const smplfit_handle* h, smplfit_info* info) {
  if (!h || !info) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_get_info: null argument");
  const sf::HostTables& t = h->t;
  info->num_vertices = t.V;
  info->num_joints = t.J;
  info->num_betas = t.num_betas();
  info->has_kid = t.n_kid;
  info->padded_vertices = t.Vp;
  info->num_used_vertices = t.n_used;
  info->skin_width = t.KW;
  info->num_segments = (int)t.segments.size();
  info->num_fk_levels = t.num_levels();
  info->adj_last_level = t.adj_last_level;
  info->has_device = h->has_device ? 1 : 0;
  info->gemm_vgprs = h->gemm_vgprs;
  // (the path of a default fit; whether it is batch-major does not depend on the batch)
  info->vertex_path = t.general ? SMPLFIT_PATH_GENERAL : route_of(h, 1, CallShape{}).bm ? SMPLFIT_PATH_BATCH_MAJOR : SMPLFIT_PATH_WAVE;
  info->share_fallback = t.share_fallback;
  return SMPLFIT_OK;
}

int smplfit_get_table(const smplfit_handle* h, int table_id, int32_t* dst, size_t cap, size_t* n) {
  if (!h || !n) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_get_table: null argument");
  const sf::HostTables& t = h->t;
  std::vector<int32_t> tmp;
  const std::vector<int32_t>* src = nullptr;
  switch (table_id) {
    case SMPLFIT_TAB_PART_ASSIGNMENT: src = &t.part_assignment; break;
    case SMPLFIT_TAB_SORT_PERM: src = &t.perm; break;
    case SMPLFIT_TAB_PART_TYPE: src = &t.part_type; break;
    case SMPLFIT_TAB_FK_ORDER: src = &t.fk_js; break;
    case SMPLFIT_TAB_FK_LEVEL_START: src = &t.fk_level_start; break;
    case SMPLFIT_TAB_ADJ_FLAG: src = &t.adj_flag; break;
    case SMPLFIT_TAB_USED_PART: src = &t.used_part; break;
    case SMPLFIT_TAB_SEGMENTS:
      tmp = sf::flatten(t.segments);
      src = &tmp;
      break;
    case SMPLFIT_TAB_VERTEX_PIECES:
      for (auto& g : t.vpieces) {
        tmp.push_back(g.start);
        tmp.push_back(g.count);
        tmp.push_back(g.part);
        tmp.push_back(g.used);
        tmp.push_back(g.nj);
      }
      src = &tmp;
      break;
    case SMPLFIT_TAB_JOINT_PAIRS: src = &t.pair_j; break;
    case SMPLFIT_TAB_CELL_COUNTS:
      for (auto& st : t.shares) tmp.push_back(st.ncells);
      src = &tmp;
      break;
    case SMPLFIT_TAB_INV_SLOT: src = &t.inv_slot; break;
    case SMPLFIT_TAB_PART_SEG_START: src = &t.part_seg_start; break;
    case SMPLFIT_TAB_ANC_START: src = &t.anc_start; break;
    case SMPLFIT_TAB_ANC: src = &t.anc; break;
    case SMPLFIT_TAB_ROT_SLOTS:
      tmp.assign(t.rot_slots, t.rot_slots + t.J);
      src = &tmp;
      break;
    case SMPLFIT_TAB_REFINE_WAVES:
      if (t.adj_parts.size() <= (size_t)sf::kRefMaxAdj) tmp.assign(t.refine_waves, t.refine_waves + t.adj_parts.size());
      src = &tmp;
      break;
    default: return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_get_table: unknown table id");
  }
  *n = src->size();
  if (dst && !src->empty()) std::memcpy(dst, src->data(), std::min(cap, src->size()) * sizeof(int32_t));
  return SMPLFIT_OK;
}

int smplfit_get_share_table(const smplfit_handle* h, int kind, int what, int32_t* dst, size_t cap, size_t* n) {
  if (!h || !n) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_get_share_table: null argument");
  const sf::HostTables& t = h->t;
  if (kind < 0 || kind >= (int)t.shares.size() || what < 0 || what > 5)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_get_share_table: unknown kind / table (or a model without batch-major tables)");
  const sf::ShareTable& st = t.shares[kind];
  const std::vector<int32_t>* const tabs[] = {&st.piece_start, &st.pieces,
                                              kind % sf::kShareKinds == sf::kShareResidual ? &st.row_joints : &st.row_part,
                                              &st.aux_start, &st.aux_rows, &st.aux_pad};
  const std::vector<int32_t>* src = tabs[what];
  *n = src->size();
  if (dst && !src->empty()) std::memcpy(dst, src->data(), std::min(cap, src->size()) * sizeof(int32_t));
  return SMPLFIT_OK;
}

int smplfit_pick_share_mult(const smplfit_handle* h, int kind, int batch) {
  if (!h || h->t.shares.empty() || kind < 0 || kind >= sf::kShareKinds || batch <= 0) return -1;
  return sf::pick_share_mult(h->t, share_index(kind, batch), (int)align_up((size_t)batch, 128) / 64, tune().share_slots);
}

size_t smplfit_workspace_bytes(const smplfit_handle* h, int batch) {
  if (!h || batch <= 0) return 0;
  return chunked_workspace_bytes(h->t, batch);
}

// ---- segments of a share_beta batch -----------------------------------------------------------------
int smplfit_share_segments_create(const int32_t* sizes, int32_t count, int32_t flags, smplfit_share_segments** out) {
  if (!sizes || !out) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_share_segments_create: null argument");
  *out = nullptr;
  auto* p = new smplfit_share_segments();
  const std::string err = sf::build_share_segments(sizes, count, p->t);
  if (!err.empty()) {
    delete p;
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_share_segments_create: " + err);
  }
  if (!(flags & SMPLFIT_CREATE_HOST_ONLY)) {
    if (p->dev.upload(p->t.row_seg, &p->d_row_seg) || p->dev.upload(p->t.seg_blk, &p->d_seg_blk) ||
        p->dev.upload(p->t.blk_rows, &p->d_blk_rows)) {
      smplfit_share_segments_destroy(p);
      return fail(SMPLFIT_ERR_HIP, "smplfit_share_segments_create: device upload failed");
    }
    p->has_device = true;
  }
  *out = p;
  return SMPLFIT_OK;
}

void smplfit_share_segments_destroy(smplfit_share_segments* p) {
  if (!p) return;
  p->dev.free_all();
  delete p;
}

int32_t smplfit_share_segments_batch(const smplfit_share_segments* p) { return p ? p->t.batch : 0; }

int smplfit_share_segments_get_table(const smplfit_share_segments* p, int what, int32_t* dst, size_t cap, size_t* n) {
  if (!p || !n) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_share_segments_get_table: null argument");
  const std::vector<int32_t>* const tabs[] = {&p->t.row_seg, &p->t.seg_blk, &p->t.blk_rows};
  if (what < 0 || what > 2) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_share_segments_get_table: unknown table");
  const std::vector<int32_t>* src = tabs[what];
  *n = src->size();
  if (dst && !src->empty()) std::memcpy(dst, src->data(), std::min(cap, src->size()) * sizeof(int32_t));
  return SMPLFIT_OK;
}

size_t smplfit_share_segments_workspace_bytes(const smplfit_handle* h, int batch, const smplfit_share_segments* p) {
  if (!p) return smplfit_workspace_bytes(h, batch);
  if (!h || batch <= 0 || batch != p->t.batch) return 0;
  return segments_workspace_bytes(h, *p);
}

int smplfit_fit_f32(const smplfit_handle* h, const float* target_vertices,
                    const float* target_joints, const float* vertex_weights,
                    const float* joint_weights, int batch, int num_iter, float beta_regularizer,
                    float beta_regularizer2, float kid_regularizer, int final_adjust_rots,
                    float* pose_rotvecs, float* shape_betas, float* trans, float* kid_factor,
                    float* orientations, float* relative_orientations, void* workspace,
                    size_t workspace_bytes, void* hip_stream) {
  return smplfit_fit_warm_f32(h, target_vertices, target_joints, vertex_weights, joint_weights, batch,
                              num_iter, beta_regularizer, beta_regularizer2, kid_regularizer,
                              final_adjust_rots, nullptr, nullptr, 0, nullptr, pose_rotvecs, shape_betas,
                              trans, kid_factor, orientations, relative_orientations, workspace,
                              workspace_bytes, hip_stream);
}

int smplfit_fit_warm_f32(const smplfit_handle* h, const float* target_vertices,
                         const float* target_joints, const float* vertex_weights,
                         const float* joint_weights, int batch, int num_iter, float beta_regularizer,
                         float beta_regularizer2, float kid_regularizer, int final_adjust_rots,
                         const float* initial_pose_rotvecs, const float* initial_shape_betas,
                         int num_initial_betas, const float* initial_kid_factor, float* pose_rotvecs,
                         float* shape_betas, float* trans, float* kid_factor, float* orientations,
                         float* relative_orientations, void* workspace, size_t workspace_bytes,
                         void* hip_stream) {
  smplfit_fit_args a{};
  a.target_vertices = target_vertices; a.target_joints = target_joints;
  a.vertex_weights = vertex_weights; a.joint_weights = joint_weights;
  a.batch = batch; a.num_iter = num_iter;
  a.beta_regularizer = beta_regularizer; a.beta_regularizer2 = beta_regularizer2;
  a.kid_regularizer = kid_regularizer; a.final_adjust_rots = final_adjust_rots;
  a.initial_pose_rotvecs = initial_pose_rotvecs; a.initial_shape_betas = initial_shape_betas;
  a.num_initial_betas = num_initial_betas; a.initial_kid_factor = initial_kid_factor;
  a.pose_rotvecs = pose_rotvecs; a.shape_betas = shape_betas; a.trans = trans; a.kid_factor = kid_factor;
  a.orientations = orientations; a.relative_orientations = relative_orientations;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.hip_stream = hip_stream;
  return smplfit_fit_ex_f32(h, &a);
}

int smplfit_fit_ex_f32(const smplfit_handle* h, const smplfit_fit_args* args) { return smplfit_fit_segments_f32(h, args, nullptr); }

int smplfit_fit_segments_f32(const smplfit_handle* h, const smplfit_fit_args* args, const smplfit_share_segments* segments) {
  if (!args) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_ex_f32: null arguments");
  if (int rc = check_segments("smplfit_fit_segments_f32", segments, args->batch, args->share_allreduce)) return rc;
  if (int rc = check_call("smplfit_fit_f32", h, args->batch, args->workspace, args->workspace_bytes,
                          smplfit_share_segments_workspace_bytes(h, args->batch, segments),
                          segments ? "smplfit_share_segments_workspace_bytes" : "smplfit_workspace_bytes"))
    return rc;
  if (!segments) return fit_impl(h, args, nullptr);
  smplfit_fit_args a = *args;
  a.share_beta = 1;  // segments imply shared shapes within them
  return fit_impl(h, &a, nullptr, false, segments);
}

int smplfit_fit_known_shape_f32(const smplfit_handle* h, const float* shape_betas,
                                int num_betas_given, const float* kid_factor,
                                const float* initial_pose_rotvecs, const float* target_vertices,
                                const float* target_joints, const float* vertex_weights,
                                const float* joint_weights, int batch, int num_iter,
                                int final_adjust_rots, int scale_fit, float* pose_rotvecs, float* trans,
                                float* scale_corr, float* orientations, float* relative_orientations,
                                void* workspace, size_t workspace_bytes, void* hip_stream) {
  int rc = check_call("smplfit_fit_known_shape_f32", h, batch, workspace, workspace_bytes, smplfit_workspace_bytes(h, batch),
                      "smplfit_workspace_bytes");
  if (rc) return rc;
  if (!shape_betas || !target_vertices || !pose_rotvecs || !trans)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_known_shape_f32: null input/output pointer");
  if (num_iter < 1) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_known_shape_f32: num_iter must be >= 1");
  if (scale_fit && !scale_corr)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_known_shape_f32: scale_fit needs the scale_corr output");
  const sf::HostTables& t = h->t;
  if (kid_factor && !t.n_kid)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_known_shape_f32: kid_factor given to a handle without kid");
  if (num_betas_given < 0 || num_betas_given > t.num_betas())
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_known_shape_f32: more betas than the model holds; slice first");
  KnownShapeOptions o{num_iter, final_adjust_rots ? 1 : 0, scale_fit ? 1 : 0};
  hipStream_t st = (hipStream_t)hip_stream;
  const Workspace ws = fit_workspace(h, batch, workspace);
  return run_fit_known_shape(h, shape_betas, num_betas_given, kid_factor, initial_pose_rotvecs,
                             target_vertices, target_joints, vertex_weights, joint_weights, batch, o,
                             pose_rotvecs, trans, scale_corr, orientations, relative_orientations, ws, st);
}

int smplfit_part_rotations_f32(const smplfit_handle* h, const float* target_vertices,
                               const float* target_joints, const float* vertex_weights,
                               const float* joint_weights, int batch, float* glob_rotmats,
                               void* workspace, size_t workspace_bytes, void* hip_stream) {
  int rc = check_call("smplfit_part_rotations_f32", h, batch, workspace, workspace_bytes, smplfit_workspace_bytes(h, batch),
                      "smplfit_workspace_bytes");
  if (rc) return rc;
  if (!target_vertices || !glob_rotmats)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_part_rotations_f32: null pointer");
  const Workspace ws = fit_workspace(h, batch, workspace);
  smplfit_fit_args a{};  // one rotation pass; the rotations go to the orientations
  a.target_vertices = target_vertices; a.target_joints = target_joints;
  a.vertex_weights = vertex_weights; a.joint_weights = joint_weights;
  a.batch = batch; a.num_iter = 1;
  a.orientations = glob_rotmats;
  return run_fit(h, a, true, nullptr, ws, (hipStream_t)hip_stream);
}

int smplfit_forward_f32(const smplfit_handle* h, const float* pose_rotvecs,
                        const float* glob_rotmats, const float* shape_betas, int num_betas_given,
                        const float* trans, const float* kid_factor, int batch, float* vertices,
                        float* joints, float* orientations, void* workspace, size_t workspace_bytes,
                        void* hip_stream) {
  smplfit_forward_args a{};
  a.pose_rotvecs = pose_rotvecs; a.glob_rotmats = glob_rotmats; a.shape_betas = shape_betas;
  a.num_betas_given = num_betas_given; a.trans = trans; a.kid_factor = kid_factor; a.batch = batch;
  a.vertices = vertices; a.joints = joints; a.orientations = orientations;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.hip_stream = hip_stream;
  return smplfit_forward_ex_f32(h, &a);
}

int smplfit_forward_ex_f32(const smplfit_handle* h, const smplfit_forward_args* args) {
  if (!args) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_forward_ex_f32: null arguments");
  const int batch = args->batch;
  int rc = check_call("smplfit_forward_f32", h, batch, args->workspace, args->workspace_bytes, smplfit_workspace_bytes(h, batch),
                      "smplfit_workspace_bytes");
  if (rc) return rc;
  const DevModel& d = h->d;
  const ForwardInputs in = forward_inputs(*args);
  if ((rc = check_forward_inputs("smplfit_forward_f32", d, in))) return rc;
  if (!args->joints) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_forward_f32: joints output is required");
  hipStream_t st = (hipStream_t)args->hip_stream;
  const Workspace ws = fit_workspace(h, batch, args->workspace);
  const ForwardArgs fa = forward_args(in, forward_nb(d, in), args->trans, args->joints, args->orientations);
  launch_forward_joint(d, fa, ws, batch, st);
  if (args->vertices)  // the mesh at the same inputs, to the caller's (B, V, 3)
    if ((rc = launch_posed_pass(h, route_of(h, batch, {Entry::kForward}), {nullptr, mesh_alone(&fa, args->vertices)}, ws, batch, st))) return rc;
  return post_launch_check();
}

size_t smplfit_forward_backward_workspace_bytes(const smplfit_handle* h, int batch) {
  if (!h || batch <= 0) return 0;
  Arena ar{nullptr};
  backward_layout(h->t, batch, ar);
  return ar.off;
}

int smplfit_forward_backward_f32(const smplfit_handle* h, const smplfit_forward_backward_args* a) {
  const char* who = "smplfit_forward_backward_f32";
  if (!a) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null arguments");
  const int B = a->batch;
  if (int rc = check_call(who, h, B, a->workspace, a->workspace_bytes, smplfit_forward_backward_workspace_bytes(h, B),
                          "smplfit_forward_backward_workspace_bytes"))
    return rc;
  const ForwardInputs in = forward_inputs(*a);
  if (int rc = check_forward_inputs(who, h->d, in)) return rc;
  Arena ar{(char*)a->workspace};
  const BackwardLayout l = backward_layout(h->t, B, ar);
  Cotangents ct;
  ct.vertices = a->grad_vertices;
  ct.joints = a->grad_joints;
  ct.orient = a->grad_orientations;
  if (int rc = launch_forward_backward(h, in, backward_nb(in), ct, grad_outputs(*a), l, B, (hipStream_t)a->hip_stream)) return rc;
  return post_launch_check();
}

// ---- BodyModel.rototranslate: one launch, no workspace (rigid_inputs) ----------------------------------
int smplfit_rototranslate_f32(const smplfit_handle* h, const smplfit_rototranslate_args* a) {
  const char* who = "smplfit_rototranslate_f32";
  if (!a) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null arguments");
  RigidInputs in;
  if (int rc = rigid_inputs(who, h, *a, &in)) return rc;
  if (!a->new_pose_rotvecs || !a->new_trans) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null output pointer");
  const int B = a->batch;
  if (B == 0) return 0;
  hipLaunchKernelGGL(k_rototranslate, dim3((B + kRigidBlock - 1) / kRigidBlock), dim3(kRigidBlock), 0,
                     (hipStream_t)a->hip_stream, in, a->new_pose_rotvecs, a->new_trans, B);
  return post_launch_check();
}

int smplfit_rototranslate_backward_f32(const smplfit_handle* h, const smplfit_rototranslate_backward_args* a) {
  const char* who = "smplfit_rototranslate_backward_f32";
  if (!a) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null arguments");
  RigidInputs in;
  if (int rc = rigid_inputs(who, h, *a, &in)) return rc;
  if (a->grad_kid_factor && !h->d.jt.n_kid)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": grad_kid_factor asked of a handle without kid");
  const int B = a->batch;
  if (B == 0) return 0;
  RigidGrads g{};
  g.g_pose = a->grad_new_pose_rotvecs;
  g.g_trans = a->grad_new_trans;
  g.gR = a->grad_R;
  g.gt = a->grad_t;
  g.gpose = a->grad_pose_rotvecs;
  g.gbetas = in.betas ? a->grad_shape_betas : nullptr;
  g.gtrans = a->grad_trans;
  g.gkid = a->grad_kid_factor;
  hipLaunchKernelGGL(k_rototranslate_backward, dim3((B + kRigidBlock - 1) / kRigidBlock), dim3(kRigidBlock), 0,
                     (hipStream_t)a->hip_stream, in, g, B);
  return post_launch_check();
}

size_t smplfit_mesh_objective_workspace_bytes(const smplfit_handle* h, int batch) {
  return smplfit_forward_backward_workspace_bytes(h, batch);
}

size_t smplfit_fit_objective_workspace_bytes(const smplfit_handle* h, int batch) {
  if (!h || batch <= 0) return 0;
  Arena ar{nullptr};
  objective_layout(h->t, batch, ar);
  return ar.off;
}

int smplfit_mesh_objective_f32(const smplfit_handle* h, const smplfit_mesh_objective_args* a) {
  if (!a) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_mesh_objective_f32: null arguments");
  return objective_impl("smplfit_mesh_objective_f32", h, *a, nullptr, smplfit_mesh_objective_workspace_bytes(h, a->batch),
                        "smplfit_mesh_objective_workspace_bytes");
}

int smplfit_fit_objective_f32(const smplfit_handle* h, const smplfit_fit_objective_args* a) {
  if (!a) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_fit_objective_f32: null arguments");
  const JointTerm jt{a->target_joints, a->joint_weights, a->joint_scale};
  return objective_impl("smplfit_fit_objective_f32", h, *a, &jt, smplfit_fit_objective_workspace_bytes(h, a->batch),
                        "smplfit_fit_objective_workspace_bytes");
}

int smplfit_shape_solve_f32(const smplfit_handle* h, const float* glob_rotmats,
                            const float* target_vertices, const float* target_joints,
                            const float* vertex_weights, const float* joint_weights, int batch,
                            float beta_regularizer, float beta_regularizer2, float kid_regularizer,
                            int add_mean, float* shape_betas, float* trans, float* kid_factor,
                            float* vertices_out, float* joints_out, void* workspace,
                            size_t workspace_bytes, void* hip_stream) {
  smplfit_shape_solve_args a{};
  a.glob_rotmats = glob_rotmats; a.target_vertices = target_vertices; a.target_joints = target_joints;
  a.vertex_weights = vertex_weights; a.joint_weights = joint_weights; a.batch = batch;
  a.beta_regularizer = beta_regularizer; a.beta_regularizer2 = beta_regularizer2;
  a.kid_regularizer = kid_regularizer; a.add_mean = add_mean;
  a.shape_betas = shape_betas; a.trans = trans; a.kid_factor = kid_factor;
  a.vertices_out = vertices_out; a.joints_out = joints_out;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.hip_stream = hip_stream;
  return smplfit_shape_solve_ex_f32(h, &a);
}

int smplfit_shape_solve_ex_f32(const smplfit_handle* h, const smplfit_shape_solve_args* args) {
  return smplfit_shape_solve_segments_f32(h, args, nullptr);
}

int smplfit_shape_solve_segments_f32(const smplfit_handle* h, const smplfit_shape_solve_args* args_in,
                                     const smplfit_share_segments* segments) {
  if (!args_in) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_shape_solve_ex_f32: null arguments");
  smplfit_shape_solve_args with_share = *args_in;
  if (segments) with_share.share_beta = 1;  // segments imply shared shapes within them
  const smplfit_shape_solve_args* args = &with_share;
  const int batch = args->batch;
  int rc = check_segments("smplfit_shape_solve_segments_f32", segments, batch, args->share_allreduce);
  if (rc) return rc;
  rc = check_call("smplfit_shape_solve_f32", h, batch, args->workspace, args->workspace_bytes,
                  smplfit_share_segments_workspace_bytes(h, batch, segments),
                  segments ? "smplfit_share_segments_workspace_bytes" : "smplfit_workspace_bytes");
  if (rc) return rc;
  if (!args->glob_rotmats || !args->target_vertices || !args->shape_betas || !args->trans)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_shape_solve_f32: null pointer");
  if ((rc = check_scale_share("smplfit_shape_solve_ex_f32", args->scale_mode, args->scale_corr, args->share_beta, args->share_allreduce)))
    return rc;
  if (args->scale_mode && (args->vertices_out || args->joints_out))
    return fail(SMPLFIT_ERR_UNSUPPORTED, "smplfit_shape_solve_ex_f32: no mesh outputs with a scale unknown");
  if (args->kid_regularizer_reference && !h->t.n_kid)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_shape_solve_ex_f32: kid_regularizer_reference given to a handle without kid");
  if (args->beta_regularizer_reference && (args->num_reference_betas < 0 || args->num_reference_betas > h->t.num_betas()))
    return fail(SMPLFIT_ERR_BAD_ARG,
                "smplfit_shape_solve_ex_f32: num_reference_betas must lie in [0, the model's betas]; slice first");
  const DevModel& d = h->d;
  const float *vertex_weights = args->vertex_weights, *joint_weights = args->joint_weights;
  hipStream_t st = (hipStream_t)args->hip_stream;
  const Workspace ws = segments ? point_segments(fit_workspace(h, batch, args->workspace), h, *segments, args->workspace)
                                : fit_workspace(h, batch, args->workspace);
  const bool joints = args->target_joints != nullptr;
  const SolveWeights w = solve_weights(joints, vertex_weights, joint_weights);
  FitOptions o{1, args->beta_regularizer, args->beta_regularizer2, args->kid_regularizer, 0, 0};
  o.share_beta = args->share_beta ? 1 : 0;
  o.segments = segments;
  o.share_allreduce = args->share_allreduce;
  o.share_user = args->share_user;
  o.scale_mode = args->scale_mode;
  o.scale_reg = args->scale_regularizer;
  const int use_ref = (args->beta_regularizer_reference || args->kid_regularizer_reference) ? 1 : 0;
  if (use_ref)  // the ridge pulls towards these (pt/bodyfitter.py:1224-1255); missing columns are 0
    hipLaunchKernelGGL(k_fill_shape, dim3((batch + 255) / 256), dim3(256), 0, st, ws, batch, d.S, d.jt.n_kid,
                       args->beta_regularizer_reference,
                       args->beta_regularizer_reference ? std::min(args->num_reference_betas, d.S - d.jt.n_kid - d.jt.n_pad) : 0,
                       args->kid_regularizer_reference);
  // one iteration of fit() at given rotations: targets in, joint stage (prologue only), normal equations, solve
  const bool scaled = o.scale_mode != 0;
  const Route r = route_of(h, batch, {Entry::kShapeSolve, joints, vertex_weights != nullptr, w.v, o.scale_mode, o.share_beta != 0});
  // (batch-major: the weight stream only where the weights enter the solve)
  const TargetsIn t{args->target_vertices, args->target_joints, vertex_weights, w.v ? vertex_weights : nullptr};
  if ((rc = launch_targets_in(h, r, t, ws, batch, st))) return rc;
  JointStageArgs ja{};
  ja.tj = rotation_targets(ws, joints);  // unused without the joint block
  ja.rj = nullptr;
  ja.rj_shared = 1;
  ja.Gprev = args->glob_rotmats;
  ja.jw = joint_weights;
  ja.fit_rotations = 0;
  ja.do_prologue = 1;
  set_joint_block(&ja, d, joints, w);
  if (!joints) hipMemsetAsync(ws.tjreg, 0, (size_t)batch * d.J * 3 * 4, st);
  launch_joint_stage(d, ja, ws, batch, st);
  if ((rc = launch_normal_equations(h, r, joints, w, ja.tj, joint_weights, scaled, ws, batch, st))) return rc;
  rc = enqueue_solve(h, r, ws, batch, o, joints, w, joint_weights, use_ref, scaled, st);
  if (rc) return rc;
  // a scaled solve leaves the shape as the reference returns it (undivided, :1277-1283) in beta_out
  hipLaunchKernelGGL(k_emit_solution, dim3((batch + 255) / 256), dim3(256), 0, st, ws,
                     o.scale_mode ? ws.beta_out : ws.beta, batch, d.S, d.jt.n_kid, d.S - d.jt.n_kid - d.jt.n_pad, args->add_mean,
                     args->shape_betas, args->trans, args->kid_factor);
  if (o.scale_mode)
    hipLaunchKernelGGL(k_copy, dim3(16), dim3(256), 0, st, ws.scale, args->scale_corr, (size_t)batch);
  if (args->joints_out)
    hipLaunchKernelGGL(k_copy, dim3(64), dim3(256), 0, st, ws.rjoints, args->joints_out,
                       (size_t)batch * d.J * 3);
  if (args->vertices_out)  // the mesh at the solution
    if ((rc = launch_lbs_pass(h, r, mesh_alone(nullptr, args->vertices_out), ws, batch, st))) return rc;
  return post_launch_check();
}

size_t smplfit_shape_solve_backward_workspace_bytes(const smplfit_handle* h, int batch) {
  if (!h || batch <= 0) return 0;
  Arena ar{nullptr};
  adjoint_layout(h->t, batch, ar);
  return ar.off;
}

int smplfit_shape_solve_backward_f32(const smplfit_handle* h, const smplfit_shape_solve_backward_args* a) {
  const char* who = "smplfit_shape_solve_backward_f32";
  if (!a) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null arguments");
  const int B = a->batch;
  if (int rc = check_call(who, h, B, a->workspace, a->workspace_bytes, smplfit_shape_solve_backward_workspace_bytes(h, B),
                          "smplfit_shape_solve_backward_workspace_bytes"))
    return rc;
  const DevModel& d = h->d;
  if (d.S > sf::kAdjMaxUnknowns)
    return fail(SMPLFIT_ERR_UNSUPPORTED, std::string(who) + ": more than 17 shape unknowns");
  if (!a->glob_rotmats || !a->target_vertices || !a->shape_betas || !a->trans)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (d.jt.n_kid && !a->kid_factor) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": a kid handle needs kid_factor");
  if (!d.jt.n_kid && (a->kid_factor || a->grad_kid_factor || a->kid_regularizer_reference || a->grad_kid_regularizer_reference))
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": kid fields given to a handle without kid");
  if (a->joint_weights && !a->target_joints)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": joint_weights without target_joints");
  if ((a->grad_target_joints || a->grad_joint_weights) && !a->target_joints)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": a joint gradient without target_joints");
  const int nb = h->t.num_betas();
  const bool bref = a->beta_regularizer_reference || a->grad_beta_regularizer_reference;
  if (bref && (a->num_reference_betas < 0 || a->num_reference_betas > nb))
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": num_reference_betas must lie in [0, the model's betas]; slice first");
  hipStream_t st = (hipStream_t)a->hip_stream;
  Arena ar{(char*)a->workspace};
  const AdjointLayout l = adjoint_layout(h->t, B, ar);
  const Workspace& ws = l.fb.ws;
  const AdjWorkspace& aw = l.aw;
  const bool joints = a->target_joints != nullptr;
  const SolveWeights w = solve_weights(joints, a->vertex_weights, a->joint_weights);
  AdjArgs k{};
  k.glob = a->glob_rotmats;
  k.tv = a->target_vertices;
  k.tj = a->target_joints;
  k.vw = w.v ? a->vertex_weights : nullptr;
  k.jw = w.j ? a->joint_weights : nullptr;
  k.beta_reg = a->beta_regularizer;
  k.beta_reg2 = a->beta_regularizer2;
  k.kid_reg = a->kid_regularizer;
  k.nb = nb;
  k.nref = a->grad_beta_regularizer_reference ? a->num_reference_betas : 0;
  k.betas = a->shape_betas;
  k.trans = a->trans;
  k.kid = a->kid_factor;
  k.g_betas = a->grad_shape_betas;
  k.g_trans = a->grad_trans;
  k.g_kid = a->grad_kid_factor;
  k.o_tv = a->grad_target_vertices;
  k.o_tj = a->grad_target_joints;
  k.o_vw = a->grad_vertex_weights;
  k.o_jw = a->grad_joint_weights;
  k.o_bref = a->grad_beta_regularizer_reference;
  k.o_kref = a->grad_kid_regularizer_reference;
  k.want_glob = a->grad_glob_rotmats ? 1 : 0;
  // (lambda_x, lambda_t) and the gradients of the ridge references
  ensure_max_lds((const void*)k_adj_gram);
  hipLaunchKernelGGL(k_adj_gram, dim3(B), dim3(256), adj_gram_lds_bytes(d), st, d, k, aw, B);
  const bool vertex_pass = k.o_tv || k.o_vw || k.want_glob;
  if (vertex_pass) {
    // recompute the pose blend shapes at the given rotations (the template is added by k_adj_apply)
    ForwardArgs fa{};
    fa.glob = a->glob_rotmats;
    fa.joints = ws.rjoints;
    launch_forward_joint(d, fa, ws, B, st);
    hipLaunchKernelGGL(k_adj_zero_bias, dim3((B + 255) / 256), dim3(256), 0, st, ws.rp, B, d.Kp, sf::rp_pos(d.P, d.Kp));
    if (int rc = launch_gemm(d, ws, B, st)) return rc;
  }
  if (vertex_pass || k.o_tj || k.o_jw)
    hipLaunchKernelGGL(k_adj_apply, dim3(B), dim3(256), adj_apply_lds_bytes(d), st, d, ws, k, aw, B, vertex_pass ? 1 : 0);
  if (k.want_glob) {
    // three vector-Jacobian products of the forward at given rotations: at the solution with the
    // cotangents c1, at the multipliers with c2, and at zero shape with c2 — each recomputes its posed pass
    ForwardInputs in{};
    in.glob = a->glob_rotmats;
    GradOutputs out{};
    Cotangents ct;
    const auto vjp = [&](const float* betas, const float* kid, const float* cv, const float* cj, float* g) {
      in.betas = nb ? betas : nullptr;
      in.kid = kid;
      ct.vertices = cv;
      ct.joints = joints ? cj : nullptr;
      out.glob = g;
      return launch_forward_backward(h, in, in.betas ? nb : 0, ct, out, l.fb, B, st);
    };
    if (int rc = vjp(a->shape_betas, a->kid_factor, aw.c1, aw.c1j, aw.g1)) return rc;
    if (int rc = vjp(aw.lamb, d.jt.n_kid ? aw.lamk : nullptr, aw.c2, aw.c2j, aw.g2)) return rc;
    if (int rc = vjp(nullptr, nullptr, aw.c2, aw.c2j, aw.g3)) return rc;
    const size_t n = (size_t)B * d.J * 9;
    hipLaunchKernelGGL(k_adj_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, aw.g1, aw.g2, aw.g3,
                       a->grad_glob_rotmats, n);
  }
  return post_launch_check();
}

size_t smplfit_fit_backward_workspace_bytes(const smplfit_handle* h, int batch, int num_iter) {
  if (!h || batch <= 0 || num_iter <= 0) return 0;
  Arena ar{nullptr};
  fit_backward_layout(h->t, batch, num_iter, ar);
  return ar.off;
}

int smplfit_fit_backward_f32(const smplfit_handle* h, const smplfit_fit_backward_args* a) {
  const char* who = "smplfit_fit_backward_f32";
  if (!a) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null arguments");
  if (int rc = check_call(who, h, a->batch, a->workspace, a->workspace_bytes,
                          smplfit_fit_backward_workspace_bytes(h, a->batch, a->num_iter), "smplfit_fit_backward_workspace_bytes"))
    return rc;
  if (int rc = check_sweep_call(who, h, a->num_iter, a->target_joints, a->vertex_weights, a->joint_weights,
                                a->grad_target_joints, a->grad_vertex_weights, a->grad_joint_weights))
    return rc;
  if (!a->target_vertices) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (!h->d.jt.n_kid && a->grad_kid_factor)
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": grad_kid_factor given to a handle without kid");
  return run_fit_backward(h, *a);
}

size_t smplfit_fit_known_shape_backward_workspace_bytes(const smplfit_handle* h, int batch, int num_iter) {
  if (!h || batch <= 0 || num_iter <= 0) return 0;
  Arena ar{nullptr};
  known_shape_backward_layout(h->t, batch, num_iter, ar);
  return ar.off;
}

int smplfit_fit_known_shape_backward_f32(const smplfit_handle* h, const smplfit_fit_known_shape_backward_args* a) {
  const char* who = "smplfit_fit_known_shape_backward_f32";
  if (!a) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null arguments");
  if (int rc = check_call(who, h, a->batch, a->workspace, a->workspace_bytes,
                          smplfit_fit_known_shape_backward_workspace_bytes(h, a->batch, a->num_iter),
                          "smplfit_fit_known_shape_backward_workspace_bytes"))
    return rc;
  if (int rc = check_sweep_call(who, h, a->num_iter, a->target_joints, a->vertex_weights, a->joint_weights,
                                a->grad_target_joints, a->grad_vertex_weights, a->grad_joint_weights))
    return rc;
  if (!a->shape_betas || !a->target_vertices) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (a->num_betas_given < 0 || a->num_betas_given > h->t.num_betas())
    return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": more betas than the model holds; slice first");
  if (a->kid_factor && !h->d.jt.n_kid) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": kid_factor given to a handle without kid");
  if (a->grad_kid_factor && !a->kid_factor) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": grad_kid_factor without kid_factor");
  return run_known_shape_backward(h, *a);
}

// ---- topology transfer + fused conversion ---------------------------------------------------------
int smplfit_transfer_create(int32_t num_vertices_in, int32_t num_vertices_out, const int32_t* indptr,
                            const int32_t* indices, const float* values, int flags, smplfit_transfer** out) {
  if (!out || !indptr || num_vertices_in <= 0 || num_vertices_out <= 0)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_transfer_create: null argument / empty matrix");
  *out = nullptr;
  if (flags & ~(SMPLFIT_CREATE_HOST_ONLY | SMPLFIT_TRANSFER_NEGATE_X))
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_transfer_create: unknown flag bits");
  if (indptr[0] != 0) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_transfer_create: indptr[0] must be 0");
  for (int r = 0; r < num_vertices_out; ++r)
    if (indptr[r + 1] < indptr[r]) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_transfer_create: indptr must not decrease");
  const int nnz = indptr[num_vertices_out];
  if (nnz > 0 && (!indices || !values)) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_transfer_create: null indices / values");
  for (int e = 0; e < nnz; ++e)
    if (indices[e] < 0 || indices[e] >= num_vertices_in)
      return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_transfer_create: column index outside the input vertices");
  auto* t = new smplfit_transfer();
  t->v_in = num_vertices_in;
  t->v_out = num_vertices_out;
  t->indptr.assign(indptr, indptr + num_vertices_out + 1);
  t->indices.assign(indices, indices + nnz);
  t->values.assign(values, values + nnz);
  t->negate_x = (flags & SMPLFIT_TRANSFER_NEGATE_X) != 0;
  sf::transpose_csr(t->v_out, t->v_in, t->indptr, t->indices, t->values, t->t_indptr, t->t_indices, t->t_values);
  if (!(flags & SMPLFIT_CREATE_HOST_ONLY) &&
      (t->dev.upload(t->indptr, &t->d_indptr) || t->dev.upload(t->indices, &t->d_indices) ||
       t->dev.upload(t->values, &t->d_values) ||
       t->dev.upload(t->t_indptr, &t->d_t_indptr) || t->dev.upload(t->t_indices, &t->d_t_indices) ||
       t->dev.upload(t->t_values, &t->d_t_values))) {
    smplfit_transfer_destroy(t);
    return fail(SMPLFIT_ERR_HIP, "smplfit_transfer_create: device upload failed");
  }
  *out = t;
  return SMPLFIT_OK;
}

void smplfit_transfer_destroy(smplfit_transfer* t) {
  if (!t) return;
  t->dev.free_all();
  delete t;
}

int smplfit_transfer_f32(const smplfit_transfer* t, const float* in_vertices, int batch, float* out_vertices,
                         void* hip_stream) {
  if (!t || !in_vertices || !out_vertices || batch < 0)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_transfer_f32: null pointer / negative batch");
  if (!t->d_indptr) return fail(SMPLFIT_ERR_HIP, "smplfit_transfer_f32: the matrix was created host-only (no device)");
  if (batch == 0) return SMPLFIT_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  if (t->negate_x)
    launch_transfer_rows<true>(t->d_indptr, t->d_indices, t->d_values, t->v_in, t->v_out, in_vertices, batch, out_vertices, st);
  else
    launch_transfer_rows<false>(t->d_indptr, t->d_indices, t->d_values, t->v_in, t->v_out, in_vertices, batch, out_vertices, st);
  return post_launch_check();
}

// grad_in = M^T grad_out: k_transfer_rows on the transposed CSR, the cotangent on the staged side (12 V_out bytes of LDS)
int smplfit_transfer_backward_f32(const smplfit_transfer* t, const float* grad_out_vertices, int batch,
                                  float* grad_in_vertices, void* hip_stream) {
  if (!t || !grad_out_vertices || !grad_in_vertices || batch < 0)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_transfer_backward_f32: null pointer / negative batch");
  if (batch == 0) return SMPLFIT_OK;  // nothing to enqueue: before the host-only check (unlike the forward; see the header)
  if (!t->d_t_indptr)
    return fail(SMPLFIT_ERR_HIP, "smplfit_transfer_backward_f32: the matrix was created host-only (no device)");
  hipStream_t st = (hipStream_t)hip_stream;
  if (t->negate_x)
    launch_transfer_rows<true>(t->d_t_indptr, t->d_t_indices, t->d_t_values, t->v_out, t->v_in, grad_out_vertices, batch,
                               grad_in_vertices, st);
  else
    launch_transfer_rows<false>(t->d_t_indptr, t->d_t_indices, t->d_t_values, t->v_out, t->v_in, grad_out_vertices, batch,
                                grad_in_vertices, st);
  return post_launch_check();
}

int smplfit_convert_plan_create(const smplfit_handle* in, const smplfit_handle* out, const smplfit_transfer* transfer,
                                smplfit_convert_plan** plan) {
  if (!in || !out || !plan) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_convert_plan_create: null argument");
  *plan = nullptr;
  if (!in->has_device || !out->has_device)
    return fail(SMPLFIT_ERR_HIP, "smplfit_convert_plan_create: both handles need a device");
  if (transfer ? (transfer->v_in != in->t.V || transfer->v_out != out->t.V) : (in->t.V != out->t.V))
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_convert_plan_create: vertex counts of the models and the matrix disagree");
  const CallShape conv{Entry::kConvert, false};  // (whether the route is batch-major does not depend on the batch)
  if (!route_of(in, 1, conv).bm || !route_of(out, 1, conv).bm || !out->t.has_regressor)
    return fail(SMPLFIT_ERR_UNSUPPORTED,
                "smplfit_convert_plan_create: the fused conversion needs the batch-major kernels on both models "
                "(<= 4 skinning weights per vertex, 10 betas, >= 1024 vertices) and the output model's joint "
                "regressor; use forward + smplfit_transfer_f32 + fit");
  auto* p = new smplfit_convert_plan();
  p->in = in;
  p->out = out;
  if (int rc = upload_slot_transfer(p, p->dev, transfer, "smplfit_convert_plan_create")) {
    smplfit_convert_plan_destroy(p);
    return rc;
  }
  *plan = p;
  return SMPLFIT_OK;
}

void smplfit_convert_plan_destroy(smplfit_convert_plan* p) {
  if (!p) return;
  p->dev.free_all();
  delete p;
}

size_t smplfit_convert_workspace_bytes(const smplfit_convert_plan* p, int batch) {
  if (!p || batch <= 0) return 0;
  return chunked_workspace_bytes(p->out->t, batch, &p->in->t);
}

int smplfit_convert_f32(const smplfit_convert_plan* p, const smplfit_convert_args* a) {
  if (!p || !a) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_convert_f32: null argument");
  if (!a->pose_rotvecs) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_convert_f32: pose_rotvecs is required");
  if (a->shape_betas && (a->num_betas_given < 0 || a->num_betas_given > p->in->t.num_betas()))
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_convert_f32: more betas than the input model holds; slice first");
  // the plan was made while the batch-major path applied; a later smplfit_reload_options may have switched it off
  const CallShape conv{Entry::kConvert, false};
  if (!route_of(p->in, 1, conv).bm || !route_of(p->out, a->batch, conv).bm)
    return fail(SMPLFIT_ERR_UNSUPPORTED, "smplfit_convert_f32: the batch-major path is switched off");
  if (int rc = check_call("smplfit_convert_f32", p->out, a->batch, a->workspace, a->workspace_bytes,
                          smplfit_convert_workspace_bytes(p, a->batch), "smplfit_convert_workspace_bytes"))
    return rc;
  smplfit_fit_args f = fused_fit_args(*a);
  f.workspace = a->workspace;
  ConvertJob job{p, a->pose_rotvecs, a->shape_betas, a->trans, a->shape_betas ? a->num_betas_given : 0, nullptr};
  return fit_impl(p->out, &f, &job);
}

// ---- fused flip (BodyFlipper.flip) ------------------------------------------------------------------
// The conversion's pipeline with in = out = the kid handle: the mirror matrix (x negated in k_transfer_bm), the input
// mesh evaluated with kid_factor, and a warm-started fit (k_naive_flip writes its initial pose to the workspace).
int smplfit_flip_plan_create(const smplfit_handle* h, const smplfit_transfer* mirror, const int32_t* joint_perm,
                             smplfit_flip_plan** plan) {
  if (!h || !mirror || !joint_perm || !plan) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_flip_plan_create: null argument");
  *plan = nullptr;
  if (mirror->v_in != h->t.V || mirror->v_out != h->t.V)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_flip_plan_create: the mirror matrix is not (V x V) for this model");
  const int J = h->t.J;
  for (int j = 0; j < J; ++j)
    if (joint_perm[j] < 0 || joint_perm[j] >= J || joint_perm[joint_perm[j]] != j)
      return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_flip_plan_create: joint_perm must map [0, J) onto itself and be an involution");
  if (!h->has_device) return fail(SMPLFIT_ERR_HIP, "smplfit_flip_plan_create: the handle needs a device");
  const CallShape conv{Entry::kConvert, false};  // (whether the route is batch-major does not depend on the batch)
  if (!route_of(h, 1, conv).bm || !h->t.has_regressor)
    return fail(SMPLFIT_ERR_UNSUPPORTED,
                "smplfit_flip_plan_create: the fused flip needs the batch-major kernels (<= 8 skinning weights per "
                "vertex, 10 / 16 betas, >= 1024 vertices) and the model's joint regressor; use forward + "
                "smplfit_transfer_f32 + smplfit_fit_warm_f32");
  auto* p = new smplfit_flip_plan();
  p->conv.in = h;
  p->conv.out = h;
  int rc = upload_slot_transfer(&p->conv, p->dev, mirror, "smplfit_flip_plan_create");
  if (!rc && p->dev.upload(joint_perm, (size_t)J, &p->d_perm)) rc = fail(SMPLFIT_ERR_HIP, "smplfit_flip_plan_create: device upload failed");
  if (rc) {
    smplfit_flip_plan_destroy(p);
    return rc;
  }
  *plan = p;
  return SMPLFIT_OK;
}

void smplfit_flip_plan_destroy(smplfit_flip_plan* p) {
  if (!p) return;
  p->dev.free_all();
  delete p;
}

size_t smplfit_flip_workspace_bytes(const smplfit_flip_plan* p, int batch) {
  if (!p || batch <= 0) return 0;
  Arena ar{nullptr};
  flip_layout(p->conv, batch, ar);
  return ar.off;
}

int smplfit_flip_f32(const smplfit_flip_plan* p, const smplfit_flip_args* a) {
  if (!p || !a) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_flip_f32: null argument");
  const smplfit_handle* h = p->conv.out;
  const int B = a->batch;
  if (int rc = check_call("smplfit_flip_f32", h, B, a->workspace, a->workspace_bytes, smplfit_flip_workspace_bytes(p, B),
                          "smplfit_flip_workspace_bytes"))
    return rc;
  if (!a->pose_rotvecs) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_flip_f32: pose_rotvecs is required");
  if (a->shape_betas && (a->num_betas_given < 0 || a->num_betas_given > h->t.num_betas()))
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_flip_f32: more betas than the model holds; slice first");
  if (!a->out_pose_rotvecs || !a->out_shape_betas || !a->out_trans)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_flip_f32: null output pointer");
  if (a->num_iter < 1) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_flip_f32: num_iter must be >= 1");
  // the plan was made while the batch-major path applied; a later smplfit_reload_options may have switched it off
  const CallShape conv{Entry::kConvert, false};
  if (!route_of(h, B, conv).bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "smplfit_flip_f32: the batch-major path is switched off");
  hipStream_t st = (hipStream_t)a->hip_stream;
  Arena ar{(char*)a->workspace};
  const FlipLayout l = flip_layout(p->conv, B, ar);
  hipLaunchKernelGGL(k_naive_flip, dim3((B + 255) / 256), dim3(256), 0, st, a->pose_rotvecs, p->d_perm, l.init_pose, B, h->t.J);
  smplfit_fit_args f = fused_fit_args(*a);
  f.initial_pose_rotvecs = l.init_pose;
  f.initial_shape_betas = a->shape_betas;
  f.num_initial_betas = a->shape_betas ? a->num_betas_given : 0;
  f.workspace = l.fit;
  ConvertJob job{&p->conv, a->pose_rotvecs, a->shape_betas, a->trans, a->shape_betas ? a->num_betas_given : 0,
                 a->kid_factor};
  return fit_impl(h, &f, &job);
}

// ---- fused hand replacement (HandReplacer.replace_hand) ----------------------------------------------
// The weighted fit on whatever route the model and the call take (the (V) weights read through the shared-row ingest),
// k_replace_rotations on the fit's relative rotations, the forward steps from those matrices on the batch-major
// kernels, and the blend in the pass that writes the caller's (B, V, 3).
int smplfit_replace_hands_plan_create(const smplfit_handle* h, const float* fit_weights, const float* mix_weights,
                                      int32_t num_vertices, int32_t first_joint, int32_t num_joints, const float* rotvecs,
                                      int32_t num_rotvec_values, smplfit_replace_hands_plan** plan) {
  if (!h || !fit_weights || !mix_weights || !rotvecs || !plan)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_replace_hands_plan_create: null argument");
  *plan = nullptr;
  if (num_vertices != h->t.V)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_replace_hands_plan_create: the weight vectors must hold one value per vertex of the model");
  if (first_joint < 0 || num_joints < 1 || first_joint > h->t.J - num_joints)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_replace_hands_plan_create: the joint range must lie in [0, J) and hold a joint");
  if (num_rotvec_values != 3 * num_joints)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_replace_hands_plan_create: three rotation-vector values per joint of the range");
  if (!h->has_device) return fail(SMPLFIT_ERR_HIP, "smplfit_replace_hands_plan_create: the handle needs a device");
  if (h->t.n_kid || !h->t.has_regressor || !route_of(h, 1, {Entry::kForward}).bm)
    return fail(SMPLFIT_ERR_UNSUPPORTED,
                "smplfit_replace_hands_plan_create: the fused call needs a handle without the kid unknown, the model's joint "
                "regressor and the batch-major kernels for the forward (<= 8 skinning weights per vertex, 10 / 16 betas, "
                ">= 1024 vertices); use smplfit_fit_f32 + smplfit_forward_f32 and blend");
  auto* p = new smplfit_replace_hands_plan();
  p->h = h;
  p->j0 = first_joint;
  p->n = num_joints;
  DeviceArrays& dev = p->dev;
  bool ok = !dev.upload(fit_weights, (size_t)num_vertices, &p->d_fitw) && !dev.upload(mix_weights, (size_t)num_vertices, &p->d_mix) &&
            !dev.upload(rotvecs, (size_t)3 * num_joints, &p->d_rv) && !dev.alloc((size_t)9 * num_joints * sizeof(float), &p->d_mats);
  if (ok) {
    hipLaunchKernelGGL(k_rotvecs_to_mats, dim3((num_joints + 63) / 64), dim3(64), 0, (hipStream_t) nullptr, p->d_rv, p->d_mats, num_joints);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
  }
  if (!ok) {
    smplfit_replace_hands_plan_destroy(p);
    return fail(SMPLFIT_ERR_HIP, "smplfit_replace_hands_plan_create: device upload failed");
  }
  *plan = p;
  return SMPLFIT_OK;
}

void smplfit_replace_hands_plan_destroy(smplfit_replace_hands_plan* p) {
  if (!p) return;
  p->dev.free_all();
  delete p;
}

size_t smplfit_replace_hands_workspace_bytes(const smplfit_replace_hands_plan* p, int batch) {
  if (!p || batch <= 0) return 0;
  Arena ar{nullptr};
  replace_layout(p->h->t, batch, ar);
  return ar.off;
}

int smplfit_replace_hands_f32(const smplfit_replace_hands_plan* p, const smplfit_replace_hands_args* a) {
  if (!p || !a) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_replace_hands_f32: null argument");
  const smplfit_handle* h = p->h;
  const DevModel& d = h->d;
  const int B = a->batch;
  if (int rc = check_call("smplfit_replace_hands_f32", h, B, a->workspace, a->workspace_bytes,
                          smplfit_replace_hands_workspace_bytes(p, B), "smplfit_replace_hands_workspace_bytes"))
    return rc;
  if (!a->vertices || !a->out_vertices) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_replace_hands_f32: vertices and out_vertices are required");
  if (a->num_iter < 1) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_replace_hands_f32: num_iter must be >= 1");
  // the plan was made while the batch-major forward applied; a later smplfit_reload_options may have switched it off
  const Route rf = route_of(h, B, {Entry::kForward});
  if (!rf.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "smplfit_replace_hands_f32: the batch-major path is switched off");
  hipStream_t st = (hipStream_t)a->hip_stream;
  Arena ar{(char*)a->workspace};
  const ReplaceLayout fr = replace_layout(h->t, B, ar);
  float* pose = a->out_pose_rotvecs ? a->out_pose_rotvecs : fr.pose;
  float* betas = a->out_shape_betas ? a->out_shape_betas : fr.betas;
  float* trans = a->out_trans ? a->out_trans : fr.trans;
  smplfit_fit_args f{};
  f.target_vertices = a->vertices;
  f.vertex_weights = p->d_fitw;
  f.batch = B;
  f.num_iter = a->num_iter;
  f.beta_regularizer = a->beta_regularizer;
  f.beta_regularizer2 = a->beta_regularizer2;
  f.final_adjust_rots = a->final_adjust_rots;
  f.pose_rotvecs = pose;
  f.shape_betas = betas;
  f.trans = trans;
  f.relative_orientations = fr.rel;
  f.workspace = fr.fit;
  f.hip_stream = a->hip_stream;
  if (int rc = fit_impl(h, &f, nullptr, true)) return rc;
  {
    const size_t total = (size_t)B * 9 * p->n;
    hipLaunchKernelGGL(k_replace_rotations, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p->d_mats, p->d_rv, fr.rel,
                       a->out_pose_rotvecs, B, d.J, p->j0, p->n);
  }
  // the forward at the edited relative rotations (the fit's chunks have been joined: one pass over the whole batch)
  const Workspace ws = fit_workspace(h, B, fr.fit);
  ForwardInputs in{};
  in.rel = fr.rel;
  in.betas = betas;
  const ForwardArgs fa = forward_args(in, d.S - d.jt.n_kid - d.jt.n_pad, trans, ws.rjoints, nullptr);
  launch_forward_joint(d, fa, ws, B, st);
  if (int rc = launch_posed_pass(h, rf, {nullptr, mesh_blended(&fa, a->out_vertices, a->vertices, p->d_mix)}, ws, B, st)) return rc;
  return post_launch_check();
}

// ---- mesh error: the model at given parameters against the caller's targets ----------
size_t smplfit_mesh_error_workspace_bytes(const smplfit_handle* h, int batch) { return smplfit_workspace_bytes(h, batch); }

int smplfit_mesh_error_f32(const smplfit_handle* h, const smplfit_mesh_error_args* a) {
  const char* who = "smplfit_mesh_error_f32";
  if (!a) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null arguments");
  const int B = a->batch;
  if (int rc = check_call(who, h, B, a->workspace, a->workspace_bytes, smplfit_mesh_error_workspace_bytes(h, B),
                          "smplfit_mesh_error_workspace_bytes"))
    return rc;
  const DevModel& d = h->d;
  const ForwardInputs in = forward_inputs(*a);
  if (int rc = check_forward_inputs(who, d, in)) return rc;
  if (int rc = check_recon_outputs(who, a->vertices, a->joints, a->vertex_error, a->joint_error, a->target_vertices, a->target_joints))
    return rc;
  hipStream_t st = (hipStream_t)a->hip_stream;
  const Workspace ws = fit_workspace(h, B, a->workspace);
  MeshError me;
  me.fa = forward_args(in, forward_nb(d, in), a->trans, a->joints ? a->joints : ws.rjoints, nullptr);
  me.tv = a->target_vertices;
  me.tj = a->target_joints;
  me.vertices = a->vertices;
  me.verr = a->vertex_error;
  me.jerr = a->joint_error;
  if (int rc = launch_mesh_error(h, route_of(h, B, {Entry::kForward}), me, ws, B, st)) return rc;
  return post_launch_check();
}

size_t smplfit_fit_recon_workspace_bytes(const smplfit_handle* h, int batch, const smplfit_share_segments* segments) {
  if (!h || batch <= 0 || (segments && batch != segments->t.batch)) return 0;
  Arena ar{nullptr};
  recon_layout(h, batch, segments, ar);
  return ar.off;
}

int smplfit_fit_recon_f32(const smplfit_handle* h, const smplfit_fit_args* args, const smplfit_share_segments* segments,
                          const smplfit_fit_recon_args* recon) {
  const char* who = "smplfit_fit_recon_f32";
  if (!recon) return smplfit_fit_segments_f32(h, args, segments);
  if (!args) return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": null arguments");
  const int B = args->batch;
  if (int rc = check_segments(who, segments, B, args->share_allreduce)) return rc;
  if (int rc = check_call(who, h, B, args->workspace, args->workspace_bytes, smplfit_fit_recon_workspace_bytes(h, B, segments),
                          "smplfit_fit_recon_workspace_bytes"))
    return rc;
  if (int rc = check_recon_outputs(who, recon->vertices, recon->joints, recon->vertex_error, recon->joint_error,
                                   args->target_vertices, args->target_joints))
    return rc;
  // (which target the errors of a scaled fit refer to is undecided: refused before anything is enqueued)
  if (args->scale_mode) return fail(SMPLFIT_ERR_UNSUPPORTED, std::string(who) + ": the scale options are not served with reconstruction");
  Arena ar{(char*)args->workspace};
  const ReconLayout l = recon_layout(h, B, segments, ar);
  smplfit_fit_args f = *args;
  if (!f.orientations) f.orientations = l.orient;
  if (h->t.n_kid && !f.kid_factor) f.kid_factor = l.kid;
  f.workspace = l.fit;
  f.workspace_bytes = l.fit_bytes;
  if (segments) f.share_beta = 1;  // segments imply shared shapes within them
  if (int rc = fit_impl(h, &f, nullptr, false, segments)) return rc;
  // the step at the fit's results (its chunks have been joined: one pass over the whole batch, as one fit workspace)
  const DevModel& d = h->d;
  hipStream_t st = (hipStream_t)args->hip_stream;
  const Workspace ws = fit_workspace(h, B, l.fit);
  ForwardInputs in{};
  in.glob = f.orientations;
  in.betas = f.shape_betas;
  in.given = h->t.num_betas();
  in.kid = h->t.n_kid ? f.kid_factor : nullptr;
  MeshError me;
  me.fa = forward_args(in, forward_nb(d, in), f.trans, recon->joints ? recon->joints : ws.rjoints, nullptr);
  me.tv = args->target_vertices;
  me.tj = args->target_joints;
  me.vertices = recon->vertices;
  me.verr = recon->vertex_error;
  me.jerr = recon->joint_error;
  if (int rc = launch_mesh_error(h, route_of(h, B, {Entry::kForward}), me, ws, B, st)) return rc;
  return post_launch_check();
}

// ---- aligned errors: Procrustes alignment of the model onto the targets, then the distances ----
// A row-major point set of a call: x the model, y the target, w the weights or null
struct AlignSet {
  const float *x, *y, *w;
  int n;
};
int align_nslab(int n) { return (n + kAlignSlab - 1) / kAlignSlab; }
// What the launches of a (B, n, 3) set can address: the slabs of a row are grid.y of k_align_moments (at most 65535: n
// up to 2^26 gives 32768), the points of the batch in blocks of 256 are grid.x of k_align_apply (below 2^31)
constexpr int kAlignMaxPoints = 1 << 26;
bool align_counts_ok(int B, int n) { return B > 0 && n > 0 && n <= kAlignMaxPoints && (size_t)B * (size_t)n <= ((size_t)1 << 38); }

// STEP transform of a set: its moments and the solve (kAlignRoot: `set` is the joints; the moments give the row's
// validity).  rec (B, kAlignRecord) is what launch_align_measure reads; scale / rot / trans: the caller's, each may be null.
void launch_align_transform(const AlignSet& set, int mode, double* part, float* rec, float* scale, float* rot, float* trans, int B,
                            hipStream_t st) {
  const int nslab = align_nslab(set.n);
  hipLaunchKernelGGL(k_align_moments, dim3(B, nslab), dim3(256), 0, st, set.x, set.y, set.w, set.n, B, part);
  AlignSolveArgs sa{};
  sa.part = part;
  sa.x = set.x;
  sa.y = set.y;
  sa.n = set.n;
  sa.nslab = nslab;
  sa.B = B;
  sa.mode = mode;
  sa.rec = rec;
  sa.scale = scale;
  sa.rot = rot;
  sa.trans = trans;
  hipLaunchKernelGGL(k_align_solve, dim3((B + 63) / 64), dim3(64), 0, st, sa);
}
// STEP row means of (B, n) errors
void launch_align_means(const float* err, const float* w, int n, float* mean, int B, hipStream_t st) {
  hipLaunchKernelGGL(k_align_row_means, dim3((B + 3) / 4), dim3(256), 0, st, err, w, n, B, mean);
}
// STEP measure a set under the transform of `rec`: the errors (B, n), and their row means where asked for
void launch_align_measure(const AlignSet& set, const float* rec, float* err, float* mean, int B, hipStream_t st) {
  const size_t total = (size_t)B * set.n;
  hipLaunchKernelGGL(k_align_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, set.x, set.y, rec, err, set.n, total);
  if (mean) launch_align_means(err, set.w, set.n, mean, B, st);
}

// LAYOUT alignment of two (B, n, 3) arrays: the slab moments, the rows' records, and the errors where only their means
// are asked for
struct AlignPointsLayout {
  double* part;
  float *rec, *err;
};
AlignPointsLayout align_points_layout(int B, int n, Arena& ar) {
  AlignPointsLayout l;
  l.part = ar.take<double>((size_t)align_nslab(n) * B * sf::kAlignMoments);
  l.rec = ar.take<float>((size_t)B * sf::kAlignRecord);
  l.err = ar.take<float>((size_t)B * n);
  return l;
}
size_t smplfit_align_points_workspace_bytes(int batch, int num_points) {
  if (!align_counts_ok(batch, num_points)) return 0;
  Arena ar{nullptr};
  align_points_layout(batch, num_points, ar);
  return ar.off;
}

int smplfit_align_points_f32(const smplfit_align_points_args* a) {
  const char* who = "smplfit_align_points_f32";
  const auto bad = [who](const char* what) { return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (!a) return bad("null arguments");
  if (a->batch <= 0) return bad("batch must be positive");
  if (a->num_points < 1 || a->num_points > kAlignMaxPoints) return bad("num_points must lie in [1, 2^26]");
  if (!align_counts_ok(a->batch, a->num_points)) return bad("batch * num_points must not exceed 2^38");
  if (!a->source || !a->target) return bad("source and target are required");
  if (a->align != SMPLFIT_ALIGN_TRANSLATION && a->align != SMPLFIT_ALIGN_RIGID && a->align != SMPLFIT_ALIGN_SIMILARITY)
    return bad("align must be translation (2), rigid (3) or similarity (4)");
  if (!a->error && !a->mean_error && !a->scale && !a->rotation && !a->translation) return bad("at least one output is required");
  if (!a->workspace || ((uintptr_t)a->workspace & 255))
    return fail(SMPLFIT_ERR_WORKSPACE, std::string(who) + ": workspace must be a 256-byte aligned device pointer");
  if (a->workspace_bytes < smplfit_align_points_workspace_bytes(a->batch, a->num_points))
    return fail(SMPLFIT_ERR_WORKSPACE, std::string(who) + ": workspace too small (see smplfit_align_points_workspace_bytes)");
  hipStream_t st = (hipStream_t)a->hip_stream;
  Arena ar{(char*)a->workspace};
  const AlignPointsLayout l = align_points_layout(a->batch, a->num_points, ar);
  const AlignSet set{a->source, a->target, a->weights, a->num_points};
  launch_align_transform(set, a->align, l.part, l.rec, a->scale, a->rotation, a->translation, a->batch, st);
  if (a->error || a->mean_error) launch_align_measure(set, l.rec, a->error ? a->error : l.err, a->mean_error, a->batch, st);
  return post_launch_check();
}

// LAYOUT aligned mesh error: the mesh-error step's workspace, the slab moments and the records of the two sets, then
// the mesh (B,V,3) and the errors (B,V) + (B,J), each only where the caller gave no buffer for it (own_*).  The query
// has no call to look at and counts all three.
struct MeshAlignLayout {
  char* fit;
  float *mesh, *verr, *jerr, *recv, *recj;
  double *partv, *partj;
};
MeshAlignLayout mesh_align_layout(const smplfit_handle* h, int B, bool own_mesh, bool own_verr, bool own_jerr, Arena& ar) {
  MeshAlignLayout l{};
  const size_t V = h->t.V, J = h->t.J;
  l.fit = ar.take<char>(smplfit_workspace_bytes(h, B));
  l.partv = ar.take<double>((size_t)align_nslab((int)V) * B * sf::kAlignMoments);
  l.partj = ar.take<double>((size_t)align_nslab((int)J) * B * sf::kAlignMoments);
  l.recv = ar.take<float>((size_t)B * sf::kAlignRecord);
  l.recj = ar.take<float>((size_t)B * sf::kAlignRecord);
  if (own_mesh) l.mesh = ar.take<float>((size_t)B * V * 3);
  if (own_verr) l.verr = ar.take<float>((size_t)B * V);
  if (own_jerr) l.jerr = ar.take<float>((size_t)B * J);
  return l;
}
size_t mesh_align_bytes(const smplfit_handle* h, int batch, bool own_mesh, bool own_verr, bool own_jerr) {
  if (!h || batch <= 0) return 0;
  Arena ar{nullptr};
  mesh_align_layout(h, batch, own_mesh, own_verr, own_jerr, ar);
  return ar.off;
}
size_t smplfit_mesh_error_aligned_workspace_bytes(const smplfit_handle* h, int batch) {
  return mesh_align_bytes(h, batch, true, true, true);
}

int smplfit_mesh_error_aligned_f32(const smplfit_handle* h, const smplfit_mesh_error_args* a, const smplfit_mesh_align_args* al) {
  const char* who = "smplfit_mesh_error_aligned_f32";
  if (!al) return smplfit_mesh_error_f32(h, a);
  const auto bad = [who](const char* what) { return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (!a) return bad("null arguments");
  const int B = a->batch;
  // (what the align struct asks for is checked first: these refusals need no device)
  const int mode = al->align, on = al->align_on;
  const float *tv = a->target_vertices, *tj = a->target_joints;
  if (mode < 0 || mode >= sf::kAlignModeCount) return bad("unknown align (0 none, 1 root, 2 translation, 3 rigid, 4 similarity)");
  if (on < 0 || on >= sf::kAlignOnCount) return bad("unknown align_on (0 each, 1 vertices, 2 joints)");
  if (!tv) return bad("target_vertices is required");
  if (mode == sf::kAlignRoot && !tj) return bad("align = root needs target_joints");
  if (mode != sf::kAlignNone && on == sf::kAlignOnJoints && !tj) return bad("align_on = joints needs target_joints");
  const bool xform_out = al->scale || al->rotation || al->translation;
  const bool jxform_out = al->joint_scale || al->joint_rotation || al->joint_translation;
  if (!tj && (a->joint_error || al->mean_joint_error || jxform_out || al->joint_weights))
    return bad("joint_error, mean_joint_error, the joints' transform and joint_weights need target_joints");
  if (!a->vertices && !a->joints && !a->vertex_error && !a->joint_error && !al->mean_vertex_error && !al->mean_joint_error &&
      !xform_out && !jxform_out)
    return bad("at least one output is required");
  if (mode == sf::kAlignNone && (xform_out || jxform_out)) return bad("align = none has no transform to return");
  const bool each = mode >= sf::kAlignTranslation && on == sf::kAlignEach;
  if (jxform_out && !each) return bad("the joints' own transform exists with align_on = each alone (not with align = root)");
  // (a region the caller's own buffer stands in for is not asked of the workspace)
  const bool own_mesh = !a->vertices, own_verr = !a->vertex_error, own_jerr = !a->joint_error;
  if (int rc = check_call(who, h, B, a->workspace, a->workspace_bytes, mesh_align_bytes(h, B, own_mesh, own_verr, own_jerr),
                          "smplfit_mesh_error_aligned_workspace_bytes"))
    return rc;
  const DevModel& d = h->d;
  const ForwardInputs in = forward_inputs(*a);
  if (int rc = check_forward_inputs(who, d, in)) return rc;
  hipStream_t st = (hipStream_t)a->hip_stream;
  Arena ar{(char*)a->workspace};
  const MeshAlignLayout l = mesh_align_layout(h, B, own_mesh, own_verr, own_jerr, ar);
  const Workspace ws = fit_workspace(h, B, l.fit);
  const Route r = route_of(h, B, {Entry::kForward});
  MeshError me;
  me.fa = forward_args(in, forward_nb(d, in), a->trans, a->joints ? a->joints : ws.rjoints, nullptr);
  me.tv = tv;
  me.tj = tj;
  me.vertices = a->vertices;
  const bool want_v = a->vertex_error || al->mean_vertex_error, want_j = a->joint_error || al->mean_joint_error;
  float* verr = !want_v ? nullptr : a->vertex_error ? a->vertex_error : l.verr;
  float* jerr = !want_j ? nullptr : a->joint_error ? a->joint_error : l.jerr;
  if (mode == sf::kAlignNone) {  // the mesh-error step as it is, then the row means
    me.verr = verr;
    me.jerr = jerr;
    if (int rc = launch_mesh_error(h, r, me, ws, B, st)) return rc;
    if (al->mean_vertex_error) launch_align_means(verr, al->vertex_weights, d.V, al->mean_vertex_error, B, st);
    if (al->mean_joint_error) launch_align_means(jerr, al->joint_weights, d.J, al->mean_joint_error, B, st);
    return post_launch_check();
  }
  // which set gives the transform the vertices are measured under, and the joints
  const bool from_joints = mode == sf::kAlignRoot || on == sf::kAlignOnJoints;
  const bool solve_v = !from_joints && (want_v || xform_out || (on == sf::kAlignOnVertices && want_j));
  const bool solve_j = from_joints ? (want_v || want_j || xform_out) : (each && (want_j || jxform_out));
  launch_forward_joint(d, me.fa, ws, B, st);
  const bool need_mesh = a->vertices || want_v || solve_v;
  float* mesh = a->vertices ? a->vertices : l.mesh;
  if (need_mesh)
    if (int rc = launch_posed_pass(h, r, {nullptr, mesh_alone(&me.fa, mesh)}, ws, B, st)) return rc;
  const AlignSet sv{mesh, tv, al->vertex_weights, d.V}, sj{me.fa.joints, tj, al->joint_weights, d.J};
  if (solve_v) launch_align_transform(sv, mode, l.partv, l.recv, al->scale, al->rotation, al->translation, B, st);
  if (solve_j) {
    if (from_joints) launch_align_transform(sj, mode, l.partj, l.recj, al->scale, al->rotation, al->translation, B, st);
    else launch_align_transform(sj, mode, l.partj, l.recj, al->joint_scale, al->joint_rotation, al->joint_translation, B, st);
  }
  // (a record holds the origins of the set it was solved on; the other set is measured about the same two points)
  if (want_v) launch_align_measure(sv, from_joints ? l.recj : l.recv, verr, al->mean_vertex_error, B, st);
  if (want_j) launch_align_measure(sj, (from_joints || each) ? l.recj : l.recv, jerr, al->mean_joint_error, B, st);
  return post_launch_check();
}

// ---- robust reweighting and the reweighted fit ----------------------------------------
// What both entries check of the loss and the scale source before anything is enqueued
int check_robust_options(const char* who, int loss, float tuning, float scale, const float* scale_rows, float scale_floor) {
  const auto bad = [who](const char* what) { return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (loss < 0 || loss >= sf::kRobustLossCount) return bad("unknown loss (0 huber, 1 cauchy, 2 geman_mcclure, 3 tukey)");
  if (!(tuning > 0.f) || !std::isfinite(tuning)) return bad("tuning must be positive and finite");
  if (!(scale >= 0.f) || !std::isfinite(scale)) return bad("scale must be positive and finite, or 0 for none");
  if (scale > 0.f && scale_rows) return bad("scale and scale_rows cannot both be given");
  if (!(scale > 0.f) && !scale_rows && (!(scale_floor > 0.f) || !std::isfinite(scale_floor)))
    return bad("scale_floor must be positive and finite where the scale comes from the median");
  return 0;
}

// STEP reweight: sigma and the weights of every row from its errors, one launch
void launch_robust_reweight(const RobustArgs& a, int B, hipStream_t st) {
  const bool median = !(a.scale > 0.f) && !a.scale_rows;
  const size_t lds = (median && (size_t)a.nv * 4 <= kRobustStageBytes) ? (size_t)a.nv * 4 : 0;
  hipLaunchKernelGGL(k_robust_reweight, dim3(B), dim3(kRobustThreads), lds, st, a, lds ? 1 : 0);
}
void launch_robust_prior(const float* src, float value, float* dst, size_t n, hipStream_t st) {
  if (dst && n) hipLaunchKernelGGL(k_robust_prior, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, value, dst, n);
}

int smplfit_robust_weights_f32(const smplfit_robust_weights_args* a) {
  const char* who = "smplfit_robust_weights_f32";
  const auto bad = [who](const char* what) { return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (!a) return bad("null arguments");
  if (a->batch <= 0) return bad("batch must be positive");
  if (a->num_vertex_errors < 1 || a->num_vertex_errors > (1 << 30)) return bad("num_vertex_errors must lie in [1, 2^30]");
  if (a->num_joint_errors < 0 || a->num_joint_errors > (1 << 30)) return bad("num_joint_errors must lie in [0, 2^30]");
  if (!a->vertex_error || !a->out_vertex_weights) return bad("vertex_error and out_vertex_weights are required");
  const bool joints = a->num_joint_errors > 0 && a->joint_error;
  if (a->joint_error && !a->num_joint_errors) return bad("joint_error given with num_joint_errors = 0");
  if (joints && !a->out_joint_weights) return bad("joint_error needs out_joint_weights");
  if (!joints && (a->joint_weights || a->out_joint_weights)) return bad("joint weights need joint_error");
  if (int rc = check_robust_options(who, a->loss, a->tuning, a->scale, a->scale_rows, a->scale_floor)) return rc;
  RobustArgs r{};
  r.ev = a->vertex_error;
  r.ej = joints ? a->joint_error : nullptr;
  r.w0v = a->vertex_weights;
  r.w0j = a->joint_weights;
  r.wv = a->out_vertex_weights;
  r.wj = a->out_joint_weights;
  r.sigma = a->out_scale;
  r.scale_rows = a->scale_rows;
  r.nv = a->num_vertex_errors;
  r.nj = joints ? a->num_joint_errors : 0;
  r.loss = a->loss;
  r.tuning = a->tuning;
  r.scale = a->scale;
  r.floor = a->scale_floor;
  launch_robust_reweight(r, a->batch, (hipStream_t)a->hip_stream);
  return post_launch_check();
}

size_t smplfit_fit_robust_workspace_bytes(const smplfit_handle* h, int batch, const smplfit_share_segments* segments) {
  if (!h || batch <= 0 || (segments && batch != segments->t.batch)) return 0;
  Arena ar{nullptr};
  robust_layout(h, batch, segments, true, true, true, ar);
  return ar.off;
}

int smplfit_fit_robust_f32(const smplfit_handle* h, const smplfit_fit_args* args, const smplfit_share_segments* segments,
                           const smplfit_fit_recon_args* recon, const smplfit_fit_robust_args* robust) {
  const char* who = "smplfit_fit_robust_f32";
  const auto bad = [who](const char* what) { return fail(SMPLFIT_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (!args || !robust) return bad("null arguments");
  const int B = args->batch;
  if (int rc = check_segments(who, segments, B, args->share_allreduce)) return rc;
  if (int rc = check_call(who, h, B, args->workspace, args->workspace_bytes, smplfit_fit_robust_workspace_bytes(h, B, segments),
                          "smplfit_fit_robust_workspace_bytes"))
    return rc;
  if (!args->target_vertices) return bad("target_vertices is required");
  if (recon)
    if (int rc = check_recon_outputs(who, recon->vertices, recon->joints, recon->vertex_error, recon->joint_error,
                                     args->target_vertices, args->target_joints))
      return rc;
  // (the errors of a scaled fit refer to an undecided target, as with reconstruction: refused before anything is enqueued)
  if (args->scale_mode) return fail(SMPLFIT_ERR_UNSUPPORTED, std::string(who) + ": the scale options are not served with robust rounds");
  if (args->share_allreduce) return bad("share_allreduce cannot be combined with robust rounds");
  if (args->initial_pose_rotvecs || args->initial_shape_betas || args->initial_kid_factor)
    return bad("warm starts are not served: every round after the first starts from the previous round's pose");
  if (int rc = check_robust_options(who, robust->loss, robust->tuning, robust->scale, robust->scale_rows, robust->scale_floor))
    return rc;
  if (robust->num_rounds < 0) return bad("num_rounds must be >= 0");
  if (robust->round_num_iter < 0) return bad("round_num_iter must be >= 1, or 0 for num_iter");
  const bool joints = args->target_joints != nullptr;
  if (!joints && robust->joint_weights) return bad("the joint_weights output needs target_joints");
  const sf::HostTables& t = h->t;
  hipStream_t st = (hipStream_t)args->hip_stream;
  Arena ar{(char*)args->workspace};
  const RobustLayout l = robust_layout(h, B, segments, !robust->vertex_weights, !robust->joint_weights, !robust->scale_out, ar);
  float* wv = robust->vertex_weights ? robust->vertex_weights : l.wv;
  float* wj = !joints ? nullptr : robust->joint_weights ? robust->joint_weights : l.wj;
  float* sigma = robust->scale_out ? robust->scale_out : l.sigma;

  // round 0: the fit as smplfit_fit_recon_f32 runs it
  smplfit_fit_args f = *args;
  if (!f.orientations) f.orientations = l.rc.orient;
  if (t.n_kid && !f.kid_factor) f.kid_factor = l.rc.kid;
  f.workspace = l.rc.fit;
  f.workspace_bytes = l.rc.fit_bytes;
  if (segments) f.share_beta = 1;  // segments imply shared shapes within them
  if (int rc = fit_impl(h, &f, nullptr, false, segments)) return rc;

  // the mesh-error step at the current results (the fit's chunks have been joined: one pass, as one fit workspace)
  const DevModel& d = h->d;
  const auto mesh_error = [&](float* vertices, float* joints_out, float* verr, float* jerr) {
    const Workspace ws = fit_workspace(h, B, l.rc.fit);
    ForwardInputs in{};
    in.glob = f.orientations;
    in.betas = f.shape_betas;
    in.given = t.num_betas();
    in.kid = t.n_kid ? f.kid_factor : nullptr;
    MeshError me;
    me.fa = forward_args(in, forward_nb(d, in), f.trans, joints_out ? joints_out : ws.rjoints, nullptr);
    me.tv = args->target_vertices;
    me.tj = args->target_joints;
    me.vertices = vertices;
    me.verr = verr;
    me.jerr = jerr;
    return launch_mesh_error(h, route_of(h, B, {Entry::kForward}), me, ws, B, st);
  };

  // every later round: errors at the previous results, weights from them, the fit again from the previous pose
  smplfit_fit_args g = f;
  g.vertex_weights = wv;
  g.joint_weights = wj;
  g.initial_pose_rotvecs = l.pose;
  if (robust->round_num_iter) g.num_iter = robust->round_num_iter;
  RobustArgs r{};
  r.ev = l.verr;
  r.ej = joints ? l.jerr : nullptr;
  r.w0v = args->vertex_weights;
  r.w0j = joints ? args->joint_weights : nullptr;
  r.wv = wv;
  r.wj = wj;
  r.sigma = sigma;
  r.scale_rows = robust->scale_rows;
  r.nv = t.V;
  r.nj = joints ? t.J : 0;
  r.loss = robust->loss;
  r.tuning = robust->tuning;
  r.scale = robust->scale;
  r.floor = robust->scale_floor;
  for (int round = 1; round <= robust->num_rounds; ++round) {
    if (int rc = mesh_error(nullptr, nullptr, l.verr, joints ? l.jerr : nullptr)) return rc;
    launch_robust_reweight(r, B, st);
    SF_HIP_TRY(hipMemcpyAsync(l.pose, f.pose_rotvecs, (size_t)B * t.J * 3 * 4, hipMemcpyDeviceToDevice, st));
    if (int rc = fit_impl(h, &g, nullptr, false, segments)) return rc;
  }
  if (robust->num_rounds == 0) {  // no round: the prior weights (or ones), and no scale was formed
    launch_robust_prior(args->vertex_weights, 1.f, robust->vertex_weights, (size_t)B * t.V, st);
    if (joints) launch_robust_prior(args->joint_weights, 1.f, robust->joint_weights, (size_t)B * t.J, st);
    launch_robust_prior(nullptr, __builtin_nanf(""), robust->scale_out, (size_t)B, st);
  }
  if (recon)
    if (int rc = mesh_error(recon->vertices, recon->joints, recon->vertex_error, recon->joint_error)) return rc;
  return post_launch_check();
}

int smplfit_reload_options(void) {
  (void)tune();  // make sure the first-use load has happened, then replace it
  load_tuning();
  return SMPLFIT_OK;
}

uint64_t smplfit_gemm_plane_launches(void) { return g_gemm_plane_launches.load(std::memory_order_relaxed); }
uint64_t smplfit_rotation_spread_launches(void) { return g_rot_spread_launches.load(std::memory_order_relaxed); }
uint64_t smplfit_stage_launches(int stage_id) {
  if (stage_id < 0 || stage_id >= SMPLFIT_STAGE_COUNT) return 0;
  return g_stage_launches[stage_id].load(std::memory_order_relaxed);
}

int smplfit_time_kernel_f32(const smplfit_handle* h, int kernel_id, int batch, int reps,
                            void* workspace, size_t workspace_bytes, void* hip_stream,
                            float* avg_ms) {
  int rc = check_call("smplfit_time_kernel_f32", h, batch, workspace, workspace_bytes, smplfit_workspace_bytes(h, batch),
                      "smplfit_workspace_bytes");
  if (rc) return rc;
  if (!avg_ms || reps < 1) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_time_kernel_f32: bad argument");
  const DevModel& d = h->d;
  hipStream_t st = (hipStream_t)hip_stream;
  const Workspace ws = fit_workspace(h, batch, workspace);
  hipEvent_t e0, e1;
  SF_HIP_TRY(hipEventCreate(&e0));
  SF_HIP_TRY(hipEventCreate(&e1));
  // time the kernels the default fit runs: target joints given, unit weights, no scale unknown, no shared shape
  const Route r = route_of(h, batch, CallShape{});
  const int Mp = (int)align_up((size_t)batch, 128);
  auto once = [&]() -> int {
    switch (kernel_id) {
      // (a shape solve's GEMM, on the features the last fit's prologue left: planes on the route gemm_planes)
      case SMPLFIT_KERNEL_POSEDIRS_GEMM: return launch_gemm(d, ws, batch, st, r.bm, r.gemm_planes);
      case SMPLFIT_KERNEL_PAIR_GRAM:
        if (!r.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "pair-Gram kernel: batch-major path not active");
        launch_residual_bm(h, ws, batch, st, 2);
        return 0;
      case SMPLFIT_KERNEL_TRANSPOSE:
        if (!r.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "layout kernel: batch-major path not active");
        // the hook has no target pointer: ws.tvs (unused on this path, >= B*V*3 floats) stands in for the rows
        hipLaunchKernelGGL(k_layout_targets, dim3((d.V + kSlabV - 1) / kSlabV, Mp / 64), dim3(256),
                           (size_t)64 * kSlabRow * 4, st, d, ws.tvs, ws.tT, ws.resP, batch, Mp);
        return 0;
      case SMPLFIT_KERNEL_TEMPLATE_PARTSUM:
        if (!r.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "template part sums: batch-major path not active");
        {
          const ShareView sv = share_view(h, sf::kShareLbsUsed, batch);
          hipLaunchKernelGGL(k_template_partsum_bm<false>, share_grid(sv, Mp), dim3(64 * kBW), 0, st, d, sv, ws, batch, Mp);
        }
        return 0;
      case SMPLFIT_KERNEL_SHAPE_ACCUM: {
        if (r.bm) {
          launch_residual_bm(h, ws, batch, st, 1);
          return 0;
        }
        if (int rc = launch_accum_any(d, ws, batch, false, r.pair_in, st, gen_joint_rows(d) ? ws.tjc : nullptr)) return rc;
        return 0;
      }
      case SMPLFIT_KERNEL_SHAPE_SOLVE:
        // (the default fit's solve: k_solve_bm on the partial sums the last fit left, else the wave-per-instance stage)
        if (r.solve_bm) launch_solve_bm(h, r.solve_plan, ws, batch, st, 1.0f, 0.0f, 1.0f, 0, r.prologue_bm);
        else launch_shape_solve(d, ws, batch, st, 1.0f, 0.0f, 1.0f, r.pair_in, 0);
        return 0;
      case SMPLFIT_KERNEL_LBS_PARTSUM: {
        if (r.bm) {
#define SF_CALL_LBS(S_, KW_) launch_lbs_bm<S_, KW_>(h, ws, batch, st, r.psum_combine, false, false, false)
          SF_DISPATCH_SKW(d, SF_CALL_LBS);
#undef SF_CALL_LBS
          return 0;
        }
        if (int rc = launch_lbs_any<0>(d, ws, batch, false, d.S, ws.beta, ws.trans, nullptr, st)) return rc;
        return 0;
      }
      case SMPLFIT_KERNEL_JOINT_STAGE: {  // a rotation pass + prologue on the state of the last fit
        JointStageArgs ja{};
        ja.tj = ws.tjc;
        ja.rj = ws.rjoints;
        ja.rj_shared = 0;
        ja.Gprev = ws.G;
        ja.jw = nullptr;
        ja.fit_rotations = 1;
        ja.do_prologue = 1;
        ja.joint_block = gen_joint_rows(d) ? 0 : 1;
        ja.joint_block_weighted = 0;
        ja.vertex_sa_closed_form = d.general ? 0 : 1;
        // (what a default fit runs: the rotations + k_prologue_bm where that applies)
        launch_joint_stage_fit(h, ja, ws, batch, st, r.prologue_bm, r.rot_kind_next, 1, r.gemm_planes, r.rot_spread);
        return 0;
      }
      case SMPLFIT_KERNEL_REFINE: {  // (outputs into the workspace: ws.tvs is unused between fits)
        RefineArgs ra{};
        ra.tj = ws.tjc;
        ra.rj_term = ws.rjoints;
        ra.jw = nullptr;
        ra.final_adjust = 1;
        float* scratch = r.bm ? ws.tvs : ws.rverts;
        ra.pose = scratch;
        ra.betas = scratch + (size_t)batch * d.J * 3;
        ra.trans = ra.betas + (size_t)batch * d.S;
        ra.kid = nullptr;
        ra.orient = ra.trans + (size_t)batch * 3;  // (a fit always writes the orientations and the relative rotations)
        ra.rel = ra.orient + (size_t)batch * d.J * 9;
        // (what a default fit runs: k_refine_bm on the rows of the last LBS pass where that applies)
        if (r.refine_bm) launch_refine_bm(h, ra, share_view(h, r.refine_kind, batch), ws, batch, st);
        else launch_refine(d, ra, ws, batch, st);
        return 0;
      }
      case SMPLFIT_KERNEL_GRAM_COMBINE:
        if (!r.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "normal-equation combine: batch-major path not active");
        if (r.solve_bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "normal-equation combine: part of k_solve_bm (SMPLFIT_KERNEL_SHAPE_SOLVE)");
        launch_residual_bm(h, ws, batch, st, 4);
        return 0;
      case SMPLFIT_KERNEL_PSUM_COMBINE:
        if (!r.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "part-sum combine: batch-major path not active");
        if (!r.psum_combine) return fail(SMPLFIT_ERR_UNSUPPORTED, "part-sum combine: k_rotations_bm / k_refine_bm add the rows themselves");
        launch_psum_combine(d, share_view(h, sf::kShareLbsUsed, batch), ws, batch, Mp, st);
        return 0;
      case SMPLFIT_KERNEL_JD_TRANSPOSE:
        if (!r.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "joint-row transpose: batch-major path not active");
        if (!r.jd_transpose) return fail(SMPLFIT_ERR_UNSUPPORTED, "joint-row transpose: k_prologue_bm writes ws.jdT itself");
        launch_jd_transpose(d, ws, batch, st);
        return 0;
      case SMPLFIT_KERNEL_MEAN_FINISH:
        if (!r.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "mean pass: batch-major path not active");
        // (the slab sums of the layout pass are gone from ws.resP by now: the values are arbitrary, the work is the same;
        // the outputs go where the fit left them)
        hipLaunchKernelGGL(k_mean_finish, dim3(Mp / 64), dim3(64 * kMeanWaves), 0, st, d, ws.rjoints, ws.resP, ws, batch, Mp,
                           (d.V + kSlabV - 1) / kSlabV);
        return 0;
      case SMPLFIT_KERNEL_LBS_LAST:
        if (!r.bm) return fail(SMPLFIT_ERR_UNSUPPORTED, "last LBS pass: batch-major path not active");
#define SF_CALL_LBS(S_, KW_) launch_lbs_bm<S_, KW_>(h, ws, batch, st, r.psum_combine_last, false, true, false)
        SF_DISPATCH_SKW(d, SF_CALL_LBS);
#undef SF_CALL_LBS
        return 0;
      default: return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_time_kernel_f32: unknown kernel id");
    }
  };
  // Each timed launch runs right after the kernel that precedes it inside a fit (K2 before K3, K3
  // before K5), so caches are in the state the kernel sees in situ; only the target kernel is
  // bracketed by the two events.
  auto pre = [&]() {
    if (kernel_id == SMPLFIT_KERNEL_SHAPE_ACCUM) launch_gemm(d, ws, batch, st, r.bm, r.gemm_planes);
    if ((kernel_id == SMPLFIT_KERNEL_LBS_PARTSUM || kernel_id == SMPLFIT_KERNEL_LBS_LAST) && r.bm) {
      if (r.solve_bm) launch_solve_bm(h, r.solve_plan, ws, batch, st, 1.0f, 0.0f, 1.0f, 0, r.prologue_bm);
      else launch_shape_solve(d, ws, batch, st, 1.0f, 0.0f, 1.0f, r.pair_in, 0);
    }
    if (kernel_id == SMPLFIT_KERNEL_LBS_PARTSUM && !r.bm) {
      if (int rc = launch_accum_any(d, ws, batch, false, r.pair_in, st)) return rc;
    }
    return 0;
  };
  rc = pre();
  if (rc) return rc;
  rc = once();  // warm-up
  if (rc) return rc;
  float total = 0.f;
  for (int r = 0; r < reps; ++r) {
    pre();
    SF_HIP_TRY(hipEventRecord(e0, st));
    once();
    SF_HIP_TRY(hipEventRecord(e1, st));
    SF_HIP_TRY(hipEventSynchronize(e1));
    float ms1 = 0.f;
    SF_HIP_TRY(hipEventElapsedTime(&ms1, e0, e1));
    total += ms1;
  }
  const float ms = total;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_ms = ms / (float)reps;
  return post_launch_check();
}

int smplfit_primitives_f32(int primitive_id, const float* a, const float* b, float* out, int n,
                           void* hip_stream) {
  if (!a || !out || n < 0) return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_primitives_f32: null pointer / negative n");
  if (primitive_id < SMPLFIT_PRIM_PROJ_SO3 || primitive_id > SMPLFIT_PRIM_SWING_TWIST)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_primitives_f32: unknown primitive id");
  if ((primitive_id == SMPLFIT_PRIM_ALIGN_UNIT || primitive_id == SMPLFIT_PRIM_SWING_TWIST) && !b)
    return fail(SMPLFIT_ERR_BAD_ARG, "smplfit_primitives_f32: this primitive takes two inputs");
  if (n == 0) return SMPLFIT_OK;
  hipLaunchKernelGGL(k_primitives, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)hip_stream, primitive_id, a, b,
                     out, n);
  return post_launch_check();
}

}  // extern "C"
