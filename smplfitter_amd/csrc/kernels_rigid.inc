// ================================================================================================
// BodyModel.rototranslate and its backward (smplfit_rototranslate_f32, smplfit_rototranslate_backward_f32): one launch
// each, no workspace.  grid ceil(B / 256), block 256.
//   k_rototranslate            lane = instance: sf::rototranslate_instance (root rotation, R cur, log map, pelvis,
//                              translation); the block then copies the rows of its 256 instances from pose to new_pose
//   k_rototranslate_backward   lane = instance: sf::rototranslate_instance_backward; the same copy carries the pose
//                              cotangent through
// The (B, 3J) rows of a block are ONE contiguous run of floats, moved by rigid_copy_rows: consecutive lanes move
// consecutive floats, 16 bytes per lane where both pointers allow it (3J = 72 or 165 floats: a row is not 16-byte
// aligned in general, the run of a block of 256 rows is whenever the array is), dwords otherwise.  The root's three
// floats of every row are written by the lane that owns the instance, after the copy and a barrier.
// Gradients are per row: what the caller shares across the batch (R, t, betas, kid) it sums itself — no float atomics.
// ================================================================================================
constexpr int kRigidBlock = 256;

struct RigidInputs {
  const float* j_ext;    // JointTabs::j_ext (joint 0 is read)
  int S, J3;             // shape unknowns of the handle, floats per pose row
  const float *R, *t;    // (B, 9) / (9); (B, 3) / (3) / NULL
  int R_stride, t_stride;  // floats between the instances' R / t: 9 / 3, or 0 for one shared by the batch
  const float *pose, *betas, *kid, *trans;  // (B, 3J), (B, nb) / NULL, (B) / NULL, (B, 3)
  int nb, post;
};

// dst[0, n) = src[0, n) (src NULL: zeros) by the 256 threads of a block
__device__ __forceinline__ void rigid_copy_rows(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
  const int tid = threadIdx.x;
  if (!src) {
    for (size_t i = tid; i < n; i += kRigidBlock) dst[i] = 0.f;
    return;
  }
  size_t done = 0;
  if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {  // (the same in every lane)
    const size_t n4 = n >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (size_t i = tid; i < n4; i += kRigidBlock) d4[i] = s4[i];
    done = n4 << 2;
  }
  for (size_t i = done + tid; i < n; i += kRigidBlock) dst[i] = src[i];
}

__global__ __launch_bounds__(kRigidBlock) void k_rototranslate(RigidInputs a, float* new_pose, float* new_trans, int B) {
  const int b0 = blockIdx.x * kRigidBlock, b = b0 + threadIdx.x;
  const bool live = b < B;
  float root[3], tr[3];
  if (live) {
    // the instance's own root is read before anything of new_pose is written (new_pose may be pose)
    float R[9], t[3], rt[3], x[3];
    for (int k = 0; k < 9; ++k) R[k] = a.R[(size_t)b * a.R_stride + k];
    for (int c = 0; c < 3; ++c) {
      if (a.t) t[c] = a.t[(size_t)b * a.t_stride + c];
      rt[c] = a.pose[(size_t)b * a.J3 + c];
      x[c] = a.trans[(size_t)b * 3 + c];
    }
    sf::rototranslate_instance(a.j_ext, a.S, R, a.t ? t : nullptr, rt, a.betas ? a.betas + (size_t)b * a.nb : nullptr,
                               a.betas ? a.nb : 0, a.kid ? a.kid + b : nullptr, x, a.post != 0, root, tr);
  }
  if (new_pose != a.pose) {
    const size_t o = (size_t)b0 * a.J3, n = (size_t)min(kRigidBlock, B - b0) * a.J3;
    rigid_copy_rows(new_pose + o, a.pose + o, n);
    __syncthreads();  // the copy wrote the old roots: the new ones follow it
  }
  if (live)
    for (int c = 0; c < 3; ++c) {
      new_pose[(size_t)b * a.J3 + c] = root[c];
      new_trans[(size_t)b * 3 + c] = tr[c];
    }
}

struct RigidGrads {
  const float *g_pose, *g_trans;  // cotangents of new_pose (B, 3J) / new_trans (B, 3); NULL = 0
  float *gR, *gt, *gpose, *gbetas, *gtrans, *gkid;  // out, each NULL = not wanted: (B, 9), (B, 3), (B, 3J), (B, nb), (B, 3), (B)
};

__global__ __launch_bounds__(kRigidBlock) void k_rototranslate_backward(RigidInputs a, RigidGrads g, int B) {
  const int b0 = blockIdx.x * kRigidBlock, b = b0 + threadIdx.x;
  const bool live = b < B;
  float groot[3];
  if (live) {
    float R[9], t[3], rt[3], x[3], gr[3], gx[3], gR[9], gt[3], gtr[3];
    for (int k = 0; k < 9; ++k) R[k] = a.R[(size_t)b * a.R_stride + k];
    for (int c = 0; c < 3; ++c) {
      if (a.t) t[c] = a.t[(size_t)b * a.t_stride + c];
      rt[c] = a.pose[(size_t)b * a.J3 + c];
      x[c] = a.trans[(size_t)b * 3 + c];
      if (g.g_pose) gr[c] = g.g_pose[(size_t)b * a.J3 + c];
      if (g.g_trans) gx[c] = g.g_trans[(size_t)b * 3 + c];
    }
    sf::rototranslate_instance_backward(
        a.j_ext, a.S, R, a.t ? t : nullptr, rt, a.betas ? a.betas + (size_t)b * a.nb : nullptr, a.betas ? a.nb : 0,
        a.kid ? a.kid + b : nullptr, x, a.post != 0, g.g_pose ? gr : nullptr, g.g_trans ? gx : nullptr,
        g.gR ? gR : nullptr, g.gt ? gt : nullptr, groot, g.gbetas ? g.gbetas + (size_t)b * a.nb : nullptr,
        g.gtrans ? gtr : nullptr, g.gkid ? g.gkid + b : nullptr);
    if (g.gR)
      for (int k = 0; k < 9; ++k) g.gR[(size_t)b * 9 + k] = gR[k];
    for (int c = 0; c < 3; ++c) {
      if (g.gt) g.gt[(size_t)b * 3 + c] = gt[c];
      if (g.gtrans) g.gtrans[(size_t)b * 3 + c] = gtr[c];
    }
  }
  if (!g.gpose) return;  // (the same in every lane)
  if (g.gpose != g.g_pose) {
    const size_t o = (size_t)b0 * a.J3, n = (size_t)min(kRigidBlock, B - b0) * a.J3;
    rigid_copy_rows(g.gpose + o, g.g_pose ? g.g_pose + o : nullptr, n);
    __syncthreads();
  }
  if (live)
    for (int c = 0; c < 3; ++c) g.gpose[(size_t)b * a.J3 + c] = groot[c];
}
