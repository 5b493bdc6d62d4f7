/*
 * smplfit.h — C-ABI of the MI355X-native SMPL-family fitter (libsmplfit_hip.so).
 *
 * Drop-in boundary for ONE hot path of isarandi/smplfitter: smplfitter.pt.BodyFitter.fit()
 * (reference src/smplfitter/pt/bodyfitter.py:283-549) and the LBS forward it is scored with
 * (reference src/smplfitter/pt/bodymodel.py:121-307).  The reference is pure Python/PyTorch and has
 * no FFI of its own; these entry points are what a ctypes binding inside its BodyFitter /
 * BodyModel would call (see INTEGRATION.md for that stub).  Plain pointers and sizes only — no
 * torch types.  All array arguments of the compute calls are DEVICE pointers (HIP, gfx950), fp32,
 * C-contiguous; all work is enqueued on the caller's stream; nothing synchronises the device.
 *
 * Ownership: the handle owns the uploaded model constants and derived tables only.  The caller
 * owns inputs, outputs and the workspace (size from smplfit_workspace_bytes).  A handle is
 * read-only after creation: concurrent calls on different streams are safe if their workspaces
 * are distinct.
 *
 * Errors: every call returns 0 on success or a negative smplfit_status; smplfit_last_error()
 * returns a thread-local message.  No exceptions cross the boundary.  A non-SPD Gramian yields NaN
 * outputs (the reference discards cholesky_ex's info, pt/bodyfitter.py:1083).
 */
#ifndef SMPLFIT_H_
#define SMPLFIT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smplfit_handle smplfit_handle;

typedef enum smplfit_status {
  SMPLFIT_OK = 0,
  SMPLFIT_ERR_BAD_ARG = -1,     /* null pointer, bad size, option conflict                 */
  SMPLFIT_ERR_UNSUPPORTED = -2, /* model shape / option outside what the kernels implement */
  SMPLFIT_ERR_WORKSPACE = -3,   /* workspace too small / misaligned                         */
  SMPLFIT_ERR_HIP = -4,         /* HIP runtime error (no device, launch failure, OOM)       */
} smplfit_status;

/* Model constants as the reference's BodyModel holds them (pt/bodymodel.py:80-93), HOST pointers,
 * fp32, C-contiguous, original vertex order.  Copied during smplfit_create. */
typedef struct smplfit_model_desc {
  int32_t num_vertices;            /* V                                                        */
  int32_t num_joints;              /* J (<= 64)                                                */
  int32_t num_betas;               /* S                                                        */
  int32_t is_smpl_family;          /* model_name.startswith('smpl') (pt/bodyfitter.py:34)      */
  const float* v_template;         /* (V,3)  identity-pose corrective already folded in        */
  const float* shapedirs;          /* (V,3,S)                                                  */
  const float* posedirs;           /* (V,3,9(J-1))                                             */
  const float* weights;            /* (V,J) dense skinning weights                             */
  const float* J_template;         /* (J,3)                                                    */
  const float* J_shapedirs;        /* (J,3,S)                                                  */
  const int32_t* parents;          /* (J) kinematic parents, parents[0] ignored                */
  const float* J_regressor_post_lbs; /* (J, regressor_num_vertices) or NULL                    */
  int32_t regressor_num_vertices;  /* must equal V for the joints-omitted path                 */
  /* kid blend shape (BodyFitter(enable_kid=True), pt/bodyfitter.py:52-58; BodyModel.forward's
   * kid_factor, pt/bodymodel.py:258-295): when enable_kid != 0 the handle carries ONE extra shape
   * unknown whose vertex / joint directions are kid_shapedir / kid_J_shapedir. */
  int32_t enable_kid;
  const float* kid_shapedir;       /* (V,3) or NULL                                            */
  const float* kid_J_shapedir;     /* (J,3) or NULL                                            */
} smplfit_model_desc;

enum { SMPLFIT_CREATE_HOST_ONLY = 1 }; /* build tables, upload nothing (no GPU needed)         */

/* Builds the part / level / sparse-skinning tables of BodyFitter.__init__
 * (pt/bodyfitter.py:25-233) and uploads model + tables to the current HIP device. */
int smplfit_create(const smplfit_model_desc* desc, int flags, smplfit_handle** out);
void smplfit_destroy(smplfit_handle* h);

const char* smplfit_last_error(void);
const char* smplfit_version(void);
/* Version of this header's structs and entry points; bumped whenever a struct gains a field or a signature
 * changes.  A client compares it with the SMPLFIT_ABI_VERSION it was built against before the first call. */
#define SMPLFIT_ABI_VERSION 7
int smplfit_abi_version(void);

typedef struct smplfit_info {
  int32_t num_vertices, num_joints, num_betas; /* num_betas excludes the kid unknown */
  int32_t has_kid;
  int32_t padded_vertices;     /* Vp: vertices padded for the kernels                          */
  int32_t num_used_vertices;   /* vertices entering the part sums (pt/bodyfitter.py:109-114)   */
  int32_t skin_width;          /* (joint, weight) pairs kept per vertex: 4, 8, or — general path — the largest
                                  count of non-zero weights of a vertex rounded up to 4 (up to 64)              */
  int32_t num_segments;        /* part-aligned 64-vertex tiles                                 */
  int32_t num_fk_levels;
  int32_t adj_last_level;
  int32_t has_device;
  int32_t gemm_vgprs;          /* registers per lane of the split-bf16 GEMM kernels as built (0 without a device):
                                  they must own whole CUs (>= 256); below that the fp32-MFMA GEMM runs instead  */
  int32_t vertex_path;         /* which kernels the vertex passes of a default (unit-weight) fit run on:
                                  SMPLFIT_PATH_BATCH_MAJOR (lane = instance, the fast path: <= 8 weights per vertex,
                                  10 or 16 betas with or without the kid unknown, >= 1024 vertices),
                                  SMPLFIT_PATH_WAVE (one wave per instance: small subsets, non-normalised weights —
                                  about 0.4x the rate) or SMPLFIT_PATH_GENERAL (any number of betas up to 1023 / of
                                  skinning weights up to 64: run-time loops, the normal equations as one rank-k
                                  update on the matrix cores, every option of the fit)              */
  int32_t share_fallback;      /* bit k: cell table k (see smplfit_get_share_table) is a copy of a wider or coarser
                                  one because its own domain was too small for its cells; 0xffff: the model has
                                  no cell tables at all (SMPLFIT_PATH_WAVE)                                        */
} smplfit_info;
enum smplfit_vertex_path { SMPLFIT_PATH_WAVE = 0, SMPLFIT_PATH_BATCH_MAJOR = 1, SMPLFIT_PATH_GENERAL = 2 };
int smplfit_get_info(const smplfit_handle* h, smplfit_info* info);

/* Introspection of the host tables, for tests.  Copies up to cap int32 entries, sets *n. */
enum smplfit_table_id {
  SMPLFIT_TAB_PART_ASSIGNMENT = 0, /* (V)  argmax weight, toes->feet                            */
  SMPLFIT_TAB_SORT_PERM = 1,       /* (Vp) original index of sorted slot, -1 = padding          */
  SMPLFIT_TAB_PART_TYPE = 2,       /* (J)  0 none, 1 multi-joint, 2 bone, 3 leaf                */
  SMPLFIT_TAB_FK_ORDER = 3,        /* joints by tree level (pt/bodyfitter.py:181-192)           */
  SMPLFIT_TAB_FK_LEVEL_START = 4,  /* (levels+1)                                                */
  SMPLFIT_TAB_ADJ_FLAG = 5,        /* (J)  1 if refined by the final adjustment                 */
  SMPLFIT_TAB_USED_PART = 6,       /* (J)  1 if the part's vertices enter the part sums         */
  SMPLFIT_TAB_SEGMENTS = 7,        /* (nseg,3) start, count, part                               */
  SMPLFIT_TAB_VERTEX_PIECES = 8,   /* (npieces,5) start, count, part, used, joints: the pieces of the
                                      sorted slots the batch-major vertex kernels walk (runs of one
                                      part with at most four skinning joints)                    */
  SMPLFIT_TAB_JOINT_PAIRS = 10,    /* (npairs,2) joints j1 < j2 that share a vertex: the units of the pair-Gram form  */
  SMPLFIT_TAB_CELL_COUNTS = 9,     /* (8) cells per instance block of the cell tables below: the four kinds'
                                      coarse tables, then their fine ones (empty: the model has no
                                      batch-major tables)                                          */
  /* tables derived for single kernels (any model unless noted) */
  SMPLFIT_TAB_INV_SLOT = 11,       /* (V)  sorted slot of every original vertex                 */
  SMPLFIT_TAB_PART_SEG_START = 12, /* (J+1) first segment of each part, empty range: unused part */
  SMPLFIT_TAB_ANC_START = 13,      /* (J+1) CSR offsets into the next table                     */
  SMPLFIT_TAB_ANC = 14,            /* ancestors of every joint, root first, the joint excluded  */
  SMPLFIT_TAB_ROT_SLOTS = 15,      /* (J)  the joint's slot among the joints a toe copies its rotation
                                      from, numbered by ascending toe; -1 = none                */
  SMPLFIT_TAB_REFINE_WAVES = 16,   /* one value per adjustable part, in level order: the wave (0-7) of the
                                      batch-major refinement kernel that owns it                */
};
int smplfit_get_table(const smplfit_handle* h, int table_id, int32_t* dst, size_t cap, size_t* n);

/* Cell tables of the batch-major vertex kernels (test access): `kind` 0 residual pass, 1 part sums over every slot,
 * 2 over the used parts, 3 over the adjustable parts; 4-7: the FINE tables of the same kinds, which batches of up
 * to SMPLFIT_FINE_B (default 768) instances walk — eight times the cells, a short walk per wave; the rows of partial
 * sums differ, so a small batch agrees with a large one to rounding, not bit for bit.
 * `what` 0 piece_start (ncells + 1), 1 piece records
 * (npieces + 1, 12): count, joints[4], local slots[4], first slot, row closed behind the piece (-1 none), kind 0:
 * joints of that row | (cell + 1) << 8 behind the last piece of a cell; 2 the rows: part per row (kinds 1-3) or
 * (nrows, 12) joint of every local slot, -1 unused (kind 0); 3 aux_start (J + 1) and 4 aux_rows: per joint, CSR, where
 * the combine kernels find its partial sums — the rows of its part, ascending (kinds 1-3), or the offsets of its
 * moments in the residual pass's output, ncells * (S + 6) / 4 * 4 + row * 36 + 3 * local slot in (row, slot) order
 * (kind 0); 5 aux_pad: kind 0 the same as (J, pitch) rows, pitch = the longest run rounded up to 16, -1 behind a
 * joint's last entry; size 0 for kinds 1-3. */
int smplfit_get_share_table(const smplfit_handle* h, int kind, int what, int32_t* dst, size_t cap, size_t* n);
/* Cells per wave a launch over `batch` instances picks for `kind` 0-3 — of the fine table when the batch takes it
 * (with the current tuning options). */
int smplfit_pick_share_mult(const smplfit_handle* h, int kind, int batch);

/* Bytes of device workspace a call on `batch` instances needs (256-byte aligned base). */
size_t smplfit_workspace_bytes(const smplfit_handle* h, int batch);

/*
 * BodyFitter.fit, default configuration (pt/bodyfitter.py:283-549): no share_beta, no scale, no kid,
 * no warm start.
 *   target_vertices (B,V,3); target_joints (B,J,3) or NULL; vertex_weights (B,V) or NULL;
 *   joint_weights (B,J) or NULL.
 * Outputs: pose_rotvecs (B,3J), shape_betas (B,S), trans (B,3); kid_factor (B) (only for kid
 * handles, else NULL), orientations (B,J,3,3) and relative_orientations (B,J,3,3) (parent^T @
 * global, pt/bodyfitter.py:523-533) may be NULL.  kid_regularizer: ridge weight of the kid unknown
 * (the reference defaults it to beta_regularizer, pt/bodyfitter.py:1235-1237); ignored without kid.
 */
int smplfit_fit_f32(const smplfit_handle* h, const float* target_vertices,
                    const float* target_joints, const float* vertex_weights,
                    const float* joint_weights, int batch, int num_iter, float beta_regularizer,
                    float beta_regularizer2, float kid_regularizer, int final_adjust_rots,
                    float* pose_rotvecs, float* shape_betas, float* trans, float* kid_factor,
                    float* orientations, float* relative_orientations, void* workspace,
                    size_t workspace_bytes, void* hip_stream);

/*
 * BodyModel.forward (pt/bodymodel.py:121-307).  Exactly one of pose_rotvecs (B,3J) /
 * glob_rotmats (B,J,3,3) non-NULL; shape_betas (B,num_betas_given) or NULL; trans (B,3) or NULL;
 * kid_factor (B) or NULL (kid handles only).
 * Outputs: vertices (B,V,3) may be NULL (joints only); joints (B,J,3); orientations (B,J,3,3) may
 * be NULL.
 */
int smplfit_forward_f32(const smplfit_handle* h, const float* pose_rotvecs,
                        const float* glob_rotmats, const float* shape_betas, int num_betas_given,
                        const float* trans, const float* kid_factor, int batch, float* vertices,
                        float* joints,
                        float* orientations, void* workspace, size_t workspace_bytes,
                        void* hip_stream);

/* The general form of smplfit_forward_f32: additionally rel_rotmats (B,J,3,3), the relative rotation matrices of
 * BodyModel.forward (pt/bodymodel.py:230-234: global rotations by the kinematic chain, inside the joint kernel).
 * Exactly one of pose_rotvecs / glob_rotmats / rel_rotmats non-NULL (all NULL: rest pose).  Zero-initialise. */
typedef struct smplfit_forward_args {
  const float* pose_rotvecs;   /* (B,3J) or NULL */
  const float* glob_rotmats;   /* (B,J,3,3) or NULL */
  const float* rel_rotmats;    /* (B,J,3,3) or NULL */
  const float* shape_betas;    /* (B,num_betas_given) or NULL */
  int32_t num_betas_given;
  const float* trans;          /* (B,3) or NULL */
  const float* kid_factor;     /* (B) or NULL */
  int32_t batch;
  float* vertices;             /* out (B,V,3) or NULL */
  float* joints;               /* out (B,J,3) */
  float* orientations;         /* out (B,J,3,3) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_forward_args;
int smplfit_forward_ex_f32(const smplfit_handle* h, const smplfit_forward_args* args);

/* Vector-Jacobian product of smplfit_forward_ex_f32 (the backward of BodyModel.forward under autograd).
 * Inputs: the forward's, exactly as in the forward arguments struct (one rotation form or none).  Upstream gradients, each may
 * be NULL (= zero): grad_vertices (B,V,3), grad_joints (B,J,3), grad_orientations (B,J,3,3).  Outputs, each may be
 * NULL (= not wanted): the gradient of the rotation form given (grad_pose_rotvecs (B,3J) | grad_glob_rotmats (B,J,3,3)
 * | grad_rel_rotmats (B,J,3,3)), grad_shape_betas (B,num_betas_given), grad_trans (B,3), grad_kid_factor (B).
 * The call recomputes the forward's joint stage and posedirs product from the inputs (nothing is kept from a forward
 * call); with grad_vertices NULL no vertex-sized kernel runs.  Rotation vectors: the derivative of the exponential
 * map at r = 0 is [e_i]x (the reference's autograd returns 0 there).  Deterministic: no float atomics.
 * Workspace: smplfit_forward_backward_workspace_bytes (its own query; smplfit_workspace_bytes is unchanged).
 * Zero-initialise. */
size_t smplfit_forward_backward_workspace_bytes(const smplfit_handle* h, int batch);
typedef struct smplfit_forward_backward_args {
  const float* pose_rotvecs;       /* (B,3J) or NULL */
  const float* glob_rotmats;       /* (B,J,3,3) or NULL */
  const float* rel_rotmats;        /* (B,J,3,3) or NULL */
  const float* shape_betas;        /* (B,num_betas_given) or NULL */
  int32_t num_betas_given;
  const float* trans;              /* (B,3) or NULL (the gradients do not depend on it) */
  const float* kid_factor;         /* (B) or NULL (kid handles only) */
  int32_t batch;
  const float* grad_vertices;      /* (B,V,3) or NULL */
  const float* grad_joints;        /* (B,J,3) or NULL */
  const float* grad_orientations;  /* (B,J,3,3) or NULL */
  float* grad_pose_rotvecs;        /* out (B,3J) or NULL */
  float* grad_glob_rotmats;        /* out (B,J,3,3) or NULL */
  float* grad_rel_rotmats;         /* out (B,J,3,3) or NULL */
  float* grad_shape_betas;         /* out (B,num_betas_given) or NULL */
  float* grad_trans;               /* out (B,3) or NULL */
  float* grad_kid_factor;          /* out (B) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_forward_backward_args;
int smplfit_forward_backward_f32(const smplfit_handle* h, const smplfit_forward_backward_args* args);

/* BodyModel.rototranslate (pt/bodymodel.py:383-453) for a batch: the body parameters after the rigid transform (R, t),
 *   new_pose_rotvecs = [mat2rotvec(R rotvec2mat(pose[0:3])), pose[3:]]   (pose[3:] copied bit for bit)
 *   pelvis    = J_template[0] + J_shapedirs[0, :, :num_betas_given] shape_betas (+ kid_J_shapedir[0] kid_factor)
 *   new_trans = R trans + t + (R - I) pelvis          (post_translate != 0)
 *   new_trans = R (trans - t) + (R - I) pelvis        (post_translate == 0)
 * so that forward(new_pose_rotvecs, shape_betas, new_trans) = R forward(pose_rotvecs, shape_betas, trans) + t (or
 * R (forward(...) - t)).  R is (B,3,3) with R_per_instance != 0, else one (3,3) for the batch; t likewise (B,3) / (3),
 * or NULL (= 0).  new_pose_rotvecs may be pose_rotvecs itself (in place: only the three root values are written) and
 * new_trans may be trans; the buffers must not overlap in any other way.  One kernel launch on hip_stream, no
 * workspace, no synchronisation; batch == 0 enqueues nothing.  Zero-initialise. */
typedef struct smplfit_rototranslate_args {
  const float* R;              /* (B,3,3) or (3,3) */
  int32_t R_per_instance;
  const float* t;              /* (B,3), (3) or NULL */
  int32_t t_per_instance;
  const float* pose_rotvecs;   /* (B,3J) */
  const float* shape_betas;    /* (B,num_betas_given) or NULL */
  int32_t num_betas_given;
  const float* trans;          /* (B,3) */
  const float* kid_factor;     /* (B) or NULL (kid handles only) */
  int32_t post_translate;
  int32_t batch;
  float* new_pose_rotvecs;     /* out (B,3J) */
  float* new_trans;            /* out (B,3) */
  void* hip_stream;
} smplfit_rototranslate_args;
int smplfit_rototranslate_f32(const smplfit_handle* h, const smplfit_rototranslate_args* args);

/* Vector-Jacobian product of smplfit_rototranslate_f32.  Inputs as in the forward struct.  Upstream gradients, each
 * may be NULL (= zero): grad_new_pose_rotvecs (B,3J), grad_new_trans (B,3).  Outputs, each may be NULL (= not wanted),
 * always one row per instance — the caller sums the rows of what it shared across the batch, so there are no float
 * atomics and the result is deterministic: grad_R (B,3,3), grad_t (B,3), grad_pose_rotvecs (B,3J; may be
 * grad_new_pose_rotvecs itself), grad_shape_betas (B,num_betas_given), grad_trans (B,3), grad_kid_factor (B).
 * At a root rotation vector of exactly 0 the derivative of the exponential map is [e_i]x (the reference's autograd
 * returns 0 there); where the log map's |xyz| is 0 its gradient is 0.  One launch, no workspace.  Zero-initialise. */
typedef struct smplfit_rototranslate_backward_args {
  const float* R;
  int32_t R_per_instance;
  const float* t;
  int32_t t_per_instance;
  const float* pose_rotvecs;
  const float* shape_betas;
  int32_t num_betas_given;
  const float* trans;
  const float* kid_factor;
  int32_t post_translate;
  int32_t batch;
  const float* grad_new_pose_rotvecs;  /* (B,3J) or NULL */
  const float* grad_new_trans;         /* (B,3) or NULL */
  float* grad_R;                       /* out (B,3,3) or NULL */
  float* grad_t;                       /* out (B,3) or NULL */
  float* grad_pose_rotvecs;            /* out (B,3J) or NULL */
  float* grad_shape_betas;             /* out (B,num_betas_given) or NULL */
  float* grad_trans;                   /* out (B,3) or NULL */
  float* grad_kid_factor;              /* out (B) or NULL */
  void* hip_stream;
} smplfit_rototranslate_backward_args;
int smplfit_rototranslate_backward_f32(const smplfit_handle* h, const smplfit_rototranslate_backward_args* args);

/* Value and gradient of the mesh-distance objective in one call (a refinement step of BodyFlipperOpt):
 *   loss[b] = scale * sum_v w_bv |v_bv - t_bv|,   L = sum_b loss[b],
 * v = the vertices of smplfit_forward_ex_f32 at the inputs (trans included), t = target_vertices, w = vertex_weights
 * (NULL: 1).  Outputs: loss (B, required) and the gradients of L, each may be NULL (= not wanted): the gradient of the
 * rotation form given, grad_shape_betas (B,num_betas_given), grad_trans (B,3), grad_kid_factor (B).  The cotangent of
 * a vertex is scale * w * (v - t) / |v - t|, exactly 0 where |v - t| == 0.  The skinned vertex and its cotangent are
 * formed in registers by the vertex pass of the backward: neither reaches memory, and the joint stage and the
 * posedirs product run once.  Rotation vectors at r = 0 and determinism: as smplfit_forward_backward_f32.
 * Serves every model.  Workspace: smplfit_mesh_objective_workspace_bytes.  Zero-initialise. */
size_t smplfit_mesh_objective_workspace_bytes(const smplfit_handle* h, int batch);
typedef struct smplfit_mesh_objective_args {
  const float* pose_rotvecs;       /* (B,3J) or NULL */
  const float* glob_rotmats;       /* (B,J,3,3) or NULL */
  const float* rel_rotmats;        /* (B,J,3,3) or NULL */
  const float* shape_betas;        /* (B,num_betas_given) or NULL */
  int32_t num_betas_given;
  const float* trans;              /* (B,3) or NULL */
  const float* kid_factor;         /* (B) or NULL (kid handles only) */
  int32_t batch;
  const float* target_vertices;    /* (B,V,3) */
  const float* vertex_weights;     /* (B,V) or NULL */
  float scale;
  float* loss;                     /* out (B) */
  float* grad_pose_rotvecs;        /* out (B,3J) or NULL */
  float* grad_glob_rotmats;        /* out (B,J,3,3) or NULL */
  float* grad_rel_rotmats;         /* out (B,J,3,3) or NULL */
  float* grad_shape_betas;         /* out (B,num_betas_given) or NULL */
  float* grad_trans;               /* out (B,3) or NULL */
  float* grad_kid_factor;          /* out (B) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_mesh_objective_args;
int smplfit_mesh_objective_f32(const smplfit_handle* h, const smplfit_mesh_objective_args* args);

/* The mesh-distance objective with a joint term (a refinement step of BodyFitterOpt):
 *   loss[b] = scale * sum_v w_bv |v_bv - t_bv|  +  joint_scale * sum_j u_bj |p_bj - q_bj|,   L = sum_b loss[b],
 * v, t, w as in smplfit_mesh_objective_f32; p = the joints of smplfit_forward_ex_f32 at the inputs (trans included),
 * q = target_joints (B,J,3) or NULL, u = joint_weights (B,J) or NULL (= 1; refused without target_joints).  The
 * cotangent of a joint is joint_scale * u * (p - q) / |p - q|, exactly 0 where |p - q| == 0 or u == 0; the joint terms
 * of an instance are added in joint order.  Outputs and every other field: as smplfit_mesh_objective_f32.  With
 * target_joints NULL the call makes the launches of smplfit_mesh_objective_f32 and returns its bits.
 * Workspace: smplfit_fit_objective_workspace_bytes (the backward's plus a (B,J,3) cotangent).  Zero-initialise. */
size_t smplfit_fit_objective_workspace_bytes(const smplfit_handle* h, int batch);
typedef struct smplfit_fit_objective_args {
  const float* pose_rotvecs;       /* (B,3J) or NULL */
  const float* glob_rotmats;       /* (B,J,3,3) or NULL */
  const float* rel_rotmats;        /* (B,J,3,3) or NULL */
  const float* shape_betas;        /* (B,num_betas_given) or NULL */
  int32_t num_betas_given;
  const float* trans;              /* (B,3) or NULL */
  const float* kid_factor;         /* (B) or NULL (kid handles only) */
  int32_t batch;
  const float* target_vertices;    /* (B,V,3) */
  const float* vertex_weights;     /* (B,V) or NULL */
  float scale;
  const float* target_joints;      /* (B,J,3) or NULL */
  const float* joint_weights;      /* (B,J) or NULL */
  float joint_scale;
  float* loss;                     /* out (B) */
  float* grad_pose_rotvecs;        /* out (B,3J) or NULL */
  float* grad_glob_rotmats;        /* out (B,J,3,3) or NULL */
  float* grad_rel_rotmats;         /* out (B,J,3,3) or NULL */
  float* grad_shape_betas;         /* out (B,num_betas_given) or NULL */
  float* grad_trans;               /* out (B,3) or NULL */
  float* grad_kid_factor;          /* out (B) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_fit_objective_args;
int smplfit_fit_objective_f32(const smplfit_handle* h, const smplfit_fit_objective_args* args);

/* Adjoint of smplfit_shape_solve_ex_f32 (the backward of BodyFitter.fit_with_known_pose under autograd): for fixed
 * global rotations the solve is a weighted ridge least-squares problem in (shape unknowns, trans), and its
 * vector-Jacobian product has a closed form.
 * Inputs: the forward's (rotations, targets, weights, regularisers, ridge references with num_reference_betas) and the
 * forward's results shape_betas (B, the model's betas), trans (B,3) in the frame of the targets AS PASSED (add_mean = 1)
 * and kid_factor (B, kid handles).  Cotangents, each may be NULL (= zero): grad_shape_betas, grad_trans,
 * grad_kid_factor.  Outputs, each may be NULL (= not wanted, no work done for it): the gradients of target_vertices
 * (B,V,3), target_joints (B,J,3), vertex_weights (B,V), joint_weights (B,J) - exactly 0 where the weights rule
 * (both kinds only if both are given with target joints) ignores the weight -, beta_regularizer_reference
 * (B,num_reference_betas), kid_regularizer_reference (B) and glob_rotmats (B,J,3,3; through the pose blend shapes too,
 * as smplfit_forward_ex_f32 with glob_rotmats evaluates them).  The call recomputes what it needs from the inputs and
 * accumulates its own normal matrix, whichever route the forward's solve took; it serves any number of skinning
 * weights and up to 17 shape unknowns (betas + kid; more: SMPLFIT_ERR_UNSUPPORTED); no share_beta, no scale unknown.
 * A system that is not positive definite gives NaN gradients for that instance.  Stream-ordered, no allocation, no
 * synchronisation; deterministic: no float atomics.  Workspace: smplfit_shape_solve_backward_workspace_bytes.
 * Zero-initialise. */
size_t smplfit_shape_solve_backward_workspace_bytes(const smplfit_handle* h, int batch);
typedef struct smplfit_shape_solve_backward_args {
  const float* glob_rotmats;                /* (B,J,3,3) */
  const float* target_vertices;             /* (B,V,3) */
  const float* target_joints;               /* (B,J,3) or NULL */
  const float* vertex_weights;              /* (B,V) or NULL */
  const float* joint_weights;               /* (B,J) or NULL */
  float beta_regularizer, beta_regularizer2, kid_regularizer;
  const float* beta_regularizer_reference;  /* (B,num_reference_betas) or NULL */
  int32_t num_reference_betas;
  const float* kid_regularizer_reference;   /* (B) or NULL */
  int32_t batch;
  const float* shape_betas;                 /* (B, the model's betas): the forward's result */
  const float* trans;                       /* (B,3) */
  const float* kid_factor;                  /* (B), kid handles */
  const float* grad_shape_betas;            /* (B, the model's betas) or NULL */
  const float* grad_trans;                  /* (B,3) or NULL */
  const float* grad_kid_factor;             /* (B) or NULL */
  float* grad_target_vertices;              /* out (B,V,3) or NULL */
  float* grad_target_joints;                /* out (B,J,3) or NULL */
  float* grad_vertex_weights;               /* out (B,V) or NULL */
  float* grad_joint_weights;                /* out (B,J) or NULL */
  float* grad_beta_regularizer_reference;   /* out (B,num_reference_betas) or NULL */
  float* grad_kid_regularizer_reference;    /* out (B) or NULL */
  float* grad_glob_rotmats;                 /* out (B,J,3,3) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_shape_solve_backward_args;
int smplfit_shape_solve_backward_f32(const smplfit_handle* h, const smplfit_shape_solve_backward_args* args);

/* Adjoint of smplfit_fit_ex_f32 (the backward of BodyFitter.fit under autograd): the gradients of
 * the targets and weights of a fit from the cotangents of its results.  Inputs as smplfit_fit_args passes them (no warm
 * start, no share_beta, no scale unknown).  Cotangents, each may be NULL (= zero): grad_pose_rotvecs (B,3J),
 * grad_shape_betas (B, the model's betas), grad_trans (B,3), grad_kid_factor (B, kid handles), grad_orientations,
 * grad_relative_orientations (B,J,3,3).  Outputs, each may be NULL (= not wanted, no output): the gradients of
 * target_vertices (B,V,3), target_joints (B,J,3), vertex_weights (B,V), joint_weights (B,J).  Nothing is kept from the
 * forward call: a forward sweep recomputes the rotations and the solution of every iteration, a reverse sweep
 * alternates the adjoints of the rotation pass and of the refinement with smplfit_forward_backward_f32 and
 * smplfit_shape_solve_backward_f32.  Any number of skinning weights and joints, up to 17 shape unknowns (more:
 * SMPLFIT_ERR_UNSUPPORTED).  An instance whose projection or solve is singular gets non-finite gradients, the others
 * are not touched.  Stream-ordered, no allocation, no synchronisation; deterministic: no float atomics.
 * Workspace: smplfit_fit_backward_workspace_bytes(h, batch, num_iter). */
size_t smplfit_fit_backward_workspace_bytes(const smplfit_handle* h, int batch, int num_iter);
typedef struct smplfit_fit_backward_args {
  const float* target_vertices;             /* (B,V,3) */
  const float* target_joints;               /* (B,J,3) or NULL */
  const float* vertex_weights;              /* (B,V) or NULL */
  const float* joint_weights;               /* (B,J) or NULL */
  int32_t batch;
  int32_t num_iter;
  float beta_regularizer, beta_regularizer2, kid_regularizer;
  int32_t final_adjust_rots;
  const float* grad_pose_rotvecs;           /* (B,3J) or NULL */
  const float* grad_shape_betas;            /* (B, the model's betas) or NULL */
  const float* grad_trans;                  /* (B,3) or NULL */
  const float* grad_kid_factor;             /* (B) or NULL */
  const float* grad_orientations;           /* (B,J,3,3) or NULL */
  const float* grad_relative_orientations;  /* (B,J,3,3) or NULL */
  float* grad_target_vertices;              /* out (B,V,3) or NULL */
  float* grad_target_joints;                /* out (B,J,3) or NULL */
  float* grad_vertex_weights;               /* out (B,V) or NULL */
  float* grad_joint_weights;                /* out (B,J) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_fit_backward_args;
int smplfit_fit_backward_f32(const smplfit_handle* h, const smplfit_fit_backward_args* args);

/* BodyFitter.fit with a warm start (pt/bodyfitter.py:363-382): smplfit_fit_f32 plus
 *   initial_pose_rotvecs (B,3J) or NULL, initial_shape_betas (B,num_initial_betas) or NULL,
 *   initial_kid_factor (B) or NULL (enable_kid handles only).
 * When a pose or betas are given, the first rotation pass runs against the model posed with the initial
 * values (composed with its orientations) instead of the template, and the ridge of every shape solve
 * pulls towards initial_shape_betas / initial_kid_factor (beta/kid_regularizer_reference, :1072-1081,
 * :1224-1255).  All three NULL is exactly smplfit_fit_f32.  This is the call BodyFlipper.flip makes
 * (pt/bodyflipper.py:71-81). */
int smplfit_fit_warm_f32(const smplfit_handle* h, const float* target_vertices,
                         const float* target_joints, const float* vertex_weights,
                         const float* joint_weights, int batch, int num_iter, float beta_regularizer,
                         float beta_regularizer2, float kid_regularizer, int final_adjust_rots,
                         const float* initial_pose_rotvecs, const float* initial_shape_betas,
                         int num_initial_betas, const float* initial_kid_factor, float* pose_rotvecs,
                         float* shape_betas, float* trans, float* kid_factor, float* orientations,
                         float* relative_orientations, void* workspace, size_t workspace_bytes,
                         void* hip_stream);

/* The general form of the fit call: every option of the two entry points above in one struct, plus
 *   share_beta != 0 -- BodyFitter.fit(share_beta=True): one shape (betas [+ kid]) for the whole batch;
 *   the regularised, centred normal equations of all instances are summed before the Cholesky solve
 *   (pt/lstsq.py:24-26 through lstsq_partial_share :32-90 with every unknown shared), every instance
 *   keeps its own translation.  The sum runs over the instances in order on one GPU; when the batch
 *   is sharded over ranks (one process per GPU) `share_allreduce` completes it: after the local sum
 *   of every shape solve the driver calls it once, on the calling thread, and it must ENQUEUE on
 *   `hip_stream` an in-place sum all-reduce of `sums` (device memory, `count` = S*S + S doubles) over
 *   the ranks -- e.g. ncclAllReduce(sums, sums, count, ncclDouble, ncclSum, comm, stream) -- and
 *   return 0.  Every rank then solves the same summed system.  NULL = the batch is the whole batch.
 *   scale_mode -- BodyFitter.fit(scale_target=True) / (scale_fit=True): the LAST shape solve gets one more
 *   unknown, the refinement sees scaled targets resp. a scaled reference, the mean is added back scaled.
 *   shape_betas / kid_factor are returned as the reference returns them (undivided by the scale).
 *   share_beta together with scale_mode: the scaled solve shares the shape and keeps one scale per
 *   instance (lstsq_partial_share with n_shared = S, pt/lstsq.py:50-90): every instance contributes the
 *   Schur complement of its scale entry, the S x S sums are solved once, the scales follow.
 * Zero-initialise the struct; fields left 0 / NULL mean "not given". */
typedef int (*smplfit_share_allreduce_fn)(void* user, double* sums, int32_t count, void* hip_stream);

typedef struct smplfit_fit_args {
  const float* target_vertices;      /* (B,V,3) */
  const float* target_joints;        /* (B,J,3) or NULL */
  const float* vertex_weights;       /* (B,V) or NULL */
  const float* joint_weights;        /* (B,J) or NULL */
  int32_t batch, num_iter;
  float beta_regularizer, beta_regularizer2, kid_regularizer;
  int32_t final_adjust_rots;
  const float* initial_pose_rotvecs; /* (B,3J) or NULL */
  const float* initial_shape_betas;  /* (B,num_initial_betas) or NULL */
  int32_t num_initial_betas;
  const float* initial_kid_factor;   /* (B) or NULL */
  int32_t share_beta;
  int32_t scale_mode;                /* 0; 1 = scale_target, 2 = scale_fit (the last solve, :434-519) */
  float scale_regularizer;
  float* pose_rotvecs;               /* out (B,3J) */
  float* shape_betas;                /* out (B,S) */
  float* trans;                      /* out (B,3) */
  float* kid_factor;                 /* out (B) or NULL */
  float* orientations;               /* out (B,J,3,3) or NULL */
  float* relative_orientations;      /* out (B,J,3,3) or NULL */
  float* scale_corr;                 /* out (B), required with scale_mode != 0 */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
  smplfit_share_allreduce_fn share_allreduce; /* NULL, or the cross-rank sum of a sharded share_beta fit */
  void* share_user;                  /* passed back to share_allreduce */
} smplfit_fit_args;
int smplfit_fit_ex_f32(const smplfit_handle* h, const smplfit_fit_args* args);

/* BodyFitter.fit_with_known_shape (pt/bodyfitter.py:655-838): pose and translation (and, with
 * scale_fit, one scale factor per instance) for KNOWN shape parameters.  num_iter rotation passes
 * against the model posed at the current rotations, then fit_scale_and_translation (:1628-1681) and,
 * with final_adjust_rots, the dependent refinement.
 *   shape_betas (B,num_betas_given) -- betas beyond the handle's count are an error, missing ones are 0
 *   kid_factor (B) or NULL          -- only on a handle created with enable_kid
 *   initial_pose_rotvecs (B,3J) or NULL (rest pose)
 *   target_* / *_weights            -- as smplfit_fit_f32
 * Outputs: pose_rotvecs (B,3J), trans (B,3); scale_corr (B) is written only when scale_fit != 0;
 * orientations / relative_orientations (B,J,3,3) may be NULL.
 * The reference's scale branch multiplies a (B,) scale into (B,3) means and therefore only runs for
 * B == 1 (:1675-1676); here every instance gets its own scale, which is what B == 1 calls return. */
int smplfit_fit_known_shape_f32(const smplfit_handle* h, const float* shape_betas,
                                int num_betas_given, const float* kid_factor,
                                const float* initial_pose_rotvecs, const float* target_vertices,
                                const float* target_joints, const float* vertex_weights,
                                const float* joint_weights, int batch, int num_iter,
                                int final_adjust_rots, int scale_fit, float* pose_rotvecs, float* trans,
                                float* scale_corr, float* orientations, float* relative_orientations,
                                void* workspace, size_t workspace_bytes, void* hip_stream);

/* Adjoint of smplfit_fit_known_shape_f32 without scale_fit and without a warm start (the backward of
 * BodyFitter.fit_with_known_shape under autograd): the gradients of the shape, the targets and the
 * weights from the cotangents of the results.  Inputs as smplfit_fit_known_shape_f32 takes them.  Cotangents, each may
 * be NULL (= zero): grad_pose_rotvecs (B,3J), grad_trans (B,3), grad_orientations, grad_relative_orientations
 * (B,J,3,3).  Outputs, each may be NULL (= not wanted; its share is not computed): the gradients of target_vertices
 * (B,V,3), target_joints (B,J,3), vertex_weights (B,V), joint_weights (B,J), shape_betas (B,num_betas_given) and
 * kid_factor (B).  Nothing is kept from the forward call: a forward sweep recomputes the rotations of every
 * iteration, a reverse sweep runs the adjoints of the output stage, the refinement, the alignment and the rotation
 * passes, each mesh's cotangent through the vector-Jacobian product of smplfit_forward_backward_f32.  Any number of
 * skinning weights and joints; up to 17 shape unknowns (betas + padding + kid: the per-instance refinement adjoint
 * holds them in registers; more: SMPLFIT_ERR_UNSUPPORTED).  Without target_joints the model needs a joint regressor
 * over its vertices (SMPLFIT_ERR_BAD_ARG otherwise, as the forward).  An instance whose projection is singular gets
 * non-finite gradients, the others are not touched.  Stream-ordered, no allocation, no synchronisation;
 * deterministic: no float atomics.  Workspace: smplfit_fit_known_shape_backward_workspace_bytes(h, batch, num_iter). */
size_t smplfit_fit_known_shape_backward_workspace_bytes(const smplfit_handle* h, int batch, int num_iter);
typedef struct smplfit_fit_known_shape_backward_args {
  const float* shape_betas;                 /* (B,num_betas_given) */
  int32_t num_betas_given;
  const float* kid_factor;                  /* (B) or NULL */
  const float* target_vertices;             /* (B,V,3) */
  const float* target_joints;               /* (B,J,3) or NULL */
  const float* vertex_weights;              /* (B,V) or NULL */
  const float* joint_weights;               /* (B,J) or NULL */
  int32_t batch;
  int32_t num_iter;
  int32_t final_adjust_rots;
  const float* grad_pose_rotvecs;           /* (B,3J) or NULL */
  const float* grad_trans;                  /* (B,3) or NULL */
  const float* grad_orientations;           /* (B,J,3,3) or NULL */
  const float* grad_relative_orientations;  /* (B,J,3,3) or NULL */
  float* grad_target_vertices;              /* out (B,V,3) or NULL */
  float* grad_target_joints;                /* out (B,J,3) or NULL */
  float* grad_vertex_weights;               /* out (B,V) or NULL */
  float* grad_joint_weights;                /* out (B,J) or NULL */
  float* grad_shape_betas;                  /* out (B,num_betas_given) or NULL */
  float* grad_kid_factor;                   /* out (B) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_fit_known_shape_backward_args;
int smplfit_fit_known_shape_backward_f32(const smplfit_handle* h, const smplfit_fit_known_shape_backward_args* args);

/* Stage entry points for parity tests. */

/* First rotation pass of fit (pt/bodyfitter.py:384-394 -> _fit_global_rotations :1321-1416):
 * centres the targets, fits every part's global rotation against the template mesh.
 * glob_rotmats (B,J,3,3) out. */
int smplfit_part_rotations_f32(const smplfit_handle* h, const float* target_vertices,
                               const float* target_joints, const float* vertex_weights,
                               const float* joint_weights, int batch, float* glob_rotmats,
                               void* workspace, size_t workspace_bytes, void* hip_stream);

/* One shape solve (pt/bodyfitter.py:840-1102, _fit_shape -> _fit_shape_gram) for given global
 * rotations on targets that are centred internally exactly as fit() does.  add_mean = 0: trans /
 * vertices / joints stay in the centred frame (stage parity tests); add_mean = 1: the target mean is
 * added back to trans, i.e. fit_with_known_pose (pt/bodyfitter.py:552-653) once the caller has turned
 * pose_rotvecs into global rotations.  vertices_out (B,V,3) / joints_out (B,J,3) may be NULL. */
int smplfit_shape_solve_f32(const smplfit_handle* h, const float* glob_rotmats,
                            const float* target_vertices, const float* target_joints,
                            const float* vertex_weights, const float* joint_weights, int batch,
                            float beta_regularizer, float beta_regularizer2, float kid_regularizer,
                            int add_mean, float* shape_betas, float* trans, float* kid_factor,
                            float* vertices_out, float* joints_out, void* workspace,
                            size_t workspace_bytes, void* hip_stream);

/* The general form of smplfit_shape_solve_f32: fit_with_known_pose (pt/bodyfitter.py:552-653) with the
 * options it hands to the shape solve (:623-638 -> _fit_shape_general :1104-1319).
 *   beta_regularizer_reference (B,num_reference_betas) / kid_regularizer_reference (B) -- the values the
 *   ridge pulls towards (:1224-1255); missing betas are 0; ignored with share_beta, as the all-shared
 *   branch of the reference drops them (pt/lstsq.py:45-47)
 *   share_beta, share_allreduce, share_user -- as smplfit_fit_args
 *   scale_mode, scale_regularizer           -- one more unknown (1 scale_target, 2 scale_fit);
 *   scale_corr (B) out; shape_betas / kid_factor as the reference returns them (undivided); with
 *   add_mean the UNSCALED target mean is added to trans (:642-643).  No mesh outputs with a scale.
 * Zero-initialise the struct; fields left 0 / NULL mean "not given". */
typedef struct smplfit_shape_solve_args {
  const float* glob_rotmats;         /* (B,J,3,3) */
  const float* target_vertices;      /* (B,V,3) */
  const float* target_joints;        /* (B,J,3) or NULL */
  const float* vertex_weights;       /* (B,V) or NULL */
  const float* joint_weights;        /* (B,J) or NULL */
  int32_t batch;
  float beta_regularizer, beta_regularizer2, kid_regularizer;
  int32_t add_mean;
  const float* beta_regularizer_reference; /* (B,num_reference_betas) or NULL */
  int32_t num_reference_betas;
  const float* kid_regularizer_reference;  /* (B) or NULL */
  int32_t share_beta;
  int32_t scale_mode;
  float scale_regularizer;
  float* shape_betas;                /* out (B,S) */
  float* trans;                      /* out (B,3) */
  float* kid_factor;                 /* out (B) or NULL */
  float* scale_corr;                 /* out (B), required with scale_mode != 0 */
  float* vertices_out;               /* out (B,V,3) or NULL */
  float* joints_out;                 /* out (B,J,3) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
  smplfit_share_allreduce_fn share_allreduce;
  void* share_user;
} smplfit_shape_solve_args;
int smplfit_shape_solve_ex_f32(const smplfit_handle* h, const smplfit_shape_solve_args* args);

/*
 * Topology transfer — BodyConverter.convert_vertices (pt/bodyconverter.py:128-149): out = M in with the sparse
 * (V_out x V_in) matrix BodyConverter.__init__ loads (pt/bodyconverter.py:31-47; the first V_in columns of the
 * official *_deftrafo_setup.pkl matrix, common.py:425-429).  smplfit_transfer_create copies a CSR matrix (HOST
 * pointers: indptr (V_out + 1), indices / values (nnz)) and uploads it to the current device (flags =
 * SMPLFIT_CREATE_HOST_ONLY: no upload, for tests).  smplfit_transfer_f32: in_vertices (B,V_in,3) ->
 * out_vertices (B,V_out,3), device pointers; the entries of a row are added in CSR order, as the reference's sparse
 * product does.
 * flags | SMPLFIT_TRANSFER_NEGATE_X: the product is followed by x -> -x (BodyFlipper.flip_vertices,
 * pt/bodyflipper.py:99-119: the mirror matrix, then the x axis flipped); every use of the matrix — smplfit_transfer_f32
 * and the fused calls — honours it.  Other flag bits are rejected.
 */
enum { SMPLFIT_TRANSFER_NEGATE_X = 2 };
typedef struct smplfit_transfer smplfit_transfer;
int smplfit_transfer_create(int32_t num_vertices_in, int32_t num_vertices_out, const int32_t* indptr,
                            const int32_t* indices, const float* values, int flags, smplfit_transfer** out);
void smplfit_transfer_destroy(smplfit_transfer* t);
int smplfit_transfer_f32(const smplfit_transfer* t, const float* in_vertices, int batch, float* out_vertices,
                         void* hip_stream);
/* Adjoint of smplfit_transfer_f32: grad_in (B,V_in,3) = M^T grad_out (B,V_out,3); with SMPLFIT_TRANSFER_NEGATE_X the x
 * component is negated as well (the negation is diagonal and commutes with the product).  The entries of an input
 * vertex are added in ascending output-row order: deterministic, no float atomics.  An input vertex that no row
 * uses gets exactly 0.  Device pointers, stream-ordered, no workspace, no allocation, no synchronisation.
 * Refusals as smplfit_transfer_f32 (null pointer / negative batch: SMPLFIT_ERR_BAD_ARG; a host-only matrix:
 * SMPLFIT_ERR_HIP), with ONE difference: a batch of 0 returns SMPLFIT_OK before the matrix is looked at, so also for a
 * host-only matrix, where smplfit_transfer_f32 refuses the host-only matrix first. */
int smplfit_transfer_backward_f32(const smplfit_transfer* t, const float* grad_out_vertices, int batch,
                                  float* grad_in_vertices, void* hip_stream);

/*
 * BodyConverter.convert, default branch (pt/bodyconverter.py:49-126: forward of the input model :86, convert_vertices
 * :87, fit of the output model with enable_kid :110-117), as ONE call that keeps every intermediate in the kernels'
 * own instance-innermost layout: the input model's posed vertices never leave their stream buffer, the transfer writes
 * the output model's target stream directly (no (B,V,3) intermediates, no layout pass).
 *   smplfit_convert_plan_create(in, out, transfer, &plan): `in` = handle of body_model_in (no kid unknown), `out` =
 *   handle of body_model_out (normally created with enable_kid, as BodyConverter's fitter is), `transfer` = NULL for
 *   models of one topology (identity).  Returns SMPLFIT_ERR_UNSUPPORTED when one of the models is outside what the
 *   batch-major kernels take — the caller then runs smplfit_forward_f32 + smplfit_transfer_f32 + smplfit_fit_f32.
 *   The plan borrows the two handles (keep them alive) and owns its re-indexed copy of the matrix.
 *   smplfit_convert_f32: inputs pose_rotvecs (B,3 J_in), shape_betas (B,num_betas_given) or NULL, trans (B,3) or NULL
 *   of the INPUT model (its mesh is evaluated without kid_factor, as the reference does); the fit options of
 *   smplfit_fit_f32 (the reference passes beta_regularizer = 0, final_adjust_rots = 0, kid_regularizer = 1e9 or 0);
 *   outputs as smplfit_fit_f32 for the OUTPUT model.  Workspace: smplfit_convert_workspace_bytes(plan, batch).
 */
typedef struct smplfit_convert_plan smplfit_convert_plan;
int smplfit_convert_plan_create(const smplfit_handle* in, const smplfit_handle* out, const smplfit_transfer* transfer,
                                smplfit_convert_plan** plan);
void smplfit_convert_plan_destroy(smplfit_convert_plan* plan);
size_t smplfit_convert_workspace_bytes(const smplfit_convert_plan* plan, int batch);
typedef struct smplfit_convert_args {
  const float* pose_rotvecs;         /* (B,3 J_in) */
  const float* shape_betas;          /* (B,num_betas_given) or NULL */
  int32_t num_betas_given;
  const float* trans;                /* (B,3) or NULL */
  int32_t batch, num_iter;
  float beta_regularizer, beta_regularizer2, kid_regularizer;
  int32_t final_adjust_rots;
  float* out_pose_rotvecs;           /* (B,3 J_out) */
  float* out_shape_betas;            /* (B,S_out) */
  float* out_trans;                  /* (B,3) */
  float* out_kid_factor;             /* (B) or NULL */
  float* out_orientations;           /* (B,J_out,3,3) or NULL */
  float* out_relative_orientations;  /* (B,J_out,3,3) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_convert_args;
int smplfit_convert_f32(const smplfit_convert_plan* plan, const smplfit_convert_args* args);

/*
 * BodyFlipper.flip (pt/bodyflipper.py:34-92) as ONE call: forward of the input parameters WITH kid_factor, the mirror
 * transfer (a smplfit_transfer made with SMPLFIT_TRANSFER_NEGATE_X) straight into the fit's target stream, the naively
 * flipped pose (joints permuted, rotation vectors times (1,-1,-1), pt/bodyflipper.py:121-133) written to the
 * workspace, and the fit warm-started from that pose and the input betas (first rotation pass against the model posed
 * with them; ridge reference = the input betas).  No (B,V,3) intermediate is written and nothing synchronises.
 *   smplfit_flip_plan_create(h, mirror, joint_perm, &plan): `h` = handle of the model with the kid unknown (the
 *   flipper's BodyFitter(enable_kid=True)), `mirror` = (V x V) transfer, `joint_perm` (J) = the joint mirror map
 *   (HOST pointer; must be in range and an involution).  SMPLFIT_ERR_UNSUPPORTED where the batch-major kernels do not
 *   take the model — the caller then runs forward + smplfit_transfer_f32 + smplfit_fit_warm_f32.  The plan borrows
 *   the handle (keep it alive) and owns its re-indexed copy of the matrix and of the permutation.
 *   smplfit_flip_f32: inputs pose_rotvecs (B,3J), shape_betas (B,num_betas_given) or NULL, trans (B,3) or NULL,
 *   kid_factor (B) or NULL (the input mesh is evaluated with it); fit options as smplfit_fit_f32 (the reference passes
 *   beta_regularizer = beta_regularizer2 = 1e-2, final_adjust_rots = 1, kid_regularizer = 1e9 without kid_factor,
 *   else 0); outputs as smplfit_fit_f32.  Workspace: smplfit_flip_workspace_bytes(plan, batch).
 */
typedef struct smplfit_flip_plan smplfit_flip_plan;
int smplfit_flip_plan_create(const smplfit_handle* h, const smplfit_transfer* mirror, const int32_t* joint_perm,
                             smplfit_flip_plan** plan);
void smplfit_flip_plan_destroy(smplfit_flip_plan* plan);
size_t smplfit_flip_workspace_bytes(const smplfit_flip_plan* plan, int batch);
typedef struct smplfit_flip_args {
  const float* pose_rotvecs;         /* (B,3J) */
  const float* shape_betas;          /* (B,num_betas_given) or NULL */
  int32_t num_betas_given;
  const float* trans;                /* (B,3) or NULL */
  const float* kid_factor;           /* (B) or NULL */
  int32_t batch, num_iter;
  float beta_regularizer, beta_regularizer2, kid_regularizer;
  int32_t final_adjust_rots;
  float* out_pose_rotvecs;           /* (B,3J) */
  float* out_shape_betas;            /* (B,S) */
  float* out_trans;                  /* (B,3) */
  float* out_kid_factor;             /* (B) or NULL */
  float* out_orientations;           /* (B,J,3,3) or NULL */
  float* out_relative_orientations;  /* (B,J,3,3) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_flip_args;
int smplfit_flip_f32(const smplfit_flip_plan* plan, const smplfit_flip_args* args);

/*
 * HandReplacer.replace_hand (pt/handreplacer.py:61-74) as ONE call: the vertex-weighted fit of the model to the input
 * meshes (no target joints, no warm start), the fitted relative rotations of a joint range overwritten with constant
 * replacement rotations, the forward of the edited parameters, and the blend with the input mesh,
 *   out[b,v] = in[b,v] + (new[b,v] - in[b,v]) * mix[v],
 * exactly in[b,v] where mix[v] == 0.  The weights of the fit are ONE (V) vector for the whole batch, read as such: no
 * (B,V) weight tensor exists.  The fit runs on the route its model and call take (a weighted fit with more than 10
 * betas: the wave-per-instance kernels); the forward runs on the batch-major kernels from the relative rotation
 * matrices, and the new mesh is blended where it is written: no (B,V,3) intermediate.  Nothing synchronises.
 *   smplfit_replace_hands_plan_create(h, fit_weights, mix_weights, num_vertices, first_joint, num_joints, rotvecs,
 *   num_rotvec_values, &plan): `h` = handle WITHOUT the kid unknown; fit_weights / mix_weights (num_vertices = V) and
 *   rotvecs (num_rotvec_values = 3 num_joints: the rotation vectors of the joints [first_joint, first_joint +
 *   num_joints)) are HOST pointers.  SMPLFIT_ERR_BAD_ARG for a length that does not match or a range outside [0, J);
 *   SMPLFIT_ERR_UNSUPPORTED where the batch-major kernels do not take the model's forward, for a kid handle and for a
 *   model without its joint regressor — the caller then runs smplfit_fit_f32 + smplfit_forward_f32 and blends.  The plan
 *   borrows the handle (keep it alive) and owns device copies of the three vectors.
 *   smplfit_replace_hands_f32: vertices (B,V,3) in, out_vertices (B,V,3) out (may be the same buffer); the fit options
 *   of smplfit_fit_f32 (the reference passes num_iter = 3, beta_regularizer = 0, final_adjust_rots = 0);
 *   out_pose_rotvecs / out_shape_betas / out_trans: the EDITED parameters, each may be NULL.
 *   Workspace: smplfit_replace_hands_workspace_bytes(plan, batch).  Zero-initialise the struct.
 */
typedef struct smplfit_replace_hands_plan smplfit_replace_hands_plan;
int smplfit_replace_hands_plan_create(const smplfit_handle* h, const float* fit_weights, const float* mix_weights,
                                      int32_t num_vertices, int32_t first_joint, int32_t num_joints, const float* rotvecs,
                                      int32_t num_rotvec_values, smplfit_replace_hands_plan** plan);
void smplfit_replace_hands_plan_destroy(smplfit_replace_hands_plan* plan);
size_t smplfit_replace_hands_workspace_bytes(const smplfit_replace_hands_plan* plan, int batch);
typedef struct smplfit_replace_hands_args {
  const float* vertices;             /* (B,V,3) */
  int32_t batch, num_iter;
  float beta_regularizer, beta_regularizer2;
  int32_t final_adjust_rots;
  float* out_vertices;               /* (B,V,3) */
  float* out_pose_rotvecs;           /* (B,3J) or NULL */
  float* out_shape_betas;            /* (B,S) or NULL */
  float* out_trans;                  /* (B,3) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_replace_hands_args;
int smplfit_replace_hands_f32(const smplfit_replace_hands_plan* plan, const smplfit_replace_hands_args* args);

/* ---- share_beta over segments of the batch: many tracks in one call -----------
 * A plan of segments cuts the batch into consecutive runs of rows — `sizes`, a HOST array of `count` positive sizes
 * that sum to the batch — and a call with it solves one shape (and one kid factor) per run, as share_beta does for a
 * whole batch: the rows of a run get exactly the bits of a share_beta call on those rows alone.  Every option of
 * share_beta holds (weights, num_iter, ridge weights, warm starts, kid, the scale options: one shape per run, one
 * scale per row).  The sum of a run's systems has a fixed order that depends on the sizes alone (blocks of 64 rows
 * counted from the run's first row, then the run's partial rows; no atomics).
 *   smplfit_share_segments_create: SMPLFIT_ERR_BAD_ARG for count < 1, a size < 1 or a sum beyond INT32_MAX; flags:
 *   SMPLFIT_CREATE_HOST_ONLY builds the tables without a device (the calls below then refuse the plan).  The plan
 *   owns device copies of its tables on the device that was current at creation and may serve any handle there.
 *   smplfit_share_segments_get_table: `what` 0 the run of every row (batch), 1 per run (first partial block, blocks),
 *   2 per partial block (first row, rows); the calling convention of smplfit_get_table.
 *   smplfit_fit_segments_f32 / smplfit_shape_solve_segments_f32: the _ex calls with a plan.  share_beta is implied;
 *   args->batch must equal the plan's and share_allreduce must be NULL (SMPLFIT_ERR_BAD_ARG).  With a NULL plan they
 *   ARE the _ex calls.  Workspace: smplfit_share_segments_workspace_bytes(h, batch, plan) — with a NULL plan the value
 *   of smplfit_workspace_bytes(h, batch); 0 for a batch that is not the plan's. */
typedef struct smplfit_share_segments smplfit_share_segments;
int smplfit_share_segments_create(const int32_t* sizes, int32_t count, int32_t flags, smplfit_share_segments** out);
void smplfit_share_segments_destroy(smplfit_share_segments* plan);
int32_t smplfit_share_segments_batch(const smplfit_share_segments* plan);
int smplfit_share_segments_get_table(const smplfit_share_segments* plan, int what, int32_t* dst, size_t cap, size_t* n);
size_t smplfit_share_segments_workspace_bytes(const smplfit_handle* h, int batch, const smplfit_share_segments* plan);
int smplfit_fit_segments_f32(const smplfit_handle* h, const smplfit_fit_args* args, const smplfit_share_segments* plan);
int smplfit_shape_solve_segments_f32(const smplfit_handle* h, const smplfit_shape_solve_args* args,
                                     const smplfit_share_segments* plan);

/* ---- mesh error: the model at given parameters, measured against the targets ----------
 * What follows a fit: the parametric mesh and joints at its parameters, and how far each vertex and joint lies from
 * its target.
 *   vertices (B,V,3), joints (B,J,3)   the forward at the inputs (the bits of smplfit_forward_ex_f32)
 *   vertex_error (B,V)                 |vertices[b,v] - target_vertices[b,v]|, Euclidean
 *   joint_error (B,J)                  |joints[b,j] - target_joints[b,j]|
 * The errors are unweighted.  A non-finite target or parameter row gives non-finite values in that row alone.  Each of
 * the four outputs may be NULL, at least one must be given (SMPLFIT_ERR_BAD_ARG); joint_error without target_joints
 * is SMPLFIT_ERR_BAD_ARG.  Where `vertices` is NULL on the batch-major kernels no (B,V,3) is written anywhere.  A
 * refused call enqueues nothing and leaves the outputs as they were.  Zero-initialise the structs.
 *   smplfit_mesh_error_f32: the step on its own.  The inputs of the forward's argument struct: one rotation form or none, betas,
 *   kid, trans; target_vertices (required) and target_joints.  Workspace: smplfit_mesh_error_workspace_bytes(h, batch).
 *   smplfit_fit_recon_f32: smplfit_fit_segments_f32 (plan may be NULL) followed, on the same stream, by the step at
 *   the fit's own orientations, shape_betas, kid_factor and trans against the fit's targets.  Every result of the fit
 *   keeps the bits of the call without reconstruction.  args->scale_mode != 0: SMPLFIT_ERR_UNSUPPORTED.  A NULL
 *   `recon` makes it smplfit_fit_segments_f32.  Workspace (args->workspace): smplfit_fit_recon_workspace_bytes(h,
 *   batch, plan); 0 for a batch that is not the plan's. */
typedef struct smplfit_mesh_error_args {
  const float* pose_rotvecs;   /* (B,3J) or NULL */
  const float* glob_rotmats;   /* (B,J,3,3) or NULL */
  const float* rel_rotmats;    /* (B,J,3,3) or NULL */
  const float* shape_betas;    /* (B,num_betas_given) or NULL */
  int32_t num_betas_given;
  const float* trans;          /* (B,3) or NULL */
  const float* kid_factor;     /* (B) or NULL */
  int32_t batch;
  const float* target_vertices; /* (B,V,3) */
  const float* target_joints;   /* (B,J,3) or NULL */
  float* vertices;             /* out (B,V,3) or NULL */
  float* joints;               /* out (B,J,3) or NULL */
  float* vertex_error;         /* out (B,V) or NULL */
  float* joint_error;          /* out (B,J) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_mesh_error_args;
size_t smplfit_mesh_error_workspace_bytes(const smplfit_handle* h, int batch);
int smplfit_mesh_error_f32(const smplfit_handle* h, const smplfit_mesh_error_args* args);
typedef struct smplfit_fit_recon_args {
  float* vertices;             /* out (B,V,3) or NULL */
  float* joints;               /* out (B,J,3) or NULL */
  float* vertex_error;         /* out (B,V) or NULL */
  float* joint_error;          /* out (B,J) or NULL; needs args->target_joints */
} smplfit_fit_recon_args;
size_t smplfit_fit_recon_workspace_bytes(const smplfit_handle* h, int batch, const smplfit_share_segments* plan);
int smplfit_fit_recon_f32(const smplfit_handle* h, const smplfit_fit_args* args, const smplfit_share_segments* plan,
                          const smplfit_fit_recon_args* recon);

/* ---- aligned errors: the model moved onto the targets before it is measured -------------
 * Per row: model points x_n, target points y_n, weights w_n >= 0 (NULL = 1), W = sum w_n, weighted means xbar, ybar,
 * K = sum w_n (y_n - ybar)(x_n - xbar)^T.  The error of a point is |s R x_n + t - y_n|, unweighted, with
 *   none          s = 1, R = I, t = 0                     (the bits of smplfit_mesh_error_f32)
 *   root          s = 1, R = I, t = y_root - x_root       (joint 0; needs target_joints; both sets get it)
 *   translation   s = 1, R = I, t = ybar - xbar
 *   rigid         s = 1, R = proj_SO3(K) (det +1 also where the best orthogonal fit is a reflection), t = ybar - R xbar
 *   similarity    s = tr(R^T K) / sum w_n |x_n - xbar|^2, R as rigid, t = ybar - s R xbar
 * align_on: each (the vertices are aligned on the vertices, the joints on the joints: PA-PVE and PA-MPJPE), vertices
 * or joints (one transform from that set for both).  The row means are sum w_n e_n / W over a set, accumulated in fp64
 * in a fixed order and rounded once.  A row whose W is 0, whose spread is 0 under similarity, or that holds a
 * non-finite point or a negative or non-finite weight in the set that gives a transform gets NaN errors, means and
 * transform under that transform; no other row is affected (with root the set is the joints; the weights of a set
 * always enter its own mean).  The model moves, the target stays.  Two runs give the same bits: no float atomics.
 *   smplfit_mesh_error_aligned_f32: smplfit_mesh_error_f32 with an alignment.  A NULL `align` makes it that call.
 *   Outputs: the four of the argument struct, the two means and the transforms: scale / rotation / translation the
 *   vertices' (with align_on = joints, and with root, the joints'), joint_* the joints' own with align_on = each.
 *   `vertices` keeps the forward's bits, unaligned.  SMPLFIT_ERR_BAD_ARG, before anything is enqueued and with the
 *   outputs untouched: an unknown align or align_on; root, align_on = joints or any joint output or joint_weights
 *   without target_joints; no output at all; a transform output with none; joint_* without align_on = each.  With
 *   an alignment the mesh is written as (B,V,3), to `vertices` or into the workspace, on every kernel route.
 *   Stream-ordered: no allocation, no synchronisation.  Workspace: smplfit_mesh_error_aligned_workspace_bytes(h, batch),
 *   the most any call takes; its last three regions, B*V*12, B*V*4 and B*J*4 bytes (each rounded up to 256), stand
 *   in for `vertices`, `vertex_error` and `joint_error`, and a call that is given one of these buffers may leave that
 *   region off.
 *   smplfit_align_points_f32: the step on two arbitrary (B,N,3) arrays, no handle: translation, rigid or similarity.
 *   Workspace: smplfit_align_points_workspace_bytes(batch, num_points); 0 for a batch < 1,
 *   num_points outside [1, 2^26] or batch * num_points above 2^38, which the call refuses (SMPLFIT_ERR_BAD_ARG). */
enum smplfit_align_mode {
  SMPLFIT_ALIGN_NONE = 0,
  SMPLFIT_ALIGN_ROOT = 1,
  SMPLFIT_ALIGN_TRANSLATION = 2,
  SMPLFIT_ALIGN_RIGID = 3,
  SMPLFIT_ALIGN_SIMILARITY = 4,
};
enum smplfit_align_on {
  SMPLFIT_ALIGN_ON_EACH = 0,
  SMPLFIT_ALIGN_ON_VERTICES = 1,
  SMPLFIT_ALIGN_ON_JOINTS = 2,
};
typedef struct smplfit_mesh_align_args {
  int32_t align;               /* smplfit_align_mode */
  int32_t align_on;            /* smplfit_align_on */
  const float* vertex_weights; /* (B,V) or NULL */
  const float* joint_weights;  /* (B,J) or NULL */
  float* mean_vertex_error;    /* out (B) or NULL */
  float* mean_joint_error;     /* out (B) or NULL */
  float* scale;                /* out (B) or NULL */
  float* rotation;             /* out (B,3,3) or NULL */
  float* translation;          /* out (B,3) or NULL */
  float* joint_scale;          /* out (B) or NULL */
  float* joint_rotation;       /* out (B,3,3) or NULL */
  float* joint_translation;    /* out (B,3) or NULL */
} smplfit_mesh_align_args;
size_t smplfit_mesh_error_aligned_workspace_bytes(const smplfit_handle* h, int batch);
int smplfit_mesh_error_aligned_f32(const smplfit_handle* h, const smplfit_mesh_error_args* args,
                                   const smplfit_mesh_align_args* align);
typedef struct smplfit_align_points_args {
  int32_t batch, num_points;
  const float* source;         /* (B,N,3): the points that move */
  const float* target;         /* (B,N,3) */
  const float* weights;        /* (B,N) or NULL */
  int32_t align;               /* smplfit_align_mode: translation, rigid or similarity */
  float* error;                /* out (B,N) or NULL */
  float* mean_error;           /* out (B) or NULL */
  float* scale;                /* out (B) or NULL */
  float* rotation;             /* out (B,3,3) or NULL */
  float* translation;          /* out (B,3) or NULL */
  void* workspace;
  size_t workspace_bytes;
  void* hip_stream;
} smplfit_align_points_args;
size_t smplfit_align_points_workspace_bytes(int batch, int num_points);
int smplfit_align_points_f32(const smplfit_align_points_args* args);

/* ---- robust reweighting and the reweighted fit ------------------------------------------
 * Weights that take gross outliers out of a fit, from the per-point errors of the fit before: per row b a scale
 * sigma_b, then w = w0 * psi(e / (tuning * sigma_b)) for the row's vertices and, with the same sigma_b, joints.
 *   psi(u): huber min(1, 1/u); cauchy 1 / (1 + u^2); geman_mcclure 1 / (1 + u^2)^2; tukey (1 - u^2)^2 for u < 1, else
 *   exactly 0.  fp32, IEEE division, no transcendental.
 *   sigma_b: `scale` > 0: that value for every row; else `scale_rows` (B) if given; else max(1.4826f * med_b,
 *   scale_floor), med_b the LOWER median — element (n - 1) / 2 of the n sorted values — of the row's vertex errors whose
 *   prior weight is > 0 (all of them without prior weights), an exact selection; no such entry: scale_floor.
 * Errors are magnitudes (the sign bit is ignored); prior weights w0 (NULL = 1) are meant non-negative, a prior weight
 * of 0 gives exactly 0.  A row that holds a non-finite error, vertex or joint, gets NaN scale and NaN weights throughout
 * (entries with a zero prior weight included); so does a row whose scale_rows entry is not positive and finite, which
 * only the device can see.  No other row is affected.  SMPLFIT_ERR_BAD_ARG: an unknown loss, tuning <= 0, scale < 0, scale together with
 * scale_rows, scale_floor <= 0 where the median is the source, non-finite numbers.  A refused call enqueues nothing.
 *   smplfit_robust_weights_f32: the step on its own, one launch, no handle and no workspace: the counts are free.
 *   joint_error NULL (or num_joint_errors 0): vertices alone.  out_scale may be NULL.  Outputs may not alias inputs.
 *   smplfit_fit_robust_f32: round 0 is the fit of smplfit_fit_recon_f32 (args, plan).  Each of the num_rounds later
 *   rounds runs the mesh-error step at the previous round's results (errors into the workspace, no mesh written), the
 *   reweighting with args->vertex_weights / joint_weights as the prior weights, and the fit again with the new weights
 *   (both kinds whenever there are target joints), warm-started from the previous round's pose_rotvecs alone, with
 *   round_num_iter rotation passes (0: args->num_iter).  The results are those of the last round; vertex_weights /
 *   joint_weights / scale_out receive the weights and scales that produced it (num_rounds = 0: the prior weights or
 *   ones, and NaN scales; the fit's results are then the bits of smplfit_fit_recon_f32).  `recon` (may be NULL): the
 *   mesh-error step once more at the final results.  A plan of segments and share_beta hold in every round; sigma stays
 *   per row.  Refused: args->scale_mode != 0 (SMPLFIT_ERR_UNSUPPORTED), share_allreduce, initial_pose_rotvecs /
 *   initial_shape_betas / initial_kid_factor, num_rounds < 0, round_num_iter < 0, the joint_weights output without
 *   target_joints (SMPLFIT_ERR_BAD_ARG).  Stream-ordered: no allocation, no synchronisation.  Workspace
 *   (args->workspace): smplfit_fit_robust_workspace_bytes(h, batch, plan); 0 for a batch that is not the plan's. */
enum smplfit_robust_loss {
  SMPLFIT_ROBUST_HUBER = 0,
  SMPLFIT_ROBUST_CAUCHY = 1,
  SMPLFIT_ROBUST_GEMAN_MCCLURE = 2,
  SMPLFIT_ROBUST_TUKEY = 3,
};
typedef struct smplfit_robust_weights_args {
  int32_t batch, num_vertex_errors, num_joint_errors;
  const float* vertex_error;   /* (B,num_vertex_errors) */
  const float* joint_error;    /* (B,num_joint_errors) or NULL */
  const float* vertex_weights; /* prior (B,num_vertex_errors) or NULL */
  const float* joint_weights;  /* prior (B,num_joint_errors) or NULL */
  int32_t loss;                /* smplfit_robust_loss */
  float tuning;
  float scale;                 /* > 0: fixed sigma; 0: not given */
  const float* scale_rows;     /* (B) or NULL */
  float scale_floor;
  float* out_vertex_weights;   /* out (B,num_vertex_errors) */
  float* out_joint_weights;    /* out (B,num_joint_errors); required with joint_error */
  float* out_scale;            /* out (B) or NULL */
  void* hip_stream;
} smplfit_robust_weights_args;
int smplfit_robust_weights_f32(const smplfit_robust_weights_args* args);
typedef struct smplfit_fit_robust_args {
  int32_t loss;                /* smplfit_robust_loss */
  float tuning;
  float scale;                 /* > 0: fixed sigma; 0: not given */
  const float* scale_rows;     /* (B) or NULL */
  float scale_floor;
  int32_t num_rounds;          /* reweighted rounds behind the first fit, >= 0 */
  int32_t round_num_iter;      /* num_iter of the later rounds; 0: args->num_iter */
  float* vertex_weights;       /* out (B,V) or NULL */
  float* joint_weights;        /* out (B,J) or NULL; needs args->target_joints */
  float* scale_out;            /* out (B) or NULL */
} smplfit_fit_robust_args;
size_t smplfit_fit_robust_workspace_bytes(const smplfit_handle* h, int batch, const smplfit_share_segments* plan);
int smplfit_fit_robust_f32(const smplfit_handle* h, const smplfit_fit_args* args, const smplfit_share_segments* plan,
                           const smplfit_fit_recon_args* recon, const smplfit_fit_robust_args* robust);

/* Re-reads the SMPLFIT_* tuning variables (INTEGRATION.md lists them).  They are read once, at first use; tests and
 * the A/B tools that switch kernel paths inside one process call this after changing the environment.  Not to be
 * called while other threads are inside the library. */
int smplfit_reload_options(void);

/* Posedirs GEMM launches of this process that read the pose features as the split-bf16 planes the fit's prologue
 * kernel wrote (the default where it applies; SMPLFIT_GEMM_PLANES=0: none).  Both front ends give the same bits, so
 * this count is the one way to tell which ran: tests and A/B tools read it before and after a call. */
uint64_t smplfit_gemm_plane_launches(void);

/* Launches of the stage kernels of a fit by this process, one count per kernel: which of the lane = instance kernels
 * (k_rotations_bm, k_prologue_bm, k_solve_bm, k_refine_bm) or of their wave-per-instance counterparts served a call is
 * decided per call (route_of) and does not show in the results, which agree to rounding or to the bit.  The counts are
 * process-wide, incremented on the host with relaxed atomics where the kernel is enqueued, and meant for tests and A/B
 * tools: take the difference around a synchronised call, with no other thread inside the library.  A kernel launched in
 * two parts for one batch (two instances a wave + the odd last instance) counts once.  An unknown id gives 0. */
enum smplfit_stage_id {
  SMPLFIT_STAGE_ROTATIONS_BM = 0,        /* k_rotations_bm: part rotations, lane = instance, one round (<= 32 joints) */
  SMPLFIT_STAGE_ROTATIONS_BM_ROUNDS = 1, /* k_rotations_bm_rounds: the same in rounds of 32 joints                   */
  SMPLFIT_STAGE_PROLOGUE_BM_S10 = 2,     /* k_prologue_bm<10>: the shape prologue, 10 shape unknowns                  */
  SMPLFIT_STAGE_PROLOGUE_BM_S11 = 3,     /* k_prologue_bm<11>: 10 betas + the kid unknown                             */
  SMPLFIT_STAGE_SOLVE_BM = 4,            /* k_solve_bm: normal-equation combine + solve, lane = instance              */
  SMPLFIT_STAGE_REFINE_BM = 5,           /* k_refine_bm: refinement + epilogue, lane = instance                       */
  SMPLFIT_STAGE_GT_TO_G = 6,             /* k_gt_to_g: rotations back to instance-major in front of k_refine_epilogue */
  SMPLFIT_STAGE_JOINT_STAGE = 7,         /* k_joint_stage (wave per instance): rotations and / or the prologue        */
  SMPLFIT_STAGE_GRAM_COMBINE = 8,        /* k_gram_combine_bm (fine tables: k_gram_combine_split)                     */
  SMPLFIT_STAGE_SHAPE_SOLVE = 9,         /* k_shape_solve (wave per instance)                                         */
  SMPLFIT_STAGE_REFINE_EPILOGUE = 10,    /* k_refine_epilogue (wave per instance)                                     */
  SMPLFIT_STAGE_PSUM_COMBINE = 11,       /* k_psum_combine (fine tables: k_psum_combine_split)                        */
  SMPLFIT_STAGE_COUNT = 12,
};
uint64_t smplfit_stage_launches(int stage_id);

/* Part-rotation launches of this process that ran as k_rotations_spread: a joint per wave, the joints of a block of 64
 * instances spread over ceil(J / 8) workgroups.  Fit calls of up to 4096 instances (SMPLFIT_ROT_SPREAD_B) run it
 * wherever SMPLFIT_STAGE_ROTATIONS_BM / _ROUNDS count; larger calls, and every call with SMPLFIT_ROT_SPREAD=0, run
 * k_rotations_bm / k_rotations_bm_rounds.  Both forms give the same bits and count under the same stage id, so this
 * count is the one way to tell which ran. */
uint64_t smplfit_rotation_spread_launches(void);

/* Measurement hook (bench.py's roofline leg): launches ONE kernel of the fit `reps` times on
 * `hip_stream` between two HIP events recorded on that same stream and returns the average
 * duration in milliseconds.  The workspace must hold the state a preceding smplfit_fit_f32 call on
 * the same batch left behind.  Synchronises the stream (it is a measurement, not a product call). */
enum smplfit_kernel_id {
  SMPLFIT_KERNEL_POSEDIRS_GEMM = 2, /* K2 v_posed = v_template + pose_feature . posedirs          */
  SMPLFIT_KERNEL_SHAPE_ACCUM = 3,   /* K3 vertex block of the normal equations (batch-major path:
                                       the residual pass k_residual_bm)                            */
  SMPLFIT_KERNEL_SHAPE_SOLVE = 4,   /* K4 fp64 Cholesky solve                                      */
  SMPLFIT_KERNEL_LBS_PARTSUM = 5,   /* K5 vertices at the solution + part sums                     */
  SMPLFIT_KERNEL_PAIR_GRAM = 6,     /* batch-major path: Gramian from the rotations (k_pair_gram_bm) */
  SMPLFIT_KERNEL_TRANSPOSE = 7,     /* batch-major path: targets to the instance-innermost, part-sorted
                                       layout in one pass (k_layout_targets)                        */
  SMPLFIT_KERNEL_TEMPLATE_PARTSUM = 8, /* batch-major path: part sums against the template (first
                                       rotation estimate, k_template_partsum_bm)                    */
  /* the remaining launches of a default fit, so that a caller can attribute the whole step (bench.py's
   * roofline.kernel_ms / fit_breakdown): */
  SMPLFIT_KERNEL_JOINT_STAGE = 9,   /* K1 part rotations + shape prologue (k_joint_stage)            */
  SMPLFIT_KERNEL_REFINE = 10,       /* K6 dependent refinement + epilogue (k_refine_epilogue)       */
  SMPLFIT_KERNEL_GRAM_COMBINE = 11, /* batch-major path: partial sums -> normal-equation record     */
  SMPLFIT_KERNEL_PSUM_COMBINE = 12, /* batch-major path: rows of part sums -> (B, J, 16)            */
  SMPLFIT_KERNEL_JD_TRANSPOSE = 13, /* batch-major path: joint rows instance-innermost              */
  SMPLFIT_KERNEL_MEAN_FINISH = 14,  /* batch-major path: mean of the targets, centred joints        */
  SMPLFIT_KERNEL_LBS_LAST = 15,     /* batch-major path: the last LBS / part-sum pass (adjustable parts only) + combine */
};
int smplfit_time_kernel_f32(const smplfit_handle* h, int kernel_id, int batch, int reps,
                            void* workspace, size_t workspace_bytes, void* hip_stream,
                            float* avg_ms);

/* Test hook: the rotation primitives of the joint-level kernels, evaluated ON THE DEVICE (the
 * arithmetic that ships: hardware rsq / rcp seeds + Newton steps inside proj_SO3), one element per
 * thread, so that the reference's primitive goldens incl. the degenerate inputs (rank 1 / rank 2 /
 * reflection / zero matrices, all four mat2rotvec branches, (anti)parallel vectors) are checked
 * against the device code and not only against its host build.  Device pointers.
 *   PROJ_SO3      a (n,3,3) -> out (n,3,3)   pt/rotation.py:100-110
 *   ROTVEC2MAT    a (n,3)   -> out (n,3,3)   pt/rotation.py:236-258
 *   MAT2ROTVEC    a (n,3,3) -> out (n,3)     pt/rotation.py:261-289
 *   ALIGN_UNIT    a, b (n,3) -> out (n,3,3)  pt/rotation.py:210-224
 *   SWING_TWIST   a = b_ref (n,3), b = [b_tgt | A] (n,12) -> out (n,3,3)  pt/bodyfitter.py:1389-1412 */
enum smplfit_primitive_id {
  SMPLFIT_PRIM_PROJ_SO3 = 0,
  SMPLFIT_PRIM_ROTVEC2MAT = 1,
  SMPLFIT_PRIM_MAT2ROTVEC = 2,
  SMPLFIT_PRIM_ALIGN_UNIT = 3,
  SMPLFIT_PRIM_SWING_TWIST = 4,
};
int smplfit_primitives_f32(int primitive_id, const float* a, const float* b, float* out, int n,
                           void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SMPLFIT_H_ */
