"""ctypes binding of ``libsmplfit_hip.so`` (the C-ABI of ``include/smplfit.h``).

The shared library is built in-tree by ``smplfitter_amd.build`` (``hipcc --offload-arch=gfx950``).
There is NO fallback: if the library is missing or a call fails, an exception is raised — the product
path never routes through a CPU implementation.
"""

from __future__ import annotations

import ctypes as C
import os
import os.path as osp

import numpy as np

_HERE = osp.dirname(osp.abspath(__file__))
# SMPLFIT_LIB: another build of the same library (A/B measurements of kernel variants)
LIB_PATH = os.getenv('SMPLFIT_LIB') or osp.join(_HERE, 'libsmplfit_hip.so')

SMPLFIT_OK = 0
SMPLFIT_ERR_BAD_ARG = -1
SMPLFIT_ERR_UNSUPPORTED = -2
SMPLFIT_PATH_WAVE, SMPLFIT_PATH_BATCH_MAJOR, SMPLFIT_PATH_GENERAL = 0, 1, 2  # smplfit_info.vertex_path
SMPLFIT_ERR_WORKSPACE = -3
SMPLFIT_ERR_HIP = -4
SMPLFIT_CREATE_HOST_ONLY = 1
SMPLFIT_TRANSFER_NEGATE_X = 2  # smplfit_transfer_create: x -> -x after the product (the mirror)
SMPLFIT_ABI_VERSION = 7  # include/smplfit.h; checked against smplfit_abi_version() when the library is loaded

# smplfit_stage_id: the stage kernels smplfit_stage_launches counts
STAGE_IDS = dict(
    rotations_bm=0, rotations_bm_rounds=1, prologue_bm_s10=2, prologue_bm_s11=3, solve_bm=4, refine_bm=5, gt_to_g=6,
    joint_stage=7, gram_combine=8, shape_solve=9, refine_epilogue=10, psum_combine=11,
)

TABLE_IDS = dict(
    part_assignment=0, sort_perm=1, part_type=2, fk_order=3, fk_level_start=4, adj_flag=5,
    used_part=6, segments=7, vertex_pieces=8, cell_counts=9, joint_pairs=10,
    inv_slot=11, part_seg_start=12, anc_start=13, anc=14, rot_slots=15, refine_waves=16,
)

# every symbol include/smplfit.h declares
EXPORTED_SYMBOLS = [
    'smplfit_create', 'smplfit_destroy', 'smplfit_last_error', 'smplfit_version',
    'smplfit_get_info', 'smplfit_get_table', 'smplfit_workspace_bytes', 'smplfit_fit_f32',
    'smplfit_forward_f32', 'smplfit_part_rotations_f32', 'smplfit_shape_solve_f32',
    'smplfit_shape_solve_ex_f32', 'smplfit_fit_known_shape_f32', 'smplfit_fit_warm_f32', 'smplfit_fit_ex_f32',
    'smplfit_time_kernel_f32', 'smplfit_primitives_f32', 'smplfit_forward_ex_f32',
    'smplfit_transfer_create', 'smplfit_transfer_destroy', 'smplfit_transfer_f32', 'smplfit_transfer_backward_f32',
    'smplfit_convert_plan_create', 'smplfit_convert_plan_destroy', 'smplfit_convert_workspace_bytes',
    'smplfit_convert_f32', 'smplfit_flip_plan_create', 'smplfit_flip_plan_destroy', 'smplfit_flip_workspace_bytes',
    'smplfit_flip_f32', 'smplfit_reload_options', 'smplfit_get_share_table', 'smplfit_pick_share_mult',
    'smplfit_abi_version', 'smplfit_forward_backward_workspace_bytes', 'smplfit_forward_backward_f32',
    'smplfit_mesh_objective_workspace_bytes', 'smplfit_mesh_objective_f32',
    'smplfit_fit_objective_workspace_bytes', 'smplfit_fit_objective_f32',
    'smplfit_replace_hands_plan_create', 'smplfit_replace_hands_plan_destroy',
    'smplfit_replace_hands_workspace_bytes', 'smplfit_replace_hands_f32',
    'smplfit_shape_solve_backward_workspace_bytes', 'smplfit_shape_solve_backward_f32',
    'smplfit_fit_backward_workspace_bytes', 'smplfit_fit_backward_f32',
    'smplfit_fit_known_shape_backward_workspace_bytes', 'smplfit_fit_known_shape_backward_f32',
    'smplfit_share_segments_create', 'smplfit_share_segments_destroy', 'smplfit_share_segments_batch',
    'smplfit_share_segments_get_table', 'smplfit_share_segments_workspace_bytes', 'smplfit_fit_segments_f32',
    'smplfit_shape_solve_segments_f32', 'smplfit_gemm_plane_launches', 'smplfit_stage_launches',
    'smplfit_rotation_spread_launches', 'smplfit_rototranslate_f32', 'smplfit_rototranslate_backward_f32',
    'smplfit_mesh_error_workspace_bytes', 'smplfit_mesh_error_f32', 'smplfit_fit_recon_workspace_bytes',
    'smplfit_fit_recon_f32', 'smplfit_robust_weights_f32', 'smplfit_fit_robust_workspace_bytes', 'smplfit_fit_robust_f32',
    'smplfit_mesh_error_aligned_workspace_bytes', 'smplfit_mesh_error_aligned_f32',
    'smplfit_align_points_workspace_bytes', 'smplfit_align_points_f32',
]  # fmt: skip

# the result keys of the mesh-error step (BodyFitter.fit(requested_keys=...), BodyModel.mesh_error)
RECON_KEYS = ('vertices', 'joints', 'vertex_error', 'joint_error')

# smplfit_robust_loss, and the tuning constant BodyFitter.fit_robust picks for each (an API default: the classical 95 %
# efficiency values of Huber, Cauchy and Tukey; 3 for Geman-McClure)
ROBUST_LOSSES = dict(huber=0, cauchy=1, geman_mcclure=2, tukey=3)
ROBUST_TUNING = dict(huber=1.345, cauchy=2.385, geman_mcclure=3.0, tukey=4.685)

# smplfit_align_mode / smplfit_align_on (aligned errors)
ALIGN_MODES = dict(none=0, root=1, translation=2, rigid=3, similarity=4)
ALIGN_ON = dict(each=0, vertices=1, joints=2)

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


# smplfit_share_allreduce_fn: int (*)(void* user, double* sums, int32_t count, void* hip_stream)
ShareAllreduceFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)


class FitArgs(C.Structure):
    """smplfit_fit_args (include/smplfit.h)."""
    _fields_ = [
        ('target_vertices', C.c_void_p), ('target_joints', C.c_void_p), ('vertex_weights', C.c_void_p),
        ('joint_weights', C.c_void_p), ('batch', C.c_int32), ('num_iter', C.c_int32),
        ('beta_regularizer', C.c_float), ('beta_regularizer2', C.c_float), ('kid_regularizer', C.c_float),
        ('final_adjust_rots', C.c_int32), ('initial_pose_rotvecs', C.c_void_p),
        ('initial_shape_betas', C.c_void_p), ('num_initial_betas', C.c_int32),
        ('initial_kid_factor', C.c_void_p), ('share_beta', C.c_int32), ('scale_mode', C.c_int32),
        ('scale_regularizer', C.c_float), ('pose_rotvecs', C.c_void_p),
        ('shape_betas', C.c_void_p), ('trans', C.c_void_p), ('kid_factor', C.c_void_p),
        ('orientations', C.c_void_p), ('relative_orientations', C.c_void_p), ('scale_corr', C.c_void_p),
        ('workspace', C.c_void_p),
        ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
        ('share_allreduce', ShareAllreduceFn), ('share_user', C.c_void_p),
    ]


class ShapeSolveArgs(C.Structure):
    """smplfit_shape_solve_args (include/smplfit.h)."""
    _fields_ = [
        ('glob_rotmats', C.c_void_p), ('target_vertices', C.c_void_p), ('target_joints', C.c_void_p),
        ('vertex_weights', C.c_void_p), ('joint_weights', C.c_void_p), ('batch', C.c_int32),
        ('beta_regularizer', C.c_float), ('beta_regularizer2', C.c_float), ('kid_regularizer', C.c_float),
        ('add_mean', C.c_int32), ('beta_regularizer_reference', C.c_void_p),
        ('num_reference_betas', C.c_int32), ('kid_regularizer_reference', C.c_void_p),
        ('share_beta', C.c_int32), ('scale_mode', C.c_int32), ('scale_regularizer', C.c_float),
        ('shape_betas', C.c_void_p), ('trans', C.c_void_p), ('kid_factor', C.c_void_p),
        ('scale_corr', C.c_void_p), ('vertices_out', C.c_void_p), ('joints_out', C.c_void_p),
        ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
        ('share_allreduce', ShareAllreduceFn), ('share_user', C.c_void_p),
    ]


class ForwardArgs(C.Structure):
    """smplfit_forward_args (include/smplfit.h)."""
    _fields_ = [
        ('pose_rotvecs', C.c_void_p), ('glob_rotmats', C.c_void_p), ('rel_rotmats', C.c_void_p),
        ('shape_betas', C.c_void_p), ('num_betas_given', C.c_int32), ('trans', C.c_void_p),
        ('kid_factor', C.c_void_p), ('batch', C.c_int32), ('vertices', C.c_void_p), ('joints', C.c_void_p),
        ('orientations', C.c_void_p), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t),
        ('hip_stream', C.c_void_p),
    ]


class MeshErrorArgs(C.Structure):
    """smplfit_mesh_error_args (include/smplfit.h)."""
    _fields_ = [
        ('pose_rotvecs', C.c_void_p), ('glob_rotmats', C.c_void_p), ('rel_rotmats', C.c_void_p),
        ('shape_betas', C.c_void_p), ('num_betas_given', C.c_int32), ('trans', C.c_void_p),
        ('kid_factor', C.c_void_p), ('batch', C.c_int32), ('target_vertices', C.c_void_p),
        ('target_joints', C.c_void_p), ('vertices', C.c_void_p), ('joints', C.c_void_p),
        ('vertex_error', C.c_void_p), ('joint_error', C.c_void_p), ('workspace', C.c_void_p),
        ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
    ]


class MeshAlignArgs(C.Structure):
    """smplfit_mesh_align_args (include/smplfit.h)."""
    _fields_ = [
        ('align', C.c_int32), ('align_on', C.c_int32), ('vertex_weights', C.c_void_p), ('joint_weights', C.c_void_p),
        ('mean_vertex_error', C.c_void_p), ('mean_joint_error', C.c_void_p), ('scale', C.c_void_p),
        ('rotation', C.c_void_p), ('translation', C.c_void_p), ('joint_scale', C.c_void_p),
        ('joint_rotation', C.c_void_p), ('joint_translation', C.c_void_p),
    ]


class AlignPointsArgs(C.Structure):
    """smplfit_align_points_args (include/smplfit.h)."""
    _fields_ = [
        ('batch', C.c_int32), ('num_points', C.c_int32), ('source', C.c_void_p), ('target', C.c_void_p),
        ('weights', C.c_void_p), ('align', C.c_int32), ('error', C.c_void_p), ('mean_error', C.c_void_p),
        ('scale', C.c_void_p), ('rotation', C.c_void_p), ('translation', C.c_void_p), ('workspace', C.c_void_p),
        ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
    ]


class FitReconArgs(C.Structure):
    """smplfit_fit_recon_args (include/smplfit.h)."""
    _fields_ = [('vertices', C.c_void_p), ('joints', C.c_void_p), ('vertex_error', C.c_void_p),
                ('joint_error', C.c_void_p)]


class RobustWeightsArgs(C.Structure):
    """smplfit_robust_weights_args (include/smplfit.h)."""
    _fields_ = [
        ('batch', C.c_int32), ('num_vertex_errors', C.c_int32), ('num_joint_errors', C.c_int32),
        ('vertex_error', C.c_void_p), ('joint_error', C.c_void_p), ('vertex_weights', C.c_void_p),
        ('joint_weights', C.c_void_p), ('loss', C.c_int32), ('tuning', C.c_float), ('scale', C.c_float),
        ('scale_rows', C.c_void_p), ('scale_floor', C.c_float), ('out_vertex_weights', C.c_void_p),
        ('out_joint_weights', C.c_void_p), ('out_scale', C.c_void_p), ('hip_stream', C.c_void_p),
    ]


class FitRobustArgs(C.Structure):
    """smplfit_fit_robust_args (include/smplfit.h)."""
    _fields_ = [
        ('loss', C.c_int32), ('tuning', C.c_float), ('scale', C.c_float), ('scale_rows', C.c_void_p),
        ('scale_floor', C.c_float), ('num_rounds', C.c_int32), ('round_num_iter', C.c_int32),
        ('vertex_weights', C.c_void_p), ('joint_weights', C.c_void_p), ('scale_out', C.c_void_p),
    ]


class ForwardBackwardArgs(C.Structure):
    """smplfit_forward_backward_args (include/smplfit.h)."""
    _fields_ = [
        ('pose_rotvecs', C.c_void_p), ('glob_rotmats', C.c_void_p), ('rel_rotmats', C.c_void_p),
        ('shape_betas', C.c_void_p), ('num_betas_given', C.c_int32), ('trans', C.c_void_p),
        ('kid_factor', C.c_void_p), ('batch', C.c_int32), ('grad_vertices', C.c_void_p), ('grad_joints', C.c_void_p),
        ('grad_orientations', C.c_void_p), ('grad_pose_rotvecs', C.c_void_p), ('grad_glob_rotmats', C.c_void_p),
        ('grad_rel_rotmats', C.c_void_p), ('grad_shape_betas', C.c_void_p), ('grad_trans', C.c_void_p),
        ('grad_kid_factor', C.c_void_p), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t),
        ('hip_stream', C.c_void_p),
    ]


_RIGID_INPUTS = [
    ('R', C.c_void_p), ('R_per_instance', C.c_int32), ('t', C.c_void_p), ('t_per_instance', C.c_int32),
    ('pose_rotvecs', C.c_void_p), ('shape_betas', C.c_void_p), ('num_betas_given', C.c_int32),
    ('trans', C.c_void_p), ('kid_factor', C.c_void_p), ('post_translate', C.c_int32), ('batch', C.c_int32),
]


class RototranslateArgs(C.Structure):
    """smplfit_rototranslate_args (include/smplfit.h)."""
    _fields_ = _RIGID_INPUTS + [
        ('new_pose_rotvecs', C.c_void_p), ('new_trans', C.c_void_p), ('hip_stream', C.c_void_p),
    ]


class RototranslateBackwardArgs(C.Structure):
    """smplfit_rototranslate_backward_args (include/smplfit.h)."""
    _fields_ = _RIGID_INPUTS + [
        ('grad_new_pose_rotvecs', C.c_void_p), ('grad_new_trans', C.c_void_p), ('grad_R', C.c_void_p),
        ('grad_t', C.c_void_p), ('grad_pose_rotvecs', C.c_void_p), ('grad_shape_betas', C.c_void_p),
        ('grad_trans', C.c_void_p), ('grad_kid_factor', C.c_void_p), ('hip_stream', C.c_void_p),
    ]


class ShapeSolveBackwardArgs(C.Structure):
    """smplfit_shape_solve_backward_args (include/smplfit.h)."""
    _fields_ = [
        ('glob_rotmats', C.c_void_p), ('target_vertices', C.c_void_p), ('target_joints', C.c_void_p),
        ('vertex_weights', C.c_void_p), ('joint_weights', C.c_void_p), ('beta_regularizer', C.c_float),
        ('beta_regularizer2', C.c_float), ('kid_regularizer', C.c_float), ('beta_regularizer_reference', C.c_void_p),
        ('num_reference_betas', C.c_int32), ('kid_regularizer_reference', C.c_void_p), ('batch', C.c_int32),
        ('shape_betas', C.c_void_p), ('trans', C.c_void_p), ('kid_factor', C.c_void_p),
        ('grad_shape_betas', C.c_void_p), ('grad_trans', C.c_void_p), ('grad_kid_factor', C.c_void_p),
        ('grad_target_vertices', C.c_void_p), ('grad_target_joints', C.c_void_p), ('grad_vertex_weights', C.c_void_p),
        ('grad_joint_weights', C.c_void_p), ('grad_beta_regularizer_reference', C.c_void_p),
        ('grad_kid_regularizer_reference', C.c_void_p), ('grad_glob_rotmats', C.c_void_p),
        ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
    ]


class FitBackwardArgs(C.Structure):
    """smplfit_fit_backward_args (include/smplfit.h)."""
    _fields_ = [
        ('target_vertices', C.c_void_p), ('target_joints', C.c_void_p), ('vertex_weights', C.c_void_p),
        ('joint_weights', C.c_void_p), ('batch', C.c_int32), ('num_iter', C.c_int32),
        ('beta_regularizer', C.c_float), ('beta_regularizer2', C.c_float), ('kid_regularizer', C.c_float),
        ('final_adjust_rots', C.c_int32), ('grad_pose_rotvecs', C.c_void_p), ('grad_shape_betas', C.c_void_p),
        ('grad_trans', C.c_void_p), ('grad_kid_factor', C.c_void_p), ('grad_orientations', C.c_void_p),
        ('grad_relative_orientations', C.c_void_p), ('grad_target_vertices', C.c_void_p),
        ('grad_target_joints', C.c_void_p), ('grad_vertex_weights', C.c_void_p), ('grad_joint_weights', C.c_void_p),
        ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
    ]


class FitKnownShapeBackwardArgs(C.Structure):
    """smplfit_fit_known_shape_backward_args (include/smplfit.h)."""
    _fields_ = [
        ('shape_betas', C.c_void_p), ('num_betas_given', C.c_int32), ('kid_factor', C.c_void_p),
        ('target_vertices', C.c_void_p), ('target_joints', C.c_void_p), ('vertex_weights', C.c_void_p),
        ('joint_weights', C.c_void_p), ('batch', C.c_int32), ('num_iter', C.c_int32), ('final_adjust_rots', C.c_int32),
        ('grad_pose_rotvecs', C.c_void_p), ('grad_trans', C.c_void_p), ('grad_orientations', C.c_void_p),
        ('grad_relative_orientations', C.c_void_p), ('grad_target_vertices', C.c_void_p),
        ('grad_target_joints', C.c_void_p), ('grad_vertex_weights', C.c_void_p), ('grad_joint_weights', C.c_void_p),
        ('grad_shape_betas', C.c_void_p), ('grad_kid_factor', C.c_void_p),
        ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
    ]


class MeshObjectiveArgs(C.Structure):
    """smplfit_mesh_objective_args (include/smplfit.h)."""
    _fields_ = [
        ('pose_rotvecs', C.c_void_p), ('glob_rotmats', C.c_void_p), ('rel_rotmats', C.c_void_p),
        ('shape_betas', C.c_void_p), ('num_betas_given', C.c_int32), ('trans', C.c_void_p),
        ('kid_factor', C.c_void_p), ('batch', C.c_int32), ('target_vertices', C.c_void_p),
        ('vertex_weights', C.c_void_p), ('scale', C.c_float), ('loss', C.c_void_p),
        ('grad_pose_rotvecs', C.c_void_p), ('grad_glob_rotmats', C.c_void_p), ('grad_rel_rotmats', C.c_void_p),
        ('grad_shape_betas', C.c_void_p), ('grad_trans', C.c_void_p), ('grad_kid_factor', C.c_void_p),
        ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
    ]


class FitObjectiveArgs(C.Structure):
    """smplfit_fit_objective_args (include/smplfit.h)."""
    _fields_ = [
        ('pose_rotvecs', C.c_void_p), ('glob_rotmats', C.c_void_p), ('rel_rotmats', C.c_void_p),
        ('shape_betas', C.c_void_p), ('num_betas_given', C.c_int32), ('trans', C.c_void_p),
        ('kid_factor', C.c_void_p), ('batch', C.c_int32), ('target_vertices', C.c_void_p),
        ('vertex_weights', C.c_void_p), ('scale', C.c_float), ('target_joints', C.c_void_p),
        ('joint_weights', C.c_void_p), ('joint_scale', C.c_float), ('loss', C.c_void_p),
        ('grad_pose_rotvecs', C.c_void_p), ('grad_glob_rotmats', C.c_void_p), ('grad_rel_rotmats', C.c_void_p),
        ('grad_shape_betas', C.c_void_p), ('grad_trans', C.c_void_p), ('grad_kid_factor', C.c_void_p),
        ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
    ]


class ConvertArgs(C.Structure):
    """smplfit_convert_args (include/smplfit.h)."""
    _fields_ = [
        ('pose_rotvecs', C.c_void_p), ('shape_betas', C.c_void_p), ('num_betas_given', C.c_int32),
        ('trans', C.c_void_p), ('batch', C.c_int32), ('num_iter', C.c_int32),
        ('beta_regularizer', C.c_float), ('beta_regularizer2', C.c_float), ('kid_regularizer', C.c_float),
        ('final_adjust_rots', C.c_int32), ('out_pose_rotvecs', C.c_void_p), ('out_shape_betas', C.c_void_p),
        ('out_trans', C.c_void_p), ('out_kid_factor', C.c_void_p), ('out_orientations', C.c_void_p),
        ('out_relative_orientations', C.c_void_p), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t),
        ('hip_stream', C.c_void_p),
    ]


class FlipArgs(C.Structure):
    """smplfit_flip_args (include/smplfit.h)."""
    _fields_ = [
        ('pose_rotvecs', C.c_void_p), ('shape_betas', C.c_void_p), ('num_betas_given', C.c_int32),
        ('trans', C.c_void_p), ('kid_factor', C.c_void_p), ('batch', C.c_int32), ('num_iter', C.c_int32),
        ('beta_regularizer', C.c_float), ('beta_regularizer2', C.c_float), ('kid_regularizer', C.c_float),
        ('final_adjust_rots', C.c_int32), ('out_pose_rotvecs', C.c_void_p), ('out_shape_betas', C.c_void_p),
        ('out_trans', C.c_void_p), ('out_kid_factor', C.c_void_p), ('out_orientations', C.c_void_p),
        ('out_relative_orientations', C.c_void_p), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t),
        ('hip_stream', C.c_void_p),
    ]


class ReplaceHandsArgs(C.Structure):
    """smplfit_replace_hands_args (include/smplfit.h)."""
    _fields_ = [
        ('vertices', C.c_void_p), ('batch', C.c_int32), ('num_iter', C.c_int32), ('beta_regularizer', C.c_float),
        ('beta_regularizer2', C.c_float), ('final_adjust_rots', C.c_int32), ('out_vertices', C.c_void_p),
        ('out_pose_rotvecs', C.c_void_p), ('out_shape_betas', C.c_void_p), ('out_trans', C.c_void_p),
        ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('hip_stream', C.c_void_p),
    ]


class ModelDesc(C.Structure):
    _fields_ = [
        ('num_vertices', C.c_int32),
        ('num_joints', C.c_int32),
        ('num_betas', C.c_int32),
        ('is_smpl_family', C.c_int32),
        ('v_template', _fp),
        ('shapedirs', _fp),
        ('posedirs', _fp),
        ('weights', _fp),
        ('J_template', _fp),
        ('J_shapedirs', _fp),
        ('parents', _ip),
        ('J_regressor_post_lbs', _fp),
        ('regressor_num_vertices', C.c_int32),
        ('enable_kid', C.c_int32),
        ('kid_shapedir', _fp),
        ('kid_J_shapedir', _fp),
    ]


class Info(C.Structure):
    _fields_ = [
        (n, C.c_int32)
        for n in (
            'num_vertices', 'num_joints', 'num_betas', 'has_kid', 'padded_vertices', 'num_used_vertices',
            'skin_width', 'num_segments', 'num_fk_levels', 'adj_last_level', 'has_device', 'gemm_vgprs',
            'vertex_path', 'share_fallback',
        )
    ]  # fmt: skip


class SmplfitError(RuntimeError):
    pass


_lib = None


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not osp.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} is missing: build it with `python -m smplfitter_amd.build` '
            '(hipcc, gfx950).  smplfitter_amd has no CPU fallback.'
        )
    # PyTorch is the container for device memory and streams, so the kernels must run on the SAME
    # HIP runtime instance torch uses: torch bundles a libamdhip64.so.7 with the same SONAME as the
    # system one, and whichever is loaded first serves both.  Import torch first.
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    vp, sz, i32, f32 = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    lib.smplfit_create.argtypes = [C.POINTER(ModelDesc), i32, C.POINTER(vp)]
    lib.smplfit_create.restype = i32
    lib.smplfit_destroy.argtypes = [vp]
    lib.smplfit_destroy.restype = None
    lib.smplfit_last_error.restype = C.c_char_p
    lib.smplfit_version.restype = C.c_char_p
    lib.smplfit_get_info.argtypes = [vp, C.POINTER(Info)]
    lib.smplfit_get_info.restype = i32
    lib.smplfit_get_table.argtypes = [vp, i32, _ip, sz, C.POINTER(sz)]
    lib.smplfit_get_table.restype = i32
    lib.smplfit_workspace_bytes.argtypes = [vp, i32]
    lib.smplfit_workspace_bytes.restype = sz
    lib.smplfit_fit_f32.argtypes = [vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.smplfit_fit_f32.restype = i32
    lib.smplfit_fit_warm_f32.argtypes = [vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.smplfit_fit_warm_f32.restype = i32
    lib.smplfit_fit_ex_f32.argtypes = [vp, C.POINTER(FitArgs)]
    lib.smplfit_fit_ex_f32.restype = i32
    lib.smplfit_forward_f32.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, sz, vp]
    lib.smplfit_forward_f32.restype = i32
    lib.smplfit_part_rotations_f32.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, sz, vp]
    lib.smplfit_part_rotations_f32.restype = i32
    lib.smplfit_shape_solve_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, f32, f32, f32, i32, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.smplfit_shape_solve_f32.restype = i32
    lib.smplfit_shape_solve_ex_f32.argtypes = [vp, C.POINTER(ShapeSolveArgs)]
    lib.smplfit_shape_solve_ex_f32.restype = i32
    lib.smplfit_fit_known_shape_f32.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.smplfit_fit_known_shape_f32.restype = i32
    lib.smplfit_time_kernel_f32.argtypes = [vp, i32, i32, i32, vp, sz, vp, C.POINTER(C.c_float)]
    lib.smplfit_time_kernel_f32.restype = i32
    lib.smplfit_primitives_f32.argtypes = [i32, vp, vp, vp, i32, vp]
    lib.smplfit_primitives_f32.restype = i32
    lib.smplfit_forward_ex_f32.argtypes = [vp, C.POINTER(ForwardArgs)]
    lib.smplfit_forward_ex_f32.restype = i32
    lib.smplfit_forward_backward_workspace_bytes.argtypes = [vp, i32]
    lib.smplfit_forward_backward_workspace_bytes.restype = sz
    lib.smplfit_forward_backward_f32.argtypes = [vp, C.POINTER(ForwardBackwardArgs)]
    lib.smplfit_forward_backward_f32.restype = i32
    lib.smplfit_rototranslate_f32.argtypes = [vp, C.POINTER(RototranslateArgs)]
    lib.smplfit_rototranslate_f32.restype = i32
    lib.smplfit_rototranslate_backward_f32.argtypes = [vp, C.POINTER(RototranslateBackwardArgs)]
    lib.smplfit_rototranslate_backward_f32.restype = i32
    lib.smplfit_mesh_objective_workspace_bytes.argtypes = [vp, i32]
    lib.smplfit_mesh_objective_workspace_bytes.restype = sz
    lib.smplfit_mesh_objective_f32.argtypes = [vp, C.POINTER(MeshObjectiveArgs)]
    lib.smplfit_mesh_objective_f32.restype = i32
    lib.smplfit_fit_objective_workspace_bytes.argtypes = [vp, i32]
    lib.smplfit_fit_objective_workspace_bytes.restype = sz
    lib.smplfit_fit_objective_f32.argtypes = [vp, C.POINTER(FitObjectiveArgs)]
    lib.smplfit_fit_objective_f32.restype = i32
    lib.smplfit_transfer_create.argtypes = [i32, i32, _ip, _ip, _fp, i32, C.POINTER(vp)]
    lib.smplfit_transfer_create.restype = i32
    lib.smplfit_transfer_destroy.argtypes = [vp]
    lib.smplfit_transfer_destroy.restype = None
    lib.smplfit_transfer_f32.argtypes = [vp, vp, i32, vp, vp]
    lib.smplfit_transfer_f32.restype = i32
    lib.smplfit_transfer_backward_f32.argtypes = [vp, vp, i32, vp, vp]
    lib.smplfit_transfer_backward_f32.restype = i32
    lib.smplfit_convert_plan_create.argtypes = [vp, vp, vp, C.POINTER(vp)]
    lib.smplfit_convert_plan_create.restype = i32
    lib.smplfit_convert_plan_destroy.argtypes = [vp]
    lib.smplfit_convert_plan_destroy.restype = None
    lib.smplfit_convert_workspace_bytes.argtypes = [vp, i32]
    lib.smplfit_convert_workspace_bytes.restype = sz
    lib.smplfit_convert_f32.argtypes = [vp, C.POINTER(ConvertArgs)]
    lib.smplfit_convert_f32.restype = i32
    lib.smplfit_flip_plan_create.argtypes = [vp, vp, _ip, C.POINTER(vp)]
    lib.smplfit_flip_plan_create.restype = i32
    lib.smplfit_flip_plan_destroy.argtypes = [vp]
    lib.smplfit_flip_plan_destroy.restype = None
    lib.smplfit_flip_workspace_bytes.argtypes = [vp, i32]
    lib.smplfit_flip_workspace_bytes.restype = sz
    lib.smplfit_flip_f32.argtypes = [vp, C.POINTER(FlipArgs)]
    lib.smplfit_flip_f32.restype = i32
    lib.smplfit_replace_hands_plan_create.argtypes = [vp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32,
                                                      C.POINTER(vp)]
    lib.smplfit_replace_hands_plan_create.restype = i32
    lib.smplfit_replace_hands_plan_destroy.argtypes = [vp]
    lib.smplfit_replace_hands_plan_destroy.restype = None
    lib.smplfit_replace_hands_workspace_bytes.argtypes = [vp, i32]
    lib.smplfit_replace_hands_workspace_bytes.restype = sz
    lib.smplfit_replace_hands_f32.argtypes = [vp, C.POINTER(ReplaceHandsArgs)]
    lib.smplfit_replace_hands_f32.restype = i32
    lib.smplfit_shape_solve_backward_workspace_bytes.argtypes = [vp, i32]
    lib.smplfit_shape_solve_backward_workspace_bytes.restype = sz
    lib.smplfit_shape_solve_backward_f32.argtypes = [vp, C.POINTER(ShapeSolveBackwardArgs)]
    lib.smplfit_shape_solve_backward_f32.restype = i32
    lib.smplfit_fit_backward_workspace_bytes.argtypes = [vp, i32, i32]
    lib.smplfit_fit_backward_workspace_bytes.restype = sz
    lib.smplfit_fit_backward_f32.argtypes = [vp, C.POINTER(FitBackwardArgs)]
    lib.smplfit_fit_backward_f32.restype = i32
    lib.smplfit_fit_known_shape_backward_workspace_bytes.argtypes = [vp, i32, i32]
    lib.smplfit_fit_known_shape_backward_workspace_bytes.restype = sz
    lib.smplfit_fit_known_shape_backward_f32.argtypes = [vp, C.POINTER(FitKnownShapeBackwardArgs)]
    lib.smplfit_fit_known_shape_backward_f32.restype = i32
    lib.smplfit_reload_options.argtypes = []
    lib.smplfit_reload_options.restype = i32
    if hasattr(lib, 'smplfit_share_segments_create'):  # (an older build loaded through SMPLFIT_LIB has none of them)
        lib.smplfit_share_segments_create.argtypes = [_ip, i32, i32, C.POINTER(vp)]
        lib.smplfit_share_segments_create.restype = i32
        lib.smplfit_share_segments_destroy.argtypes = [vp]
        lib.smplfit_share_segments_destroy.restype = None
        lib.smplfit_share_segments_batch.argtypes = [vp]
        lib.smplfit_share_segments_batch.restype = i32
        lib.smplfit_share_segments_get_table.argtypes = [vp, i32, _ip, sz, C.POINTER(sz)]
        lib.smplfit_share_segments_get_table.restype = i32
        lib.smplfit_share_segments_workspace_bytes.argtypes = [vp, i32, vp]
        lib.smplfit_share_segments_workspace_bytes.restype = sz
        lib.smplfit_fit_segments_f32.argtypes = [vp, C.POINTER(FitArgs), vp]
        lib.smplfit_fit_segments_f32.restype = i32
        lib.smplfit_shape_solve_segments_f32.argtypes = [vp, C.POINTER(ShapeSolveArgs), vp]
        lib.smplfit_shape_solve_segments_f32.restype = i32
    if hasattr(lib, 'smplfit_gemm_plane_launches'):  # (as above)
        lib.smplfit_gemm_plane_launches.argtypes = []
        lib.smplfit_gemm_plane_launches.restype = C.c_uint64
    if hasattr(lib, 'smplfit_stage_launches'):  # (as above)
        lib.smplfit_stage_launches.argtypes = [i32]
        lib.smplfit_stage_launches.restype = C.c_uint64
    if hasattr(lib, 'smplfit_rotation_spread_launches'):  # (as above)
        lib.smplfit_rotation_spread_launches.argtypes = []
        lib.smplfit_rotation_spread_launches.restype = C.c_uint64
    if hasattr(lib, 'smplfit_mesh_error_f32'):  # (as above)
        lib.smplfit_mesh_error_workspace_bytes.argtypes = [vp, i32]
        lib.smplfit_mesh_error_workspace_bytes.restype = sz
        lib.smplfit_mesh_error_f32.argtypes = [vp, C.POINTER(MeshErrorArgs)]
        lib.smplfit_mesh_error_f32.restype = i32
        lib.smplfit_fit_recon_workspace_bytes.argtypes = [vp, i32, vp]
        lib.smplfit_fit_recon_workspace_bytes.restype = sz
        lib.smplfit_fit_recon_f32.argtypes = [vp, C.POINTER(FitArgs), vp, C.POINTER(FitReconArgs)]
        lib.smplfit_fit_recon_f32.restype = i32
    if hasattr(lib, 'smplfit_fit_robust_f32'):  # (as above)
        lib.smplfit_robust_weights_f32.argtypes = [C.POINTER(RobustWeightsArgs)]
        lib.smplfit_robust_weights_f32.restype = i32
        lib.smplfit_fit_robust_workspace_bytes.argtypes = [vp, i32, vp]
        lib.smplfit_fit_robust_workspace_bytes.restype = sz
        lib.smplfit_fit_robust_f32.argtypes = [vp, C.POINTER(FitArgs), vp, C.POINTER(FitReconArgs), C.POINTER(FitRobustArgs)]
        lib.smplfit_fit_robust_f32.restype = i32
    if hasattr(lib, 'smplfit_mesh_error_aligned_f32'):  # (as above)
        lib.smplfit_mesh_error_aligned_workspace_bytes.argtypes = [vp, i32]
        lib.smplfit_mesh_error_aligned_workspace_bytes.restype = sz
        lib.smplfit_mesh_error_aligned_f32.argtypes = [vp, C.POINTER(MeshErrorArgs), C.POINTER(MeshAlignArgs)]
        lib.smplfit_mesh_error_aligned_f32.restype = i32
        lib.smplfit_align_points_workspace_bytes.argtypes = [i32, i32]
        lib.smplfit_align_points_workspace_bytes.restype = sz
        lib.smplfit_align_points_f32.argtypes = [C.POINTER(AlignPointsArgs)]
        lib.smplfit_align_points_f32.restype = i32
    if os.environ.get('SMPLFIT_LIB') and not hasattr(lib, 'smplfit_abi_version'):
        _lib = lib  # an older build loaded by the A/B tools (tools/ab_fit.py): no version / share-table exports
        return lib
    lib.smplfit_abi_version.argtypes = []
    lib.smplfit_abi_version.restype = i32
    if lib.smplfit_abi_version() != SMPLFIT_ABI_VERSION:
        raise ImportError(f'{LIB_PATH} was built for ABI {lib.smplfit_abi_version()}, this package expects '
                          f'{SMPLFIT_ABI_VERSION}: rebuild it (python -m smplfitter_amd.build --force)')
    lib.smplfit_get_share_table.argtypes = [vp, i32, i32, _ip, sz, C.POINTER(sz)]
    lib.smplfit_get_share_table.restype = i32
    lib.smplfit_pick_share_mult.argtypes = [vp, i32, i32]
    lib.smplfit_pick_share_mult.restype = i32
    _lib = lib
    return lib


def check(status: int):
    """Map a C-ABI status to the exception types the reference raises for the same condition."""
    if status == SMPLFIT_OK:
        return
    msg = load().smplfit_last_error().decode()
    if status == SMPLFIT_ERR_BAD_ARG:
        raise ValueError(msg)
    if status == SMPLFIT_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise SmplfitError(f'smplfit status {status}: {msg}')


def make_desc(v_template, shapedirs, posedirs, weights, J_template, J_shapedirs, parents,
              J_regressor_post_lbs=None, is_smpl_family=True, kid_shapedir=None, kid_J_shapedir=None):
    """Build a ``ModelDesc`` from numpy arrays; returns (desc, keepalive list)."""
    f32c = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.float32)  # noqa: E731
    arrs = dict(
        v_template=f32c(v_template), shapedirs=f32c(shapedirs), posedirs=f32c(posedirs),
        weights=f32c(weights), J_template=f32c(J_template), J_shapedirs=f32c(J_shapedirs),
    )
    par = np.ascontiguousarray(np.asarray(parents), dtype=np.int32)
    V, J = arrs['weights'].shape
    S = arrs['shapedirs'].shape[2]
    assert arrs['v_template'].shape == (V, 3)
    assert arrs['shapedirs'].shape == (V, 3, S)
    assert arrs['posedirs'].shape == (V, 3, 9 * (J - 1))
    assert arrs['J_template'].shape == (J, 3) and arrs['J_shapedirs'].shape == (J, 3, S)
    d = ModelDesc()
    d.num_vertices, d.num_joints, d.num_betas = V, J, S
    d.is_smpl_family = 1 if is_smpl_family else 0
    for k, a in arrs.items():
        setattr(d, k, a.ctypes.data_as(_fp))
    d.parents = par.ctypes.data_as(_ip)
    keep = list(arrs.values()) + [par]
    if J_regressor_post_lbs is not None:
        reg = f32c(J_regressor_post_lbs)
        d.J_regressor_post_lbs = reg.ctypes.data_as(_fp)
        d.regressor_num_vertices = reg.shape[1]
        keep.append(reg)
    else:
        d.J_regressor_post_lbs = None
        d.regressor_num_vertices = 0
    if kid_shapedir is not None:
        ks, kj = f32c(kid_shapedir), f32c(kid_J_shapedir)
        assert ks.shape == (V, 3) and kj.shape == (J, 3)
        d.enable_kid = 1
        d.kid_shapedir = ks.ctypes.data_as(_fp)
        d.kid_J_shapedir = kj.ctypes.data_as(_fp)
        keep += [ks, kj]
    else:
        d.enable_kid = 0
        d.kid_shapedir = None
        d.kid_J_shapedir = None
    return d, keep


class Handle:
    """Owns a ``smplfit_handle*``."""

    def __init__(self, desc: ModelDesc, host_only: bool = False):
        lib = load()
        self._h = C.c_void_p()
        check(lib.smplfit_create(C.byref(desc), SMPLFIT_CREATE_HOST_ONLY if host_only else 0, C.byref(self._h)))
        self.info = Info()
        check(lib.smplfit_get_info(self._h, C.byref(self.info)))

    @property
    def ptr(self):
        return self._h

    def table(self, name: str) -> np.ndarray:
        lib = load()
        n = C.c_size_t()
        check(lib.smplfit_get_table(self._h, TABLE_IDS[name], None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        check(lib.smplfit_get_table(self._h, TABLE_IDS[name], out.ctypes.data_as(_ip), n.value, C.byref(n)))
        return out

    def share_table(self, kind: int, what: int) -> np.ndarray:
        """Cell tables of the batch-major vertex kernels (``smplfit_get_share_table``)."""
        lib = load()
        n = C.c_size_t()
        check(lib.smplfit_get_share_table(self._h, kind, what, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        check(lib.smplfit_get_share_table(self._h, kind, what, out.ctypes.data_as(_ip), n.value, C.byref(n)))
        return out

    def workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_workspace_bytes(self._h, int(batch)))

    def mesh_error_workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_mesh_error_workspace_bytes(self._h, int(batch)))

    def mesh_error_aligned_workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_mesh_error_aligned_workspace_bytes(self._h, int(batch)))

    def fit_recon_workspace_bytes(self, batch: int, plan: 'ShareSegments | None' = None) -> int:
        return int(load().smplfit_fit_recon_workspace_bytes(self._h, int(batch), plan.ptr if plan is not None else None))

    def fit_robust_workspace_bytes(self, batch: int, plan: 'ShareSegments | None' = None) -> int:
        return int(load().smplfit_fit_robust_workspace_bytes(self._h, int(batch), plan.ptr if plan is not None else None))

    def forward_backward_workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_forward_backward_workspace_bytes(self._h, int(batch)))

    def mesh_objective_workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_mesh_objective_workspace_bytes(self._h, int(batch)))

    def fit_objective_workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_fit_objective_workspace_bytes(self._h, int(batch)))

    def shape_solve_backward_workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_shape_solve_backward_workspace_bytes(self._h, int(batch)))

    def fit_backward_workspace_bytes(self, batch: int, num_iter: int) -> int:
        return int(load().smplfit_fit_backward_workspace_bytes(self._h, int(batch), int(num_iter)))

    def fit_known_shape_backward_workspace_bytes(self, batch: int, num_iter: int) -> int:
        return int(load().smplfit_fit_known_shape_backward_workspace_bytes(self._h, int(batch), int(num_iter)))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            load().smplfit_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reload_options():
    """Re-read the SMPLFIT_* tuning variables (they are read once, at first use): for tests and A/B tools that
    switch kernel paths inside one process."""
    check(load().smplfit_reload_options())


def gemm_plane_launches() -> int:
    """Posedirs GEMM launches of this process that read the prologue kernel's split-bf16 feature planes
    (``SMPLFIT_GEMM_PLANES=0``: none); the results do not show which front end ran, this count does."""
    return int(load().smplfit_gemm_plane_launches())


def rotation_spread_launches() -> int:
    """Part-rotation launches of this process that ran as ``k_rotations_spread``, a joint per wave
    (calls of up to 4096 instances; ``SMPLFIT_ROT_SPREAD=0``: none); both forms give the same bits and the same stage counts, this count tells them apart."""
    return int(load().smplfit_rotation_spread_launches())


def stage_launches() -> dict:
    """Launches of each stage kernel by this process (``STAGE_IDS``): process-wide host counters meant for tests and
    A/B tools, which take the difference around a synchronised call to see the route it took."""
    lib = load()
    return {k: int(lib.smplfit_stage_launches(v)) for k, v in STAGE_IDS.items()}


class Transfer:
    """Owns a ``smplfit_transfer*``: the (V_out x V_in) CSR topology-transfer matrix on the current device
    (``negate_x``: followed by x -> -x, the mirror of ``BodyFlipper``)."""

    def __init__(self, num_vertices_in: int, num_vertices_out: int, indptr, indices, values, host_only: bool = False,
                 negate_x: bool = False):
        lib = load()
        ip = np.ascontiguousarray(indptr, dtype=np.int32)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        va = np.ascontiguousarray(values, dtype=np.float32)
        if ip.shape != (num_vertices_out + 1,) or ix.shape != va.shape or ix.ndim != 1 or int(ip[-1]) != ix.shape[0]:
            raise ValueError('Transfer: indptr / indices / values do not describe a (V_out x V_in) CSR matrix')
        self.shape = (int(num_vertices_out), int(num_vertices_in))
        self._t = C.c_void_p()
        check(lib.smplfit_transfer_create(
            int(num_vertices_in), int(num_vertices_out), ip.ctypes.data_as(_ip), ix.ctypes.data_as(_ip),
            va.ctypes.data_as(_fp),
            (SMPLFIT_CREATE_HOST_ONLY if host_only else 0) | (SMPLFIT_TRANSFER_NEGATE_X if negate_x else 0),
            C.byref(self._t)))

    @property
    def ptr(self):
        return self._t

    def forward(self, in_vertices: int, batch: int, out_vertices: int, stream: 'int | None' = None):
        """``smplfit_transfer_f32`` on device addresses: (batch, V_in, 3) -> (batch, V_out, 3)."""
        vp = C.c_void_p
        check(load().smplfit_transfer_f32(self._t, vp(in_vertices), int(batch), vp(out_vertices), vp(stream)))

    def backward(self, grad_out_vertices: int, batch: int, grad_in_vertices: int, stream: 'int | None' = None):
        """``smplfit_transfer_backward_f32`` on device addresses: (batch, V_out, 3) -> (batch, V_in, 3)."""
        vp = C.c_void_p
        check(load().smplfit_transfer_backward_f32(self._t, vp(grad_out_vertices), int(batch), vp(grad_in_vertices),
                                                   vp(stream)))

    def close(self):
        if getattr(self, '_t', None) is not None and self._t.value:
            load().smplfit_transfer_destroy(self._t)
            self._t = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShareSegments:
    """Owns a ``smplfit_share_segments*``: the tables of a ``share_beta`` batch cut into consecutive runs of rows
    (``sizes``), on the current device unless ``host_only``.  Raises ``ValueError`` for sizes the library refuses."""

    TABLES = dict(row_seg=0, seg_blk=1, blk_rows=2)

    def __init__(self, sizes, host_only: bool = False):
        sz = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1)
        self._p = C.c_void_p()
        check(load().smplfit_share_segments_create(sz.ctypes.data_as(_ip), sz.shape[0],
                                                   SMPLFIT_CREATE_HOST_ONLY if host_only else 0, C.byref(self._p)))

    @property
    def ptr(self):
        return self._p

    @property
    def batch(self) -> int:
        return int(load().smplfit_share_segments_batch(self._p))

    def table(self, name: str) -> np.ndarray:
        lib = load()
        n = C.c_size_t()
        check(lib.smplfit_share_segments_get_table(self._p, self.TABLES[name], None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        check(lib.smplfit_share_segments_get_table(self._p, self.TABLES[name], out.ctypes.data_as(_ip), n.value, C.byref(n)))
        return out

    def workspace_bytes(self, h: 'Handle') -> int:
        return int(load().smplfit_share_segments_workspace_bytes(h.ptr, self.batch, self._p))

    def close(self):
        if getattr(self, '_p', None) is not None and self._p.value:
            load().smplfit_share_segments_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ConvertPlan:
    """Owns a ``smplfit_convert_plan*`` and keeps the two handles (and the matrix) it borrows alive.  Raises
    ``NotImplementedError`` when the fused conversion does not apply to the two models."""

    def __init__(self, h_in: Handle, h_out: Handle, transfer: 'Transfer | None'):
        self._keep = (h_in, h_out, transfer)
        self._p = C.c_void_p()
        check(load().smplfit_convert_plan_create(h_in.ptr, h_out.ptr, transfer.ptr if transfer is not None else None,
                                                 C.byref(self._p)))

    @property
    def ptr(self):
        return self._p

    def workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_convert_workspace_bytes(self._p, int(batch)))

    def close(self):
        if getattr(self, '_p', None) is not None and self._p.value:
            load().smplfit_convert_plan_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FlipPlan:
    """Owns a ``smplfit_flip_plan*`` and keeps the kid handle and the mirror matrix it borrows alive.  Raises
    ``NotImplementedError`` when the fused flip does not apply to the model."""

    def __init__(self, h: Handle, mirror: Transfer, joint_perm):
        perm = np.ascontiguousarray(joint_perm, dtype=np.int32)
        self._keep = (h, mirror)
        self._p = C.c_void_p()
        check(load().smplfit_flip_plan_create(h.ptr, mirror.ptr, perm.ctypes.data_as(_ip), C.byref(self._p)))

    @property
    def ptr(self):
        return self._p

    def workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_flip_workspace_bytes(self._p, int(batch)))

    def close(self):
        if getattr(self, '_p', None) is not None and self._p.value:
            load().smplfit_flip_plan_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReplaceHandsPlan:
    """Owns a ``smplfit_replace_hands_plan*`` and keeps the handle it borrows alive: the (V) fit weights, the (V) mix
    weights and the rotation vectors written over the joints ``[first_joint, first_joint + num_joints)``.  Raises
    ``ValueError`` for vectors of the wrong length or a joint range outside the model, ``NotImplementedError`` when the
    fused call does not apply to the model."""

    def __init__(self, h: Handle, fit_weights, mix_weights, first_joint: int, num_joints: int, rotvecs):
        fw = np.ascontiguousarray(fit_weights, dtype=np.float32).reshape(-1)
        mw = np.ascontiguousarray(mix_weights, dtype=np.float32).reshape(-1)
        rv = np.ascontiguousarray(rotvecs, dtype=np.float32).reshape(-1)
        if fw.shape != mw.shape:
            raise ValueError('ReplaceHandsPlan: fit_weights and mix_weights must have one length')
        self._keep = (h,)
        self._p = C.c_void_p()
        check(load().smplfit_replace_hands_plan_create(
            h.ptr, fw.ctypes.data_as(_fp), mw.ctypes.data_as(_fp), fw.shape[0], int(first_joint), int(num_joints),
            rv.ctypes.data_as(_fp), rv.shape[0], C.byref(self._p)))

    @property
    def ptr(self):
        return self._p

    def workspace_bytes(self, batch: int) -> int:
        return int(load().smplfit_replace_hands_workspace_bytes(self._p, int(batch)))

    def close(self):
        if getattr(self, '_p', None) is not None and self._p.value:
            load().smplfit_replace_hands_plan_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
