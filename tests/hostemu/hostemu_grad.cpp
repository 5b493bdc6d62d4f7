// TEST-ONLY host build of the per-instance joint backward of smplfit_forward_backward_f32 (sf::forward_joint_backward,
// sf::rotvec2mat_vjp in csrc/sf_stages.h), compiled with g++ by tests/test_forward_grad_host.py.  The kinematic tables
// come straight from the caller (parents, joints in tree order by level, [J_template | J_shapedirs | kid]).
#include <cstdint>
#include <vector>

#include "../../smplfitter_amd/csrc/sf_stages.h"

extern "C" {

void hostemu_rotvec2mat_vjp(const float* r, const float* dR, float* dr, int n) {
  for (int i = 0; i < n; ++i) sf::rotvec2mat_vjp(r + i * 3, dR + i * 9, dr + i * 3);
}

// one instance per call of the loop; pointers as in kernels_bwd.inc's k_bwd_joint (NULL = absent)
int hostemu_joint_backward(int J, int S, int n_kid, const int32_t* parents, const int32_t* fk_js,
                           const int32_t* fk_level_start, int num_levels, const float* j_ext, int B,
                           const float* pose, const float* glob, const float* rel, const float* betas, int nb,
                           const float* kid, const float* dA, const float* gjoints, const float* gorient,
                           const float* dfeat, const float* dshape, float* g_pose, float* g_glob, float* g_rel,
                           float* g_betas, float* g_kid, float* g_trans) {
  sf::JointTabs tb{};
  tb.J = J; tb.S = S; tb.n_kid = n_kid; tb.num_levels = num_levels; tb.P = 9 * (J - 1);
  tb.parents = parents; tb.fk_js = fk_js; tb.fk_level_start = fk_level_start; tb.j_ext = j_ext;
  std::vector<float> scratch(sf::joint_bwd_scratch_floats(J));
  const int P = 9 * (J - 1);
  for (int b = 0; b < B; ++b)
    sf::forward_joint_backward(
        tb, pose ? pose + (size_t)b * J * 3 : nullptr, glob ? glob + (size_t)b * J * 9 : nullptr,
        rel ? rel + (size_t)b * J * 9 : nullptr, betas ? betas + (size_t)b * nb : nullptr, betas ? nb : 0,
        kid ? kid + b : nullptr, dA ? dA + (size_t)b * J * 12 : nullptr, gjoints ? gjoints + (size_t)b * J * 3 : nullptr,
        gorient ? gorient + (size_t)b * J * 9 : nullptr, dfeat ? dfeat + (size_t)b * P : nullptr,
        dshape ? dshape + (size_t)b * S : nullptr, scratch.data(), g_pose ? g_pose + (size_t)b * J * 3 : nullptr,
        g_glob ? g_glob + (size_t)b * J * 9 : nullptr, g_rel ? g_rel + (size_t)b * J * 9 : nullptr,
        g_betas ? g_betas + (size_t)b * nb : nullptr, g_kid ? g_kid + b : nullptr,
        g_trans ? g_trans + (size_t)b * 3 : nullptr);
  return 0;
}

}  // extern "C"
