// TEST-ONLY host build of the per-instance bodies of BodyModel.rototranslate and of its backward
// (sf::rototranslate_instance, sf::rototranslate_instance_backward in csrc/sf_rigid.h: the functions the kernels of
// kernels_rigid.inc call, one lane per instance), compiled with g++ by tests/rototranslate_util.py.  j_ext: (3, S + 1)
// [J_template[0] | J_shapedirs[0] (| kid_J_shapedir[0] last when has_kid)], rows of joint 0 as in JointTabs::j_ext.
#include <cstddef>

#include "../../smplfitter_amd/csrc/sf_rigid.h"

extern "C" {

// pointers as in the C-ABI struct (NULL = absent); R_stride 9 | 0, t_stride 3 | 0
int hostemu_rototranslate(const float* j_ext, int S, int J3, int B, const float* R, int R_stride, const float* t,
                          int t_stride, const float* pose, const float* betas, int nb, const float* kid,
                          const float* trans, int post, float* new_pose, float* new_trans) {
  for (int b = 0; b < B; ++b) {
    float root[3], tr[3];
    sf::rototranslate_instance(j_ext, S, R + (size_t)b * R_stride, t ? t + (size_t)b * t_stride : nullptr,
                               pose + (size_t)b * J3, betas ? betas + (size_t)b * nb : nullptr, betas ? nb : 0,
                               kid ? kid + b : nullptr, trans + (size_t)b * 3, post != 0, root, tr);
    for (int k = 0; k < J3; ++k) new_pose[(size_t)b * J3 + k] = k < 3 ? root[k] : pose[(size_t)b * J3 + k];
    for (int c = 0; c < 3; ++c) new_trans[(size_t)b * 3 + c] = tr[c];
  }
  return 0;
}

int hostemu_rototranslate_backward(const float* j_ext, int S, int J3, int B, const float* R, int R_stride,
                                   const float* t, int t_stride, const float* pose, const float* betas, int nb,
                                   const float* kid, const float* trans, int post, const float* g_pose,
                                   const float* g_trans, float* gR, float* gt, float* gpose, float* gbetas,
                                   float* gtrans, float* gkid) {
  for (int b = 0; b < B; ++b) {
    float groot[3];
    sf::rototranslate_instance_backward(
        j_ext, S, R + (size_t)b * R_stride, t ? t + (size_t)b * t_stride : nullptr, pose + (size_t)b * J3,
        betas ? betas + (size_t)b * nb : nullptr, betas ? nb : 0, kid ? kid + b : nullptr, trans + (size_t)b * 3,
        post != 0, g_pose ? g_pose + (size_t)b * J3 : nullptr, g_trans ? g_trans + (size_t)b * 3 : nullptr,
        gR ? gR + (size_t)b * 9 : nullptr, gt ? gt + (size_t)b * 3 : nullptr, groot,
        gbetas ? gbetas + (size_t)b * nb : nullptr, gtrans ? gtrans + (size_t)b * 3 : nullptr, gkid ? gkid + b : nullptr);
    if (gpose)
      for (int k = 0; k < J3; ++k)
        gpose[(size_t)b * J3 + k] = k < 3 ? groot[k] : (g_pose ? g_pose[(size_t)b * J3 + k] : 0.f);
  }
  return 0;
}

}  // extern "C"
