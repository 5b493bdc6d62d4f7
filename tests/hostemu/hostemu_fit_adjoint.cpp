// TEST-ONLY host build of the per-instance and per-vertex arithmetic of smplfit_fit_backward_f32 (sf::proj_so3_adjoint,
// sf::fit_rot_adjoint, sf::fit_tail_adjoint, sf::partsum_vertex_adjoint, sf::centring_correction in csrc/sf_math.h and
// csrc/sf_stages.h), compiled with g++ by tests/test_fit_grad_host.py.  The sequences are those of kernels_adj.inc with
// one lane; the tables are the product's (sf::build_tables).  Vertex arrays are in the caller's vertex order.
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/smplfit.h"
#include "../../smplfitter_amd/csrc/sf_tables.h"
#include "../../smplfitter_amd/csrc/sf_stages.h"

namespace {
std::string g_err;

struct Tabs {
  sf::HostTables t;
  sf::JointTabs jt;
  bool ok;
  explicit Tabs(const smplfit_model_desc* d) {
    bool unsup = false;
    g_err = sf::build_tables(*d, t, &unsup);
    ok = g_err.empty();
    if (ok) jt = sf::bind_joint_tabs(t, [](const auto& v) { return v.data(); });
  }
};

// the part sums of one instance (J, kPsum), slots in sorted order as the kernel walks them; ref_stride 0: a shared mesh
void part_sums(const sf::HostTables& t, const float* tv, const float* rv, const float* vw, double* psum) {
  for (int k = 0; k < t.J * sf::kPsum; ++k) psum[k] = 0.0;
  for (int i = 0; i < t.n_used; ++i) {
    const int o = t.perm[i], p = t.slot_part[i];
    if (o < 0 || p < 0) continue;
    sf::partsum_vertex_d(tv + (size_t)o * 3, rv + (size_t)o * 3, vw ? vw[o] : 1.f, psum + p * sf::kPsum);
  }
}

// the vertex pass of the adjoint: g_tv += tbar, g_rv = abar, g_vw += wbar
void part_sums_adjoint(const sf::HostTables& t, const float* tv, const float* rv, const float* vw, const float* pbar,
                       float* g_tv, float* g_rv, float* g_vw) {
  for (int i = 0; i < t.n_used; ++i) {
    const int o = t.perm[i], p = t.slot_part[i];
    if (o < 0 || p < 0) continue;
    float tb[3], ab[3];
    const float wb = sf::partsum_vertex_adjoint(tv + (size_t)o * 3, rv + (size_t)o * 3, vw ? vw[o] : 1.f, vw != nullptr,
                                                pbar + p * sf::kPsum, tb, ab);
    for (int c = 0; c < 3; ++c) {
      g_tv[(size_t)o * 3 + c] += tb[c];
      if (g_rv) g_rv[(size_t)o * 3 + c] += ab[c];
    }
    if (vw && g_vw) g_vw[o] += wb;
  }
}
}  // namespace

extern "C" {

const char* hostemu_fa_last_error() { return g_err.c_str(); }

// n projections: R = proj_so3(A), Abar = adjoint(A, R, Rbar)
void hostemu_fa_proj(const float* A, const double* Rbar, float* R, double* Abar, int n) {
  for (int i = 0; i < n; ++i) {
    sf::proj_so3(A + i * 9, R + i * 9);
    double a[9], r[9];
    for (int k = 0; k < 9; ++k) a[k] = A[i * 9 + k], r[k] = R[i * 9 + k];
    sf::proj_so3_adjoint(a, r, Rbar + i * 9, Abar + i * 9);
  }
}

// One rotation pass and its adjoint.  rv (B or 1, V, 3) / rj (B or 1, J, 3): shared when ref_shared.  Gprev may be null.
// Outputs (zeroed here): Gout (B,J,9), g_tv, g_rv (B,V,3), g_vw (B,V), g_tj, g_rj (B,J,3), g_jw (B,J), g_Gprev (B,J,9).
int hostemu_fa_rot(const smplfit_model_desc* d, int B, const float* tv, const float* tj, const float* rv, const float* rj,
                   int ref_shared, const float* vw, const float* jw, const float* Gprev, const float* Gbar, float* Gout,
                   float* g_tv, float* g_rv, float* g_vw, float* g_tj, float* g_rj, float* g_jw, float* g_Gprev) {
  Tabs T(d);
  if (!T.ok) return -1;
  const sf::HostTables& t = T.t;
  const int J = t.J, V = t.V;
  std::vector<double> psum(J * sf::kPsum);
  std::vector<float> pbar(J * sf::kPsum);
  std::vector<double> scr(sf::fit_rot_adjoint_scratch(J));
  for (int b = 0; b < B; ++b) {
    const float* tvb = tv + (size_t)b * V * 3;
    const float* rvb = rv + (ref_shared ? 0 : (size_t)b * V * 3);
    const float* tjb = tj + (size_t)b * J * 3;
    const float* rjb = rj + (ref_shared ? 0 : (size_t)b * J * 3);
    const float* vwb = vw ? vw + (size_t)b * V : nullptr;
    const float* jwb = jw ? jw + (size_t)b * J : nullptr;
    const float* gp = Gprev ? Gprev + (size_t)b * J * 9 : nullptr;
    part_sums(t, tvb, rvb, vwb, psum.data());
    sf::fit_rot_forward(T.jt, psum.data(), tjb, rjb, jwb, gp, Gout + (size_t)b * J * 9);
    sf::fit_rot_adjoint(T.jt, psum.data(), tjb, rjb, jwb, gp, Gbar + (size_t)b * J * 9, pbar.data(),
                        gp ? g_Gprev + (size_t)b * J * 9 : nullptr, scr.data());
    for (size_t k = 0; k < (size_t)V * 3; ++k) g_tv[(size_t)b * V * 3 + k] = g_rv[(size_t)b * V * 3 + k] = 0.f;
    for (int k = 0; k < V; ++k) g_vw[(size_t)b * V + k] = 0.f;
    part_sums_adjoint(t, tvb, rvb, vwb, pbar.data(), g_tv + (size_t)b * V * 3, g_rv + (size_t)b * V * 3, g_vw + (size_t)b * V);
    for (int k = 0; k < J * 3; ++k) {
      g_tj[(size_t)b * J * 3 + k] = (float)scr[k];
      g_rj[(size_t)b * J * 3 + k] = (float)scr[J * 3 + k];
    }
    for (int k = 0; k < J; ++k) g_jw[(size_t)b * J + k] = (float)scr[J * 6 + k];
  }
  return 0;
}

// Output stage + refinement and their adjoint.  x (B, S): every shape unknown.  g_pose / g_orient / g_rel may be null.
int hostemu_fa_tail(const smplfit_model_desc* d, int B, const float* G, const float* x, const float* trans, const float* tv,
                    const float* tj, const float* rv, const float* rj_term, const float* rj_true, const float* vw,
                    const float* jw, int final_adjust, const float* g_pose, const float* g_orient, const float* g_rel,
                    float* Gbar, float* xbar, float* tbar, float* g_tv, float* g_rv, float* g_vw, float* g_tj,
                    float* g_rjt, float* g_rj, float* g_jw) {
  Tabs T(d);
  if (!T.ok) return -1;
  const sf::HostTables& t = T.t;
  const int J = t.J, V = t.V, S = t.S;
  std::vector<double> psum(J * sf::kPsum);
  std::vector<float> pbar(J * sf::kPsum);
  std::vector<double> scr(sf::fit_tail_adjoint_scratch(J));
  for (int b = 0; b < B; ++b) {
    const float* tvb = tv + (size_t)b * V * 3;
    const float* rvb = rv + (size_t)b * V * 3;
    const float* vwb = vw ? vw + (size_t)b * V : nullptr;
    const float* jwb = jw ? jw + (size_t)b * J : nullptr;
    part_sums(t, tvb, rvb, vwb, psum.data());
    sf::fit_tail_adjoint(T.jt, G + (size_t)b * J * 9, x + (size_t)b * S, trans + (size_t)b * 3, psum.data(),
                         tj + (size_t)b * J * 3, rj_term + (size_t)b * J * 3, rj_true + (size_t)b * J * 3, jwb,
                         final_adjust != 0, g_pose ? g_pose + (size_t)b * J * 3 : nullptr,
                         g_orient ? g_orient + (size_t)b * J * 9 : nullptr, g_rel ? g_rel + (size_t)b * J * 9 : nullptr,
                         scr.data(), Gbar + (size_t)b * J * 9, xbar + (size_t)b * S, tbar + (size_t)b * 3, pbar.data());
    for (size_t k = 0; k < (size_t)V * 3; ++k) g_tv[(size_t)b * V * 3 + k] = g_rv[(size_t)b * V * 3 + k] = 0.f;
    for (int k = 0; k < V; ++k) g_vw[(size_t)b * V + k] = 0.f;
    part_sums_adjoint(t, tvb, rvb, vwb, pbar.data(), g_tv + (size_t)b * V * 3, g_rv + (size_t)b * V * 3, g_vw + (size_t)b * V);
    for (int k = 0; k < J * 3; ++k) {
      g_tj[(size_t)b * J * 3 + k] = (float)scr[sf::fit_tail_tjbar(J) + k];
      g_rjt[(size_t)b * J * 3 + k] = (float)scr[sf::fit_tail_rjtbar(J) + k];
      g_rj[(size_t)b * J * 3 + k] = (float)scr[sf::fit_tail_rjbar(J) + k];
    }
    for (int k = 0; k < J; ++k) g_jw[(size_t)b * J + k] = (float)scr[sf::fit_tail_jwbar(J) + k];
  }
  return 0;
}

// Centring: g (n, 3) cotangents of the centred points of one instance, in place -> those of the points themselves
void hostemu_fa_uncenter(float* g, int n, const float* g_trans) {
  double sum[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) sum[c] += (double)g[i * 3 + c];
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) g[i * 3 + c] += sf::centring_correction(sum[c], g_trans ? g_trans[c] : 0.f, n);
}

}  // extern "C"
