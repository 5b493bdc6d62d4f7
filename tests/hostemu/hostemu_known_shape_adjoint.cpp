// TEST-ONLY host build of the new arithmetic of smplfit_fit_known_shape_backward_f32 (sf::align_point_d,
// sf::align_translation, sf::align_point_adjoint in csrc/sf_stages.h) and of the composition of one iteration of its
// reverse sweep (output stage and refinement -> alignment -> rotation pass), compiled with g++ by
// tests/test_known_shape_grad_host.py.  The sequences are those of smplfit_fit_known_shape_backward_f32 with one lane;
// the meshes are inputs (the forward and its vector-Jacobian product are the GPU kernels' and are tested there).  The
// tables, the part sums and their adjoint are those of hostemu_fit_adjoint.cpp.
#include "hostemu_fit_adjoint.cpp"

namespace {
// k_fa_regress: joints (J, 3) from the (V, 3) vertices of one instance
void regress(const sf::HostTables& t, const float* src, float* out) {
  for (int j = 0; j < t.J; ++j) {
    float a[3] = {0.f, 0.f, 0.f};
    for (int k = t.reg_start[j]; k < t.reg_start[j + 1]; ++k)
      for (int c = 0; c < 3; ++c) a[c] += t.reg_val[k] * src[(size_t)t.perm[t.reg_slot[k]] * 3 + c];
    for (int c = 0; c < 3; ++c) out[j * 3 + c] = a[c];
  }
}
// the regressor's transpose of k_fa_vertex: g_v += reg^T gj
void regress_T(const sf::HostTables& t, const float* gj, float* g_v) {
  for (int j = 0; j < t.J; ++j)
    for (int k = t.reg_start[j]; k < t.reg_start[j + 1]; ++k)
      for (int c = 0; c < 3; ++c) g_v[(size_t)t.perm[t.reg_slot[k]] * 3 + c] += t.reg_val[k] * gj[j * 3 + c];
}
}  // namespace

extern "C" {

// The alignment of n points and its adjoint: t = sum w (tau - r) / sum w (w null: ones); from tbar: g_tau (= -g_r) and g_w.
void hostemu_ks_align(const float* tau, const float* r, const float* w, int n, const float* tbar, float* t, float* g_tau,
                      float* g_w) {
  double acc[sf::kAlign] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) sf::align_point_d(tau + i * 3, r + i * 3, w ? w[i] : 1.f, acc);
  sf::align_translation(acc, t);
  double q[3];
  for (int c = 0; c < 3; ++c) q[c] = (double)tbar[c] / acc[3];
  for (int i = 0; i < n; ++i) {
    const float m[3] = {r[i * 3] + t[0], r[i * 3 + 1] + t[1], r[i * 3 + 2] + t[2]};
    g_w[i] = sf::align_point_adjoint(tau + i * 3, m, w ? w[i] : 1.f, q, g_tau + i * 3);
  }
}

// One iteration of the known-shape fit and its adjoint.  G = Rot(tv, rv0) Gprev; t = align(targets, rvn, rjn);
// results: log(rel(Refine(targets, rvn + t, rjn + t, G, x, t))) and t, with the cotangents g_pose (B,J,3), g_trans (B,3).
// tj null: both joint sets of the rotation stages are regressed from the vertices.  The alignment weights follow
// solve_weights.  Every output is zeroed here.
int hostemu_ks_iteration(const smplfit_model_desc* d, int B, const float* tv, const float* tj, const float* vw, const float* jw,
                         const float* rv0, const float* rj0, const float* Gprev, const float* rvn, const float* rjn,
                         const float* x, int final_adjust, const float* g_pose, const float* g_trans, float* Gout, float* trans,
                         float* g_tv, float* g_tj, float* g_vw, float* g_jw, float* g_rv0, float* g_rj0, float* g_Gprev,
                         float* g_rvn, float* g_rjn, float* g_x) {
  Tabs T(d);
  if (!T.ok) return -1;
  const sf::HostTables& t = T.t;
  const int J = t.J, V = t.V, S = t.S;
  const bool joints = tj != nullptr, wv = joints ? (vw && jw) : (vw != nullptr), wj = joints && vw && jw;
  std::vector<double> psum(J * sf::kPsum), scr(sf::fit_tail_adjoint_scratch(J));
  std::vector<float> pbar(J * sf::kPsum), ctj(J * 3), rjr(J * 3), mesh((size_t)V * 3), jn(J * 3), rjterm(J * 3), Gbar(J * 9),
      xbar(S), tmp3(J * 3);
  for (int b = 0; b < B; ++b) {
    const size_t ov = (size_t)b * V * 3, oj = (size_t)b * J * 3;
    const float *tvb = tv + ov, *rv0b = rv0 + ov, *rvnb = rvn + ov, *rjnb = rjn + oj;
    const float* vwb = vw ? vw + (size_t)b * V : nullptr;
    const float* jwb = jw ? jw + (size_t)b * J : nullptr;
    const float* gp = Gprev + (size_t)b * J * 9;
    float *gtv = g_tv + ov, *gvw = g_vw + (size_t)b * V, *gtj = g_tj + oj, *gjw = g_jw + (size_t)b * J;
    float *meshbar = g_rvn + ov, *jointsbar = g_rjn + oj, *grv0 = g_rv0 + ov, *grj0 = g_rj0 + oj;
    for (size_t k = 0; k < (size_t)V * 3; ++k) gtv[k] = meshbar[k] = grv0[k] = 0.f;
    for (int k = 0; k < V; ++k) gvw[k] = 0.f;
    for (int k = 0; k < J * 3; ++k) gtj[k] = jointsbar[k] = grj0[k] = 0.f;
    for (int k = 0; k < J; ++k) gjw[k] = 0.f;
    // ---- forward: the rotation pass, the alignment
    if (joints) {
      for (int k = 0; k < J * 3; ++k) ctj[k] = tj[oj + k], rjr[k] = rj0[oj + k];
    } else {
      regress(t, tvb, ctj.data());
      regress(t, rv0b, rjr.data());
    }
    part_sums(t, tvb, rv0b, vwb, psum.data());
    float* G = Gout + (size_t)b * J * 9;
    sf::fit_rot_forward(T.jt, psum.data(), ctj.data(), rjr.data(), jwb, gp, G);
    double acc[sf::kAlign] = {0, 0, 0, 0};
    for (int i = 0; i < V; ++i) sf::align_point_d(tvb + i * 3, rvnb + i * 3, wv ? vwb[i] : 1.f, acc);
    if (joints)
      for (int j = 0; j < J; ++j) sf::align_point_d(ctj.data() + j * 3, rjnb + j * 3, wj ? jwb[j] : 1.f, acc);
    float* tr = trans + (size_t)b * 3;
    sf::align_translation(acc, tr);
    for (size_t k = 0; k < (size_t)V * 3; ++k) mesh[k] = rvnb[k] + tr[k % 3];
    for (int k = 0; k < J * 3; ++k) jn[k] = rjnb[k] + tr[k % 3];
    // ---- reverse: output stage and refinement against the aligned mesh
    if (joints) rjterm = jn;
    else regress(t, mesh.data(), rjterm.data());
    if (final_adjust) part_sums(t, tvb, mesh.data(), vwb, psum.data());
    float tbar[3];
    sf::fit_tail_adjoint(T.jt, G, x + (size_t)b * S, tr, psum.data(), ctj.data(), rjterm.data(), jn.data(), jwb,
                         final_adjust != 0, g_pose + oj, nullptr, nullptr, scr.data(), Gbar.data(), xbar.data(), tbar, pbar.data());
    for (int s = 0; s < S; ++s) g_x[(size_t)b * S + s] = xbar[s];
    for (int c = 0; c < 3; ++c) tbar[c] += g_trans[(size_t)b * 3 + c];
    if (final_adjust) {
      part_sums_adjoint(t, tvb, mesh.data(), vwb, pbar.data(), gtv, meshbar, gvw);
      for (int k = 0; k < J; ++k) gjw[k] += (float)scr[sf::fit_tail_jwbar(J) + k];
      for (int k = 0; k < J * 3; ++k) {
        const float tjb = (float)scr[sf::fit_tail_tjbar(J) + k], rjtb = (float)scr[sf::fit_tail_rjtbar(J) + k];
        jointsbar[k] = (float)scr[sf::fit_tail_rjbar(J) + k] + (joints ? rjtb : 0.f);
        if (joints) gtj[k] += tjb;
        tmp3[k] = tjb, rjr[k] = rjtb;  // (rjr is free until the rotation pass below recomputes it)
      }
      if (!joints) {
        regress_T(t, tmp3.data(), gtv);
        regress_T(t, rjr.data(), meshbar);
      }
    }
    // ---- the alignment (k_fa_align_adj)
    double s3[3] = {0, 0, 0}, q[3];
    for (size_t k = 0; k < (size_t)V * 3; ++k) s3[k % 3] += (double)meshbar[k];
    for (int k = 0; k < J * 3; ++k) s3[k % 3] += (double)jointsbar[k];
    for (int c = 0; c < 3; ++c) q[c] = ((double)tbar[c] + s3[c]) / acc[3];
    for (int i = 0; i < V; ++i) {
      float g[3];
      const float wb = sf::align_point_adjoint(tvb + i * 3, mesh.data() + i * 3, wv ? vwb[i] : 1.f, q, g);
      for (int c = 0; c < 3; ++c) gtv[i * 3 + c] += g[c], meshbar[i * 3 + c] -= g[c];
      if (wv) gvw[i] += wb;
    }
    if (joints)
      for (int j = 0; j < J; ++j) {
        float g[3];
        const float wb = sf::align_point_adjoint(ctj.data() + j * 3, jn.data() + j * 3, wj ? jwb[j] : 1.f, q, g);
        for (int c = 0; c < 3; ++c) gtj[j * 3 + c] += g[c], jointsbar[j * 3 + c] -= g[c];
        if (wj) gjw[j] += wb;
      }
    // ---- the rotation pass that made G
    if (joints) for (int k = 0; k < J * 3; ++k) rjr[k] = rj0[oj + k];
    else regress(t, rv0b, rjr.data());
    part_sums(t, tvb, rv0b, vwb, psum.data());
    sf::fit_rot_adjoint(T.jt, psum.data(), ctj.data(), rjr.data(), jwb, gp, Gbar.data(), pbar.data(),
                        g_Gprev + (size_t)b * J * 9, scr.data());
    part_sums_adjoint(t, tvb, rv0b, vwb, pbar.data(), gtv, grv0, gvw);
    for (int k = 0; k < J; ++k) gjw[k] += (float)scr[J * 6 + k];
    for (int k = 0; k < J * 3; ++k) {
      tmp3[k] = (float)scr[k];
      rjr[k] = (float)scr[J * 3 + k];
      if (joints) gtj[k] += tmp3[k], grj0[k] = rjr[k];
    }
    if (!joints) {
      regress_T(t, tmp3.data(), gtv);
      regress_T(t, rjr.data(), grv0);
    }
  }
  return 0;
}

}  // extern "C"
