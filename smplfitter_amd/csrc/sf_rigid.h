// Per-instance bodies of BodyModel.rototranslate (reference pt/bodymodel.py:435-453) and of its backward, written once
// for the kernels (kernels_rigid.inc, one lane per instance) and the host emulation (tests/hostemu).
//
//   cur = rotvec2mat(root), new_root = mat2rotvec(R cur), pelvis = J_template[0] + J_shapedirs[0, :, :nb] betas
//   (+ kid_J_shapedir[0] kid), new_trans = R x + (R - I) pelvis (+ t), x = trans (post_translate) or trans - t.
//
// j_ext: JointTabs::j_ext, (J, 3, S + 1) [J_template | J_shapedirs (| kid_J_shapedir last)]; only joint 0 is read.
#pragma once
#include "sf_stages.h"

namespace sf {

// Pelvis of the shaped T-pose (bodymodel.py:443-445); kid: the kid factor or NULL (the handle then has a kid column).
SF_HD void rigid_pelvis(const float* j_ext, int S, const float* betas, int nb, const float* kid, float* p) {
  const int S1 = S + 1;
  for (int c = 0; c < 3; ++c) {
    float acc = 0.f;
    for (int s = 0; s < nb; ++s) acc += j_ext[c * S1 + 1 + s] * betas[s];
    p[c] = j_ext[c * S1] + acc;
    if (kid) p[c] += j_ext[c * S1 + S] * kid[0];
  }
}

// x of the translation formula: trans, or trans - t ahead of the rotation
SF_HD void rigid_x(const float* trans, const float* t, bool post, float* x) {
  for (int c = 0; c < 3; ++c) x[c] = (post || !t) ? trans[c] : trans[c] - t[c];
}

// R (9), t (3) or NULL (= 0), root (3) the root rotation vector, trans (3) -> new_root (3), new_trans (3).
// new_root / new_trans may alias root / trans: every input is read before the first output is written.
SF_HD void rototranslate_instance(const float* j_ext, int S, const float* R, const float* t, const float* root,
                                  const float* betas, int nb, const float* kid, const float* trans, bool post,
                                  float* new_root, float* new_trans) {
  float cur[9], M[9], rv[3], p[3], x[3], Rm[9], a[3], b[3];
  rotvec2mat(root, cur);
  m3_mul(R, cur, M);
  mat2rotvec(M, rv);
  rigid_pelvis(j_ext, S, betas, nb, kid, p);
  rigid_x(trans, t, post, x);
  for (int k = 0; k < 9; ++k) Rm[k] = R[k] - (k % 4 == 0 ? 1.f : 0.f);  // R - I (bodymodel.py:447-451)
  m3_vec(R, x, a);
  m3_vec(Rm, p, b);
  for (int c = 0; c < 3; ++c) {
    new_root[c] = rv[c];
    new_trans[c] = (post && t) ? a[c] + t[c] + b[c] : a[c] + b[c];
  }
}

// Backward: g_root (3) / g_trans (3) the cotangents of new_root / new_trans (NULL = 0).  Outputs, each may be NULL:
// gR (9), gt (3), groot (3), gbetas (nb), gtrans (3), gkid (1).  3 x 3 algebra in fp64 on the fp32 values the forward
// read; the rotation adjoints are mat2rotvec_adjoint_add (gradient 0 where the log map's |xyz| is 0) and
// rotvec2mat_vjp (the true derivative of the exponential map at a root of exactly 0).
SF_HD void rototranslate_instance_backward(const float* j_ext, int S, const float* R, const float* t, const float* root,
                                           const float* betas, int nb, const float* kid, const float* trans, bool post,
                                           const float* g_root, const float* g_trans, float* gR, float* gt,
                                           float* groot, float* gbetas, float* gtrans, float* gkid) {
  const int S1 = S + 1;
  float cur[9], M[9], p[3], x[3];
  rotvec2mat(root, cur);
  m3_mul(R, cur, M);
  rigid_pelvis(j_ext, S, betas, nb, kid, p);
  rigid_x(trans, t, post, x);
  double Rd[9], curd[9], Mbar[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, gRd[9], curbar[9];
  for (int k = 0; k < 9; ++k) {
    Rd[k] = R[k];
    curd[k] = cur[k];
  }
  if (g_root) {
    const double rvbar[3] = {g_root[0], g_root[1], g_root[2]};
    mat2rotvec_adjoint_add(M, rvbar, Mbar);
  }
  d3_mult(Mbar, curd, gRd);    // M = R cur:  Rbar = Mbar cur^T
  d3_tmul(Rd, Mbar, curbar);   //             curbar = R^T Mbar
  const double g[3] = {g_trans ? g_trans[0] : 0.0, g_trans ? g_trans[1] : 0.0, g_trans ? g_trans[2] : 0.0};
  double rtg[3];  // R^T g_trans
  for (int c = 0; c < 3; ++c) rtg[c] = Rd[c] * g[0] + Rd[3 + c] * g[1] + Rd[6 + c] * g[2];
  if (gR)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) gR[r * 3 + c] = (float)(gRd[r * 3 + c] + g[r] * ((double)x[c] + (double)p[c]));
  if (groot) {
    float dR[9];
    for (int k = 0; k < 9; ++k) dR[k] = (float)curbar[k];
    rotvec2mat_vjp(root, dR, groot);
  }
  const double gp[3] = {rtg[0] - g[0], rtg[1] - g[1], rtg[2] - g[2]};  // (R^T - I) g_trans
  for (int c = 0; c < 3; ++c) {
    if (gtrans) gtrans[c] = (float)rtg[c];
    if (gt) gt[c] = (float)(post ? g[c] : -rtg[c]);
  }
  if (gbetas)
    for (int s = 0; s < nb; ++s)
      gbetas[s] = (float)(j_ext[1 + s] * gp[0] + j_ext[S1 + 1 + s] * gp[1] + j_ext[2 * S1 + 1 + s] * gp[2]);
  if (gkid) gkid[0] = kid ? (float)(j_ext[S] * gp[0] + j_ext[S1 + S] * gp[1] + j_ext[2 * S1 + S] * gp[2]) : 0.f;
}

// ---- Procrustes alignment of two weighted point sets from their moments -------------------------
// The solve of smplfit_align_points_f32 / smplfit_mesh_error_aligned_f32 (k_align_solve, one lane per row) and of the
// host emulation.  m: the kAlignMoments sums of a row over points taken about provisional origins ox / oy (x' = x - ox
// the model, y' = y - oy the target), so that they hold body-sized numbers wherever the row lies:
//   m[0] = W = sum w      m[1..3] = sum w x'      m[4..6] = sum w y'      m[7 + 3 r + c] = sum w y'_r x'_c
//   m[16] = sum w |x'|^2
// mode: kAlignTranslation (s = 1, R = I), kAlignRigid (R = proj_so3(K), K the centred cross-covariance: det +1 also
// where the best orthogonal fit is a reflection), kAlignSimilarity (s = tr(R^T K) / sum w |x - xbar|^2).
// Out, fp64: s, R (9), t (3) with y ~ s R x + t, and c (3) = ybar' - s R xbar' = t + s R ox - oy, the body-sized
// offset of the centred form  s R (x - ox) + c - (y - oy)  the errors are evaluated in.
// W not positive and finite, a similarity with no spread, or any non-finite moment: every output NaN.
enum { kAlignNone = 0, kAlignRoot = 1, kAlignTranslation = 2, kAlignRigid = 3, kAlignSimilarity = 4, kAlignModeCount = 5 };
enum { kAlignEach = 0, kAlignOnVertices = 1, kAlignOnJoints = 2, kAlignOnCount = 3 };
constexpr int kAlignMoments = 17;
constexpr int kAlignRecord = 18;  // floats of a row's record for the apply kernel: s R (9), c (3), ox (3), oy (3)

SF_HD void align_solve(int mode, const double* m, const double* ox, const double* oy, double* s, double* R, double* t,
                       double* c) {
  const double W = m[0];
  const double iw = 1.0 / W;
  double xm[3], ym[3], K[9], kmax = 0.0;
  for (int k = 0; k < 3; ++k) {
    xm[k] = m[1 + k] * iw;
    ym[k] = m[4 + k] * iw;
  }
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) {
      K[r * 3 + k] = m[7 + r * 3 + k] - W * ym[r] * xm[k];
      kmax = fmax(kmax, fabs(K[r * 3 + k]));
    }
  const double var = m[16] - W * (xm[0] * xm[0] + xm[1] * xm[1] + xm[2] * xm[2]);
  for (int k = 0; k < 9; ++k) R[k] = k % 4 == 0 ? 1.0 : 0.0;
  *s = 1.0;
  bool ok = W > 0.0;
  if (mode >= kAlignRigid) {
    // (the projection normalises its input: scaled to unit size first, so that the fp32 copy neither over- nor underflows)
    float Kf[9], Rf[9];
    const double ik = kmax > 0.0 ? 1.0 / kmax : 0.0;
    for (int k = 0; k < 9; ++k) Kf[k] = (float)(K[k] * ik);
    proj_so3(Kf, Rf);
    for (int k = 0; k < 9; ++k) R[k] = (double)Rf[k];
  }
  if (mode == kAlignSimilarity) {
    double tr = 0.0;
    for (int k = 0; k < 9; ++k) tr += R[k] * K[k];
    ok = ok && var > 0.0;
    *s = tr / var;
  }
  double chk = *s;
  for (int r = 0; r < 3; ++r) {
    double rx = 0.0, ro = 0.0;
    for (int k = 0; k < 3; ++k) {
      rx += R[r * 3 + k] * xm[k];
      ro += R[r * 3 + k] * (xm[k] + ox[k]);
    }
    c[r] = ym[r] - *s * rx;
    t[r] = (ym[r] + oy[r]) - *s * ro;
    chk += c[r] + t[r] + R[r * 3] + R[r * 3 + 1] + R[r * 3 + 2];
  }
  if (!ok || !(chk - chk == 0.0)) {  // (NaN or inf anywhere)
    const double nan = __builtin_nan("");
    *s = nan;
    for (int k = 0; k < 9; ++k) R[k] = nan;
    for (int k = 0; k < 3; ++k) t[k] = c[k] = nan;
  }
}

}  // namespace sf
