// TEST-ONLY host emulation of the alignment solve (sf::align_solve, smplfitter_amd/csrc/sf_rigid.h; k_align_solve of
// kernels_align.inc runs the same text one lane per row): the moments of a point set taken serially in fp64 about the
// provisional origins the kernels use (the first point of each set), then the solve.  Built by
// tests/test_align_host.py as a shared library (g++, -ffp-contract=off) and, with ALIGN_MAIN defined, as a stand-alone
// program under -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../smplfitter_amd/csrc/sf_rigid.h"

extern "C" {

// m (17) of n points x, y (n, 3) with weights w (n) or NULL, about ox = x[0], oy = y[0]
void hostemu_align_moments(const float* x, const float* y, const float* w, int n, double* m) {
  for (int k = 0; k < sf::kAlignMoments; ++k) m[k] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double wi = w ? (double)w[i] : 1.0;
    double a[3], b[3];
    for (int k = 0; k < 3; ++k) {
      a[k] = (double)x[3 * i + k] - (double)x[k];
      b[k] = (double)y[3 * i + k] - (double)y[k];
    }
    m[0] += wi;
    for (int k = 0; k < 3; ++k) {
      m[1 + k] += wi * a[k];
      m[4 + k] += wi * b[k];
      for (int c = 0; c < 3; ++c) m[7 + 3 * k + c] += b[k] * (wi * a[c]);
    }
    m[16] += wi * (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  }
}

// out (16): s, R (9), t (3), c (3)
void hostemu_align_solve(int mode, const double* m, const double* ox, const double* oy, double* out) {
  sf::align_solve(mode, m, ox, oy, out, out + 1, out + 10, out + 13);
}

// both steps on a set; the origins are the sets' first points
void hostemu_align_points(int mode, const float* x, const float* y, const float* w, int n, double* out) {
  double m[sf::kAlignMoments];
  hostemu_align_moments(x, y, w, n, m);
  const double ox[3] = {x[0], x[1], x[2]}, oy[3] = {y[0], y[1], y[2]};
  hostemu_align_solve(mode, m, ox, oy, out);
}

}  // extern "C"

#ifdef ALIGN_MAIN
// Stand-alone: clouds under a known similarity are recovered (the residual of every point below 1e-5 of the cloud's
// size, det R = +1), in buffers of exactly n points; zero weights and a cloud without spread give NaN.  Exits non-zero
// on any failure.
#include <random>

static bool recovered(int mode, int n, int kind, std::mt19937& rng) {
  std::normal_distribution<float> nrm(0.f, 1.f);
  std::vector<float> x((size_t)3 * n), y((size_t)3 * n), w((size_t)n);
  const float far = kind == 3 ? 1000.f : 0.f, s = mode == sf::kAlignSimilarity ? 1.3f : 1.f;
  const float ca = std::cos(0.7f), sa = std::sin(0.7f);
  for (int i = 0; i < n; ++i) {
    float p[3] = {nrm(rng), nrm(rng), nrm(rng)};
    if (kind == 1) p[2] = 0.f;                 // coplanar
    if (kind == 2) p[1] = p[2] = 0.f;          // collinear
    const float q[3] = {ca * p[0] - sa * p[1], sa * p[0] + ca * p[1], p[2]};
    const bool rot = mode >= sf::kAlignRigid;
    for (int k = 0; k < 3; ++k) {
      x[(size_t)3 * i + k] = p[k] + far;
      y[(size_t)3 * i + k] = s * (rot ? q[k] : p[k]) + 2.f + far;
    }
    w[(size_t)i] = 0.5f + (float)(i % 3);
  }
  double o[16];
  hostemu_align_points(mode, x.data(), y.data(), kind == 4 ? nullptr : w.data(), n, o);
  double worst = 0.0;
  for (int i = 0; i < n; ++i) {
    double e2 = 0.0;
    for (int r = 0; r < 3; ++r) {
      double v = o[10 + r] - (double)y[(size_t)3 * i + r];
      for (int k = 0; k < 3; ++k) v += o[0] * o[1 + 3 * r + k] * (double)x[(size_t)3 * i + k];
      e2 += v * v;
    }
    worst = std::fmax(worst, std::sqrt(e2));
  }
  const double* R = o + 1;
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  // (the inputs are fp32: at 1000 m their own rounding is 6e-5 m)
  return worst <= (kind == 3 ? 5e-4 : 1e-5) && std::fabs(det - 1.0) < 1e-6;
}

int main() {
  int failures = 0;
  std::mt19937 rng(7);
  const char* kinds[] = {"random", "coplanar", "collinear", "far", "unweighted"};
  for (int mode = sf::kAlignTranslation; mode <= sf::kAlignSimilarity; ++mode)
    for (int n : {3, 24, 1000})
      for (int kind = 0; kind < 5; ++kind) {
        const bool ok = recovered(mode, n, kind, rng);
        std::printf("%s solve mode=%d n=%d %s\n", ok ? "ok  " : "FAIL", mode, n, kinds[kind]);
        failures += !ok;
      }
  {  // NaN rows
    std::vector<float> x = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f}, y = x, w0 = {0.f, 0.f, 0.f};
    std::vector<float> same = {1.f, 2.f, 3.f, 1.f, 2.f, 3.f, 1.f, 2.f, 3.f};
    double o[16];
    hostemu_align_points(sf::kAlignRigid, x.data(), y.data(), w0.data(), 3, o);
    bool ok = true;
    for (double v : o) ok = ok && v != v;
    hostemu_align_points(sf::kAlignSimilarity, same.data(), y.data(), nullptr, 3, o);
    for (double v : o) ok = ok && v != v;
    hostemu_align_points(sf::kAlignRigid, same.data(), y.data(), nullptr, 3, o);  // (no spread: rigid is still defined)
    for (double v : o) ok = ok && v == v;
    std::printf("%s solve nan rows\n", ok ? "ok  " : "FAIL");
    failures += !ok;
  }
  return failures ? 1 : 0;
}
#endif
