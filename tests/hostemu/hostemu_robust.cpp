// TEST-ONLY host emulation of the robust reweighting (k_robust_reweight, smplfitter_amd/csrc/kernels_robust.inc): the
// per-element functions of sf_math.h the kernel calls — the key of an error, the digit of a pass, the scale from the
// median, the four weight functions — compiled for the host, and a serial radix select built from the same key, digit
// and prefix functions in the kernel's order of passes.  Built by tests/test_robust_host.py as a shared library (g++,
// -ffp-contract=off) and, with ROBUST_MAIN defined, as a stand-alone program under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../smplfitter_amd/csrc/sf_math.h"

namespace {

// The lower median of the eligible entries (w0 NULL: all; else w0 > 0) of e[0, n): `count` = how many there are; the
// return value is meaningless for count 0.  Four passes of 256 bins, as the kernel runs them.
float radix_select(const float* e, const float* w0, int n, int* count) {
  uint32_t prefix = 0, rank = 0;
  *count = 0;
  for (int pass = 0; pass < sf::kRobustPasses; ++pass) {
    std::vector<uint32_t> hist(256, 0u);
    uint32_t total = 0;
    for (int i = 0; i < n; ++i) {
      if (w0 && !(w0[i] > 0.f)) continue;
      const uint32_t key = sf::robust_key(e[i]);
      if (sf::robust_prefix(key, pass) != prefix) continue;
      ++hist.at(sf::robust_digit(key, pass));
      ++total;
    }
    if (pass == 0) {
      *count = (int)total;
      if (!total) return 0.f;
      rank = (total - 1) / 2;
    }
    uint32_t d = 0;
    while (rank >= hist.at(d)) rank -= hist.at(d++);
    prefix = (prefix << 8) | d;
  }
  return sf::robust_key_value(prefix);
}

}  // namespace

extern "C" {

void hostemu_robust_keys(const float* e, uint32_t* keys, int n) {
  for (int i = 0; i < n; ++i) keys[i] = sf::robust_key(e[i]);
}
uint32_t hostemu_robust_digit(uint32_t key, int pass) { return sf::robust_digit(key, pass); }
float hostemu_robust_scale(float median, float floor) { return sf::robust_scale(median, floor); }
void hostemu_robust_psi(int loss, const float* u, float* w, int n) {
  for (int i = 0; i < n; ++i)
    w[i] = loss == 0 ? sf::robust_huber(u[i]) : loss == 1 ? sf::robust_cauchy(u[i])
         : loss == 2 ? sf::robust_geman_mcclure(u[i]) : sf::robust_tukey(u[i]);
}
// the dispatch the kernel calls
void hostemu_robust_weight(int loss, const float* u, float* w, int n) {
  for (int i = 0; i < n; ++i) w[i] = sf::robust_weight(loss, u[i]);
}
int hostemu_robust_select(const float* e, const float* w0, int n, float* median) {
  int count = 0;
  *median = radix_select(e, w0, n, &count);
  return count;
}

}  // extern "C"

#ifdef ROBUST_MAIN
// Stand-alone: the select against a sort for the sizes and the ties of the test plan, in buffers of exactly n floats (an
// index past the row is an AddressSanitizer report).  Exits non-zero on any mismatch.
#include <algorithm>
#include <cstring>
#include <limits>
#include <random>

int main() {
  int failures = 0;
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const int sizes[] = {1, 2, 3, 64, 65, 6890};
  const char* kinds[] = {"random", "ties", "equal", "halfzero", "denormal_inf", "weighted"};
  for (int n : sizes)
    for (int kind = 0; kind < 6; ++kind) {
      std::vector<float> e((size_t)n), w;
      for (int i = 0; i < n; ++i) {
        const float r = uni(rng);
        e[(size_t)i] = kind == 0 || kind == 5 ? r * r * 0.3f
                     : kind == 1 ? (float)(int)(r * 4.f) * 0.25f
                     : kind == 2 ? 0.0123f
                     : kind == 3 ? (i % 2 ? r : 0.f)
                     : (i % 3 == 0 ? std::numeric_limits<float>::denorm_min() * (float)(1 + i % 7)
                        : i % 3 == 1 ? std::numeric_limits<float>::infinity() : r);
      }
      if (kind == 5) {
        w.resize((size_t)n);
        for (int i = 0; i < n; ++i) w[(size_t)i] = i % 3 == 0 ? 0.f : uni(rng) + 0.1f;
      }
      std::vector<float> kept;
      for (int i = 0; i < n; ++i)
        if (w.empty() || w[(size_t)i] > 0.f) kept.push_back(e[(size_t)i]);
      std::sort(kept.begin(), kept.end());
      float med = -1.f;
      const int count = hostemu_robust_select(e.data(), w.empty() ? nullptr : w.data(), n, &med);
      bool ok = count == (int)kept.size();
      if (ok && count) {
        const float want = kept[(kept.size() - 1) / 2];
        ok = std::memcmp(&want, &med, 4) == 0;
      }
      std::printf("%s select n=%d %s count=%d\n", ok ? "ok  " : "FAIL", n, kinds[kind], count);
      failures += !ok;
    }
  return failures ? 1 : 0;
}
#endif
