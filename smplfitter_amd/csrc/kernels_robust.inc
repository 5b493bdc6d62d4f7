// ================================================================================================
// Robust reweighting (smplfit_robust_weights_f32, the rounds of smplfit_fit_robust_f32; DESIGN.md §23): one launch, no
// workspace.  grid B, block 512: one workgroup per instance row.
//   k_robust_reweight   the row's scale sigma — fixed, per row, or max(1.4826 * lower median of the eligible vertex
//                       errors, floor) — then w = w0 * psi(e / (tuning * sigma)) for the row's vertices and joints
//   k_robust_prior      w = w0 (NULL: a constant): what a call of zero rounds returns
// The median is an exact selection: an 8-bit radix select over sf::robust_key in four passes, integer histograms in
// LDS, so the result does not depend on the order of arrival; no float atomics.  The keys of the row are staged in LDS
// where they fit kRobustStageBytes (the flag `staged`, the same in every lane: the one branch of robust_fetch), else
// every pass reads the errors (and prior weights) again.  An ineligible entry (prior weight <= 0) carries bit 31.
// Histogram increments are combined per wave by ballot: the lanes that hold the digit of the first pending lane add
// their count once.  Pass 0 does that for up to kRobustCombine0 distinct digits of a wave step (the top byte of
// errors between a millimetre and a metre takes about three values), the later passes once (rows of ties); lanes
// still pending after that add one each.
// Every output element has one writer.  A row with a non-finite error (vertex or joint), or with a per-row scale that
// is not positive and finite, gets NaN scale and weights.
// ================================================================================================
constexpr int kRobustThreads = 512;  // four workgroups fill a CU's 32 waves (SMPL-X, 43 KB of LDS each: three fit)
constexpr size_t kRobustStageBytes = 48 * 1024;  // with the 1 KB histogram: inside the 64 KB a workgroup gets unasked
constexpr int kRobustCombine0 = 4;
constexpr uint32_t kRobustIneligible = 0x80000000u;
static_assert(kRobustThreads >= 256, "the first 256 threads clear the histogram; wave 0 scans it, four bins a lane");

struct RobustArgs {
  const float *ev, *ej;      // (B, nv); (B, nj) or null
  const float *w0v, *w0j;    // prior weights, each may be null (= 1)
  float *wv, *wj, *sigma;    // out (B, nv); (B, nj) or null; (B) or null
  const float* scale_rows;   // (B) or null
  int nv, nj, loss;
  float tuning, scale, floor;  // scale > 0: the fixed sigma of every row
};

__device__ __forceinline__ uint32_t robust_load_key(const RobustArgs& a, size_t row, int i) {
  const uint32_t key = sf::robust_key(a.ev[row + i]);
  return (a.w0v && !(a.w0v[row + i] > 0.f)) ? key | kRobustIneligible : key;
}
__device__ __forceinline__ uint32_t robust_fetch(const RobustArgs& a, size_t row, int i, const uint32_t* s_keys, int staged) {
  return staged ? s_keys[i] : robust_load_key(a, row, i);
}

// hist[digit] += 1 for every lane with `valid`; called by all lanes of a wave together
__device__ __forceinline__ void robust_hist_add(uint32_t* hist, bool valid, uint32_t digit, int lane, int rounds) {
  for (int r = 0; r < rounds; ++r) {
    const unsigned long long pending = __ballot(valid);
    if (!pending) return;
    const int leader = __ffsll(pending) - 1;
    const uint32_t d0 = __shfl(digit, leader, 64);
    const bool same = valid && digit == d0;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(m));
    if (same) valid = false;
  }
  if (valid) atomicAdd(&hist[digit], 1u);
}

// body(i, key) for every i in [0, ceil(nv / block) * block), by all lanes of every wave together (robust_hist_add needs
// whole waves); i >= nv comes with an ineligible key.  Four keys per thread are requested before the first is used:
// the histogram's ballots and atomics depend on the key, and one memory latency per key is what the pass would cost.
template <class F>
__device__ __forceinline__ void robust_for_keys(const RobustArgs& a, size_t row, const uint32_t* s_keys, int staged, F&& body) {
  constexpr int kAhead = 4;
  const int tid = threadIdx.x;
  for (int base = 0; base < a.nv; base += kAhead * kRobustThreads) {
    uint32_t key[kAhead];
    SF_UNROLL_FULL
    for (int u = 0; u < kAhead; ++u) {
      const int i = base + u * kRobustThreads + tid;
      key[u] = i < a.nv ? robust_fetch(a, row, i, s_keys, staged) : kRobustIneligible;
    }
    SF_UNROLL_FULL
    for (int u = 0; u < kAhead; ++u)
      if (base + u * kRobustThreads < a.nv) body(base + u * kRobustThreads + tid, key[u]);  // (the same in every lane)
  }
}

// w[i] = w0[i] * psi(e[i] / den) for the n entries of a row (w0 null: 1; a zero prior weight: exactly 0); `bad`: NaN.
// LOSS is a template argument so that the loop holds the one weight function and its one division.
template <int LOSS>
__device__ __forceinline__ void robust_write_weights(const float* __restrict__ e, const uint32_t* s_keys, const float* __restrict__ w0,
                                                     float* __restrict__ w, int n, float den, int bad) {
  constexpr int kAhead = 4;
  const int tid = threadIdx.x;
  for (int base = 0; base < n; base += kAhead * kRobustThreads) {
    float ee[kAhead], ww[kAhead];
    SF_UNROLL_FULL
    for (int u = 0; u < kAhead; ++u) {
      const int i = base + u * kRobustThreads + tid;
      const uint32_t key = i >= n ? 0u : s_keys ? s_keys[i] : sf::robust_key(e[i]);
      ee[u] = sf::robust_key_value(key & ~kRobustIneligible);
      ww[u] = (w0 && i < n) ? w0[i] : 1.f;
    }
    SF_UNROLL_FULL
    for (int u = 0; u < kAhead; ++u) {
      const int i = base + u * kRobustThreads + tid;
      const float v = ww[u] == 0.f ? 0.f : ww[u] * sf::robust_weight(LOSS, ee[u] / den);
      // (a bad row is NaN throughout, entries with a zero prior weight included: the row's fit is void, and a weight of
      // exactly 0 there would hide it; include/smplfit.h states this choice)
      if (i < n) w[i] = bad ? den : v;
    }
  }
}

__global__ __launch_bounds__(kRobustThreads) void k_robust_reweight(RobustArgs a, int staged) {
  extern __shared__ uint32_t s_keys[];  // staged: the nv keys of the row
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_sel[3];  // digit and rank inside it picked by the pass, the count of eligible entries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t rv = (size_t)blockIdx.x * a.nv, rj = (size_t)blockIdx.x * a.nj;
  const bool median = !(a.scale > 0.f) && !a.scale_rows;
  if (tid < 256) s_hist[tid] = 0;
  __syncthreads();

  // every error of the row once: non-finite ones, and for the median the keys and the histogram of pass 0
  int bad = 0;
  robust_for_keys(a, rv, nullptr, 0, [&](int i, uint32_t key) {
    bad |= (key & ~kRobustIneligible) >= sf::kRobustInfKey;
    if (staged && i < a.nv) s_keys[i] = key;
    if (median) robust_hist_add(s_hist, !(key & kRobustIneligible), sf::robust_digit(key, 0), lane, kRobustCombine0);
  });
  if (a.ej)
    for (int j = tid; j < a.nj; j += kRobustThreads) bad |= sf::robust_key(a.ej[rj + j]) >= sf::kRobustInfKey;
  bad = __syncthreads_or(bad);  // (also the barrier behind the keys and the histogram)

  float sigma = a.scale_rows ? a.scale_rows[blockIdx.x] : a.scale;
  if (median) {
    uint32_t prefix = 0, rank = 0, n = 0;
    for (int pass = 0; pass < sf::kRobustPasses; ++pass) {
      if (pass > 0) {
        robust_for_keys(a, rv, s_keys, staged, [&](int, uint32_t key) {
          const bool valid = !(key & kRobustIneligible) && sf::robust_prefix(key, pass) == prefix;
          robust_hist_add(s_hist, valid, sf::robust_digit(key, pass), lane, 1);
        });
        __syncthreads();
      }
      if (wave == 0) {  // the bin that holds the element of rank `rank`: four bins a lane, a scan over the wave
        const uint32_t c0 = s_hist[4 * lane], c1 = s_hist[4 * lane + 1], c2 = s_hist[4 * lane + 2], c3 = s_hist[4 * lane + 3];
        const uint32_t s = c0 + c1 + c2 + c3;
        uint32_t inc = s;
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t v = __shfl_up(inc, off, 64);
          if (lane >= off) inc += v;
        }
        if (pass == 0) {
          n = __shfl(inc, 63, 64);
          rank = n ? (n - 1) / 2 : 0;
          if (lane == 0) s_sel[2] = n;
        }
        const uint32_t exc = inc - s;
        if (rank >= exc && rank < inc) {  // (one lane; none where the row has no eligible entry)
          uint32_t r = rank - exc, dg = 4 * lane;
          if (r >= c0) { r -= c0; ++dg; if (r >= c1) { r -= c1; ++dg; if (r >= c2) { r -= c2; ++dg; } } }
          s_sel[0] = dg;
          s_sel[1] = r;
        }
      }
      __syncthreads();
      n = s_sel[2];
      if (n == 0) break;  // (the same in every thread)
      prefix = (prefix << 8) | s_sel[0];
      rank = s_sel[1];
      __syncthreads();
      if (tid < 256) s_hist[tid] = 0;
      __syncthreads();
    }
    sigma = n ? sf::robust_scale(sf::robust_key_value(prefix), a.floor) : a.floor;
  }
  // (a per-row scale is seen on the device alone: one that is not positive and finite makes its row a bad row)
  if (a.scale_rows && !(sigma > 0.f && sigma < __builtin_inff())) bad = 1;
  if (bad) sigma = __builtin_nanf("");
  if (tid == 0 && a.sigma) a.sigma[blockIdx.x] = sigma;

  const float den = a.tuning * sigma;  // (NaN in a bad row)
  const auto write = [&](auto loss) {
    robust_write_weights<decltype(loss)::value>(a.ev + rv, staged ? s_keys : nullptr, a.w0v ? a.w0v + rv : nullptr, a.wv + rv, a.nv, den, bad);
    if (a.ej && a.wj)
      robust_write_weights<decltype(loss)::value>(a.ej + rj, nullptr, a.w0j ? a.w0j + rj : nullptr, a.wj + rj, a.nj, den, bad);
  };
  switch (a.loss) {  // (the same in every thread)
    case sf::kRobustHuber: write(std::integral_constant<int, sf::kRobustHuber>{}); break;
    case sf::kRobustCauchy: write(std::integral_constant<int, sf::kRobustCauchy>{}); break;
    case sf::kRobustGemanMcClure: write(std::integral_constant<int, sf::kRobustGemanMcClure>{}); break;
    default: write(std::integral_constant<int, sf::kRobustTukey>{}); break;
  }
}

// dst[i] = src[i], or `value` where src is null
__global__ __launch_bounds__(256) void k_robust_prior(const float* __restrict__ src, float value, float* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src ? src[i] : value;
}
