// TEST-ONLY stand-alone check of sf::transpose_csr (smplfitter_amd/csrc/sf_tables.cpp), the table behind
// smplfit_transfer_backward_f32: seeded CSR matrices against a dense transpose.  Built by
// tests/test_convert_grad_host.py with -fsanitize=address,undefined (runtimes linked statically) and run as a child
// process; exits non-zero on any mismatch.  A wrong index in this table would be an out-of-bounds read in k_transfer_rows, so it is checked on the host.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../smplfitter_amd/csrc/sf_tables.h"

namespace {

struct Csr {
  int rows = 0, cols = 0;
  std::vector<int32_t> indptr, indices;
  std::vector<float> values;
};

int failures = 0;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::printf("FAIL %s: ", name);             \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
      ++failures;                                 \
      return;                                     \
    }                                             \
  } while (0)

// every value is distinct (1 + the entry's number), so that an entry of the transpose identifies the entry it came from
void check(const char* name, const Csr& m) {
  std::vector<int32_t> tp, ti;
  std::vector<float> tv;
  // (poisoned: the builder must size and fill its outputs itself)
  tp.assign(3, -7);
  ti.assign(5, -7);
  tv.assign(5, -7.f);
  sf::transpose_csr(m.rows, m.cols, m.indptr, m.indices, m.values, tp, ti, tv);
  const int nnz = m.indptr[m.rows];
  CHECK((int)tp.size() == m.cols + 1, "indptr has %zu entries, expected %d", tp.size(), m.cols + 1);
  CHECK((int)ti.size() == nnz && (int)tv.size() == nnz, "%zu indices / %zu values, expected %d", ti.size(), tv.size(), nnz);
  CHECK(tp[0] == 0, "indptr[0] = %d", tp[0]);
  for (int c = 0; c < m.cols; ++c) CHECK(tp[c + 1] >= tp[c], "indptr decreases at column %d", c);
  CHECK(tp[m.cols] == nnz, "indptr ends at %d, nnz = %d", tp[m.cols], nnz);
  for (int e = 0; e < nnz; ++e) CHECK(ti[e] >= 0 && ti[e] < m.rows, "entry %d: row index %d outside [0, %d)", e, ti[e], m.rows);
  // the entries of a column: ascending row order, duplicates of a row in their CSR order (ascending entry number = value)
  for (int c = 0; c < m.cols; ++c)
    for (int e = tp[c] + 1; e < tp[c + 1]; ++e) {
      CHECK(ti[e] >= ti[e - 1], "column %d: rows %d, %d out of order", c, ti[e - 1], ti[e]);
      CHECK(ti[e] > ti[e - 1] || tv[e] > tv[e - 1], "column %d, row %d: duplicates out of CSR order", c, ti[e]);
    }
  // exact values: every entry of the transpose is the entry of M its value names
  std::vector<char> seen(nnz, 0);
  for (int c = 0; c < m.cols; ++c)
    for (int e = tp[c]; e < tp[c + 1]; ++e) {
      const int src = (int)tv[e] - 1;
      CHECK(src >= 0 && src < nnz && tv[e] == m.values[src], "column %d: value %g is no entry of M", c, (double)tv[e]);
      CHECK(!seen[src], "entry %d of M appears twice", src);
      seen[src] = 1;
      CHECK(m.indices[src] == c, "entry %d of M (column %d) filed under column %d", src, m.indices[src], c);
      CHECK(ti[e] >= 0 && m.indptr[ti[e]] <= src && src < m.indptr[ti[e] + 1], "entry %d of M filed under row %d", src, ti[e]);
    }
  // dense transpose (small matrices): sums of duplicates included, in fp64 (the values are small integers: exact)
  if ((long long)m.rows * m.cols <= 4000000) {
    std::vector<double> dense((size_t)m.rows * m.cols, 0.0), denseT((size_t)m.rows * m.cols, 0.0);
    for (int r = 0; r < m.rows; ++r)
      for (int e = m.indptr[r]; e < m.indptr[r + 1]; ++e) dense[(size_t)r * m.cols + m.indices[e]] += m.values[e];
    for (int c = 0; c < m.cols; ++c)
      for (int e = tp[c]; e < tp[c + 1]; ++e) denseT[(size_t)c * m.rows + ti[e]] += tv[e];
    for (int r = 0; r < m.rows; ++r)
      for (int c = 0; c < m.cols; ++c)
        CHECK(dense[(size_t)r * m.cols + c] == denseT[(size_t)c * m.rows + r], "dense transpose differs at (%d, %d)", r, c);
  }
  std::printf("ok   %s: %d x %d, %d entries\n", name, m.rows, m.cols, nnz);
}

// rows of 0 .. 7 entries with seeded columns below `col_limit` (columns from there on stay empty); every third row with
// entries repeats its first column; `heavy` >= 0: that column also gets one entry in each of the first `heavy_rows` rows
Csr random_csr(unsigned seed, int rows, int cols, int col_limit, int heavy = -1, int heavy_rows = 0) {
  std::mt19937 rng(seed);
  Csr m;
  m.rows = rows;
  m.cols = cols;
  m.indptr.push_back(0);
  for (int r = 0; r < rows; ++r) {
    const int n = (int)(rng() % 8);
    int first = -1;
    for (int k = 0; k < n; ++k) {
      int c = (int)(rng() % (unsigned)col_limit);
      if (k == 0) first = c;
      if (k == n - 1 && n > 1 && r % 3 == 0) c = first;  // a repeated column inside the row
      m.indices.push_back(c);
    }
    if (heavy >= 0 && r < heavy_rows) m.indices.push_back(heavy);
    m.indptr.push_back((int32_t)m.indices.size());
  }
  for (size_t e = 0; e < m.indices.size(); ++e) m.values.push_back((float)(e + 1));
  return m;
}

}  // namespace

int main() {
  check("rows of 0-7 entries, empty columns, repeats", random_csr(1, 517, 300, 250));
  check("one column of 2000 entries", random_csr(2, 2500, 400, 380, 7, 2000));
  check("V_in = 1", random_csr(3, 64, 1, 1));
  check("V_out = 1", random_csr(4, 1, 50, 50));
  check("V_in = V_out = 1", random_csr(5, 1, 1, 1));
  check("wider than tall", random_csr(6, 1000, 20000, 20000));
  {
    Csr m;  // no entry at all
    m.rows = 5;
    m.cols = 4;
    m.indptr.assign(6, 0);
    check("empty matrix", m);
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  return 0;
}
