// TEST-ONLY stand-alone check of sf::build_share_segments (smplfitter_amd/csrc/sf_tables.cpp), the tables behind
// smplfit_fit_segments_f32 / smplfit_shape_solve_segments_f32, and of the order of the segmented sum.  Built by
// tests/test_share_segments_host.py with -fsanitize=address,undefined (runtimes linked statically) and run as a child
// process; exits non-zero on any mismatch.  A wrong index in these tables would be an out-of-bounds read in
// k_share_partial / k_share_reduce / k_shape_solve, so it is checked on the host.
//
// The sum is emulated as the driver runs it (share_sum in smplfit_hip.hip): the block list walked in groups of whole
// blocks that fit `room` rows of the system buffer, every block summed by sf::sum_rows_f64 (sf_math.h, the function the
// kernels call), then every segment's partial rows the same way.  Each group's rows are copied into a buffer that holds
// exactly them, so an index past the group is an AddressSanitizer report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../smplfitter_amd/csrc/sf_math.h"
#include "../../smplfitter_amd/csrc/sf_tables.h"

namespace {

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

// the tables of `sizes`: every index in range, the blocks tile each segment in order without gap or overlap, block
// counts = ceil(n / 64)
void check_tables(const char* name, const std::vector<int32_t>& sizes) {
  sf::ShareSegments s;
  s.row_seg.assign(3, -7);  // (poisoned: the builder must size and fill its outputs itself)
  s.seg_blk.assign(5, -7);
  s.blk_rows.assign(5, -7);
  const std::string err = sf::build_share_segments(sizes.data(), (int)sizes.size(), s);
  CHECK(err.empty(), "refused: %s", err.c_str());
  long long B = 0;
  for (int32_t n : sizes) B += n;
  const int G = (int)sizes.size();
  CHECK(s.batch == B, "batch %d, expected %lld", s.batch, B);
  CHECK((long long)s.row_seg.size() == B, "row_seg has %zu entries", s.row_seg.size());
  CHECK(s.nseg() == G && (int)s.seg_blk.size() == 2 * G, "seg_blk has %zu entries for %d segments", s.seg_blk.size(), G);
  CHECK(s.blk_rows.size() % 2 == 0, "blk_rows has an odd length");
  const int P = s.nblk();
  int row = 0, blk = 0;
  for (int g = 0; g < G; ++g) {
    const int n = sizes[g], nb = (n + 63) / 64;
    CHECK(s.seg_blk[2 * g] == blk, "segment %d: first block %d, expected %d", g, s.seg_blk[2 * g], blk);
    CHECK(s.seg_blk[2 * g + 1] == nb, "segment %d of %d rows: %d blocks, expected %d", g, n, s.seg_blk[2 * g + 1], nb);
    CHECK(blk + nb <= P, "segment %d: blocks [%d, %d) beyond the %d of the table", g, blk, blk + nb, P);
    int left = n;
    for (int k = 0; k < nb; ++k, ++blk) {
      const int r0 = s.blk_rows[2 * blk], cnt = s.blk_rows[2 * blk + 1];
      CHECK(r0 == row, "block %d: first row %d, expected %d (gap or overlap)", blk, r0, row);
      CHECK(cnt >= 1 && cnt <= 64 && cnt == (left < 64 ? left : 64), "block %d: %d rows with %d left in its segment", blk, cnt, left);
      CHECK((long long)r0 + cnt <= B, "block %d: rows [%d, %d) beyond the batch", blk, r0, r0 + cnt);
      for (int r = r0; r < r0 + cnt; ++r) CHECK(s.row_seg[r] == g, "row %d: segment %d, expected %d", r, s.row_seg[r], g);
      row += cnt;
      left -= cnt;
    }
    CHECK(left == 0, "segment %d: %d rows not covered", g, left);
  }
  CHECK(blk == P, "%d blocks in the table, %d reached from the segments", P, blk);
  CHECK(row == B, "the blocks cover %d rows of %lld", row, B);
  std::printf("ok   tables %s: %d segments, %lld rows, %d blocks\n", name, G, B, P);
}

// sums (segments, NC) of the rows cen (B, NC), as share_sum + the two kernels run them.  s == nullptr: the single
// segment [B] by the kernels' own arithmetic (no tables).
std::vector<double> segmented_sum(const sf::ShareSegments* s, int B, const std::vector<double>& cen, int NC, int room) {
  const int nblk = s ? s->nblk() : (B + 63) / 64, nseg = s ? s->nseg() : 1;
  const auto blk_first = [&](int p) { return s ? s->blk_rows[2 * p] : 64 * p; };
  const auto blk_count = [&](int p) { return s ? s->blk_rows[2 * p + 1] : (B - 64 * p < 64 ? B - 64 * p : 64); };
  std::vector<double> cenP((size_t)nblk * NC), out((size_t)nseg * NC);
  for (int p0 = 0, first = 0; p0 < nblk;) {
    int p1 = p0, cnt = 0;
    while (p1 < nblk && cnt + blk_count(p1) <= room) cnt += blk_count(p1++);
    std::vector<double> chunk(cen.begin() + (size_t)first * NC, cen.begin() + (size_t)(first + cnt) * NC);  // exactly the group
    for (int p = p0; p < p1; ++p)  // k_share_partial
      for (int e = 0; e < NC; ++e)
        cenP[(size_t)p * NC + e] = sf::sum_rows_f64(chunk.data() + (size_t)(blk_first(p) - first) * NC + e, blk_count(p), (size_t)NC);
    p0 = p1;
    first += cnt;
  }
  for (int g = 0; g < nseg; ++g) {  // k_share_reduce
    const int pf = s ? s->seg_blk[2 * g] : 0, np = s ? s->seg_blk[2 * g + 1] : nblk;
    for (int e = 0; e < NC; ++e) out[(size_t)g * NC + e] = sf::sum_rows_f64(cenP.data() + (size_t)pf * NC + e, np, (size_t)NC);
  }
  return out;
}

// the segmented sum over random records == the same two-level sum of every segment on its own, bit for bit, whatever
// the room of the system buffer; the single segment == the table-free arithmetic of a call without a plan
void check_sum(const char* name, const std::vector<int32_t>& sizes, unsigned seed, int NC) {
  sf::ShareSegments s;
  const std::string err = sf::build_share_segments(sizes.data(), (int)sizes.size(), s);
  CHECK(err.empty(), "refused: %s", err.c_str());
  const int B = s.batch;
  std::mt19937_64 rng(seed);
  std::vector<double> cen((size_t)B * NC);
  // (magnitudes spread over 2^40 and both signs: any change of the order of the additions changes the bits)
  for (double& v : cen) v = std::ldexp((double)(int64_t)(rng() >> 11) / 9007199254740992.0 - 0.5, (int)(rng() % 40));
  const std::vector<double> whole = segmented_sum(&s, B, cen, NC, B);
  for (int room : {64, 256, 320}) {  // (general path: share_chunk(B) rows, at least one block)
    const std::vector<double> chunked = segmented_sum(&s, B, cen, NC, room);
    CHECK(std::memcmp(whole.data(), chunked.data(), whole.size() * 8) == 0, "room %d changes the bits of the sums", room);
  }
  int row = 0;
  for (size_t g = 0; g < sizes.size(); ++g) {
    const int n = sizes[g];
    const std::vector<double> rows(cen.begin() + (size_t)row * NC, cen.begin() + (size_t)(row + n) * NC);
    sf::ShareSegments one;
    const int32_t nn = n;
    (void)sf::build_share_segments(&nn, 1, one);
    const std::vector<double> alone = segmented_sum(&one, n, rows, NC, n < 64 ? 64 : n);
    const std::vector<double> plain = segmented_sum(nullptr, n, rows, NC, 256);
    CHECK(std::memcmp(alone.data(), whole.data() + g * NC, (size_t)NC * 8) == 0, "segment %zu (%d rows) differs from its stand-alone sum", g, n);
    CHECK(std::memcmp(plain.data(), alone.data(), (size_t)NC * 8) == 0, "segment %zu (%d rows): the table-free single segment differs", g, n);
    row += n;
  }
  std::printf("ok   sum %s: %zu segments, %d rows, %d entries\n", name, sizes.size(), B, NC);
}

std::vector<int32_t> random_layout(unsigned seed, int count, int max_size) {
  std::mt19937 rng(seed);
  std::vector<int32_t> sizes(count);
  for (int32_t& n : sizes) n = 1 + (int32_t)(rng() % (unsigned)max_size);
  return sizes;
}

void check_refusals() {
  const char* name = "refusals";
  sf::ShareSegments s;
  const int32_t zero[] = {3, 0, 2}, neg[] = {-1}, big[] = {INT32_MAX, 1}, ok[] = {5};
  CHECK(!sf::build_share_segments(ok, 0, s).empty(), "count 0 accepted");
  CHECK(!sf::build_share_segments(nullptr, 1, s).empty(), "null sizes accepted");
  CHECK(!sf::build_share_segments(zero, 3, s).empty(), "a size of 0 accepted");
  CHECK(!sf::build_share_segments(neg, 1, s).empty(), "a negative size accepted");
  CHECK(!sf::build_share_segments(big, 2, s).empty(), "a sum beyond INT32_MAX accepted");
  CHECK(s.row_seg.empty() && s.seg_blk.empty() && s.blk_rows.empty(), "a refused layout leaves tables behind");
  std::printf("ok   refusals\n");
}

}  // namespace

int main() {
  const std::vector<int32_t> mixed = {1, 63, 64, 65, 7, 129, 8, 2};
  check_tables("[1]", {1});
  check_tables("[4096]", {4096});
  check_tables("[1] * 4096", std::vector<int32_t>(4096, 1));
  check_tables("[1,63,64,65,7,129,8,2]", mixed);
  for (unsigned seed = 1; seed <= 6; ++seed)
    check_tables(("random " + std::to_string(seed)).c_str(), random_layout(seed, 1 + (int)(seed * 37 % 200), seed % 2 ? 300 : 5));
  check_refusals();
  check_sum("[1,63,64,65,7,129,8,2]", mixed, 11, 110);
  check_sum("[300,5,70]", {300, 5, 70}, 12, 33);
  check_sum("[1] * 5", std::vector<int32_t>(5, 1), 13, 110);
  check_sum("[1200]", {1200}, 14, 7);
  check_sum("random", random_layout(9, 40, 200), 15, 13);
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  return 0;
}
