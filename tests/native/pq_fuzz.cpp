// Host sanitizer harness for the launch planning of the product-quantised scan, csrc/pqplan.h
// (built by tests/test_pq.py with -fsanitize=address,undefined).  For random list lengths -- empty
// lists, exactly 64 rows, 63 and 65, lengths around every split's whole sweep among them -- and
// every split count 1..PQ_MAX_SPLITS, the chunks that wave `wid` of split `split` takes
// (pq_first_chunk, then steps of pq_chunk_stride below pq_chunks) must cover every chunk of the
// list exactly once, and every row of the list must lie in exactly one chunk taken.  pq_scan_splits
// is checked to be a non-increasing power of two in [1, PQ_MAX_SPLITS] that is 1 once the pairs
// fill the device, pq_lds_bytes to stay within the 160 KiB of a CU for every (M, m), and pq_grid
// to refuse what does not fit a launch.  Prints "ok <cases>" or the first violation.
#include <stdio.h>

#include <random>
#include <vector>

#include "pqplan.h"

static int fail(const char* what, long long a, long long b, long long c) {
  printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
  return 1;
}

static int check_list(int64_t nl, int splits, long long& cases) {
  const int64_t nch = mk::pq_chunks(nl);
  if (nch * mk::PQ_CHUNK < nl || (nch > 0 && (nch - 1) * mk::PQ_CHUNK >= nl)) return fail("chunks", nl, nch, 0);
  std::vector<int> taken((size_t)nch, 0);
  std::vector<int> rows((size_t)nl, 0);
  const int64_t stride = mk::pq_chunk_stride(splits);
  if (stride != (int64_t)splits * mk::PQ_NW) return fail("stride", splits, stride, 0);
  for (int split = 0; split < splits; ++split) {
    for (int wid = 0; wid < mk::PQ_NW; ++wid) {
      for (int64_t c = mk::pq_first_chunk(split, wid); c < nch; c += stride) {
        ++taken[(size_t)c];
        for (int lane = 0; lane < mk::PQ_CHUNK; ++lane) {
          const int64_t row = c * mk::PQ_CHUNK + lane;
          if (row < nl) ++rows[(size_t)row];   // (the kernel's bound: a lane past the list loads nothing)
        }
      }
    }
  }
  for (int64_t c = 0; c < nch; ++c)
    if (taken[(size_t)c] != 1) return fail("chunk not taken once", nl, splits, c);
  for (int64_t r = 0; r < nl; ++r)
    if (rows[(size_t)r] != 1) return fail("row not taken once", nl, splits, r);
  ++cases;
  return 0;
}

int main() {
  long long cases = 0;
  std::mt19937_64 rng(17);
  for (int splits = 1; splits <= mk::PQ_MAX_SPLITS; ++splits) {
    const int64_t sweep = (int64_t)splits * mk::PQ_NW * mk::PQ_CHUNK;
    const int64_t edge[] = {0, 1, 63, 64, 65, 255, 256, 257, sweep - 1, sweep, sweep + 1, 2 * sweep - 1, 2 * sweep + 65};
    for (const int64_t nl : edge)
      if (check_list(nl, splits, cases)) return 1;
    for (int round = 0; round < 300; ++round)
      if (check_list((int64_t)(rng() % (round % 3 ? 700 : 9000)), splits, cases)) return 1;
  }
  int last = mk::PQ_MAX_SPLITS;
  for (int64_t npairs = 1; npairs <= 4 * mk::PQ_FILL_ITEMS; npairs += (npairs < 4096 ? 1 : 1 + (int64_t)(rng() % 97))) {
    const int s = mk::pq_scan_splits(npairs);
    if (s < 1 || s > mk::PQ_MAX_SPLITS || (s & (s - 1)) != 0 || s > last) return fail("splits", npairs, s, last);
    if (npairs >= mk::PQ_FILL_ITEMS && s != 1) return fail("splits past the fill", npairs, s, 0);
    if (s < mk::PQ_MAX_SPLITS && npairs * s < mk::PQ_FILL_ITEMS) return fail("splits under the fill", npairs, s, 0);
    last = s;
    ++cases;
  }
  if (mk::pq_scan_splits(1) != mk::PQ_MAX_SPLITS) return fail("one pair", mk::pq_scan_splits(1), 0, 0);
  for (int M = 1; M <= 128; ++M) {
    const bool ok = M == 8 || M == 16 || M == 32 || M == 64;
    if (mk::pq_subvectors_ok(M) != ok) return fail("subvectors", M, 0, 0);
    if (!ok) continue;
    for (int m = 1; m <= mk::PQ_MAX_M; ++m) {
      const int64_t b = mk::pq_lds_bytes(M, m);
      if (b != (int64_t)M * 1024 + 32 * m || b > 160 * 1024) return fail("lds", M, m, b);
      ++cases;
    }
  }
  if (mk::pq_grid(5, 8) != 40 || mk::pq_grid(0x7fffffff, 1) != 0x7fffffff || mk::pq_grid(0x10000000, 8) != 0 ||
      mk::pq_grid(0, 8) != 0)
    return fail("grid", 0, 0, 0);
  printf("ok %lld\n", cases);
  return 0;
}
