// Host sanitizer harness for the launch planning of the re-rank kernel, csrc/rerankplan.h (built by
// tests/test_pq_refine.py with -fsanitize=address,undefined).  For edge and random (nq, R) the work
// items of rr_items -- walked as the kernel walks them: a workgroup's RR_NW waves, the item's query,
// first candidate and count, its batches, steps and lane groups -- must take every (query,
// candidate) exactly once, with every slot below RR_MAX_RUN (the ids are held one a lane) and every
// taken candidate inside [0, R).  rr_run is checked to be a power of two in [RR_MIN_RUN, RR_MAX_RUN]
// that does not grow as the queries do, rr_grid to cover the items and to refuse what does not fit
// a launch, and the pieces of a row to cover its columns once: lane s of sixteen takes the pieces
// s, s + 16, ... in rr_rounds rounds.  Prints "ok <cases>" or the first violation.
#include <stdio.h>

#include <random>
#include <vector>

#include "rerankplan.h"

static int fail(const char* what, long long a, long long b, long long c) {
  printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
  return 1;
}

static int check_shape(int64_t nq, int64_t R, long long& cases) {
  const int run = mk::rr_run(nq, R);
  if (run < mk::RR_MIN_RUN || run > mk::RR_MAX_RUN || (run & (run - 1)) != 0) return fail("run", nq, R, run);
  const int64_t runs = mk::rr_runs(R, run), items = mk::rr_items(nq, R, run);
  if (items != nq * runs) return fail("items", nq, R, items);
  const int64_t nb = mk::rr_grid(items);
  if (nb * mk::RR_NW < items || (nb - 1) * mk::RR_NW >= items) return fail("grid", nq, R, nb);
  std::vector<int> taken((size_t)(nq * R), 0);
  for (int64_t blk = 0; blk < nb; ++blk) {
    for (int wid = 0; wid < mk::RR_NW; ++wid) {
      const int64_t item = blk * mk::RR_NW + wid;
      if (item >= items) continue;   // (the kernel's bound)
      const int64_t q = mk::rr_item_query(item, runs), first = mk::rr_item_first(item, runs, run);
      if (q < 0 || q >= nq || first < 0 || first >= R) return fail("item", item, q, first);
      const int cnt = mk::rr_item_count(first, R, run);
      if (cnt < 1 || cnt > run || first + cnt > R) return fail("count", item, first, cnt);
      const int batches = mk::rr_batches(cnt);
      for (int b = 0; b < batches; ++b)
        for (int u = 0; u < mk::RR_STEPS; ++u)
          for (int grp = 0; grp < mk::RR_PAIRS; ++grp) {
            const int slot = mk::rr_slot(b, u, grp);
            if (slot < 0 || slot >= mk::RR_MAX_RUN) return fail("slot", b, u, slot);
            if (slot < cnt) ++taken[(size_t)(q * R + first + slot)];   // (the kernel's bound)
          }
    }
  }
  for (int64_t i = 0; i < nq * R; ++i)
    if (taken[(size_t)i] != 1) return fail("candidate not taken once", nq, R, i);
  ++cases;
  return 0;
}

static int check_row(int F, int V, long long& cases) {
  const int np = mk::rr_pieces(F, V), rounds = mk::rr_rounds(np);
  if (np * V < F || (np - 1) * V >= F) return fail("pieces", F, V, np);
  std::vector<int> cols((size_t)F, 0);
  for (int s = 0; s < mk::RR_GROUP; ++s)
    for (int k = 0; k < rounds; ++k) {
      const int t = s + mk::RR_GROUP * k;
      if (t >= np) continue;   // (the kernel's bound)
      for (int e = 0; e < V; ++e)
        if (t * V + e < F) ++cols[(size_t)(t * V + e)];
    }
  for (int c = 0; c < F; ++c)
    if (cols[(size_t)c] != 1) return fail("column not taken once", F, V, c);
  ++cases;
  return 0;
}

int main() {
  long long cases = 0;
  std::mt19937_64 rng(23);
  const int64_t Rs[] = {1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 4096, 8191};
  const int64_t nqs[] = {1, 2, 3, 4, 5, 7, 63, 64, 65, 300};
  for (const int64_t nq : nqs)
    for (const int64_t R : Rs)
      if (check_shape(nq, R, cases)) return 1;
  for (int round = 0; round < 400; ++round)
    if (check_shape(1 + (int64_t)(rng() % 200), 1 + (int64_t)(rng() % (round % 4 ? 300 : 5000)), cases)) return 1;
  // many queries: the longest run, and a run that never grows with nq
  for (const int64_t R : Rs) {
    int last = mk::RR_MIN_RUN;
    for (int64_t nq = 1; nq <= 4 * mk::RR_FILL_ITEMS; nq += 1 + (int64_t)(rng() % 37)) {
      const int run = mk::rr_run(nq, R);
      if (run < last) return fail("run shrinks", nq, R, run);
      last = run;
      ++cases;
    }
    if (mk::rr_run(mk::RR_FILL_ITEMS, R) != mk::RR_MAX_RUN) return fail("run at the fill", R, 0, 0);
  }
  if (mk::rr_items(0, 5, 64) != 0 || mk::rr_items(5, 0, 64) != 0 || mk::rr_items(INT64_MAX / 2, 1000, 64) != 0)
    return fail("items bound", 0, 0, 0);
  if (mk::rr_grid(0) != 0 || mk::rr_grid(1) != 1 || mk::rr_grid(4) != 1 || mk::rr_grid(5) != 2 ||
      mk::rr_grid((int64_t)0x7fffffff * mk::RR_NW) != 0x7fffffff || mk::rr_grid((int64_t)0x7fffffff * mk::RR_NW + 1) != 0)
    return fail("grid bound", 0, 0, 0);
  for (int V = 4; V <= 8; V += 4)
    for (int F = 1; F <= 1100; ++F)
      if (check_row(F, V, cases)) return 1;
  printf("ok %lld\n", cases);
  return 0;
}
