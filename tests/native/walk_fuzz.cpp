// Host sanitizer harness for the work item of the index kernels, csrc/walk.h (built by
// tests/test_native_host.py with -fsanitize=address,undefined).  For 16, 48 and 64 pairs an item
// and random per-list pair counts -- empty lists, exactly PER, PER - 1 and PER + 1 among them --
// the items of walk_item must cover every pair exactly once and in order, each with 1..PER pairs
// inside its list and with the list's rows, and their number must stay within walk_max_items, the
// grid the kernels are launched at; list_of is checked at both ends and over runs of equal
// cumulative values.  Prints "ok <cases>" or the first violation.
#include <stdio.h>

#include <random>
#include <vector>

#include "walk.h"

static int fail(const char* what, long long a, long long b, long long c) {
  printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
  return 1;
}

// cum [K + 1]: every x in [cum[0], cum[K]) lies in the list list_of names
static int check_list_of(const std::vector<int64_t>& cum) {
  const int K = (int)cum.size() - 1;
  for (int64_t x = cum[0]; x < cum[K]; ++x) {
    const int k = mk::list_of(cum.data(), K, x);
    if (k < 0 || k >= K || !(cum[k] <= x && x < cum[k + 1])) return fail("list_of", K, x, k);
  }
  return 0;
}

template <int PER>
static int sweep(std::mt19937_64& rng, long long& cases) {
  const int64_t edge[] = {0, 0, 1, PER - 1, PER, PER + 1, 2 * PER, 2 * PER + 1};
  for (int round = 0; round < 400; ++round) {
    const int K = 1 + (int)(rng() % (round % 4 == 0 ? 3 : 70));
    std::vector<int64_t> poff(K + 1, 0), icum(K + 1, 0), offsets(K + 1, 0);
    for (int k = 0; k < K; ++k) {
      // (round 1: no pairs at all; otherwise the edge counts, or up to five items' worth)
      const int64_t c = round == 1 ? 0 : (rng() % 3 ? edge[rng() % 8] : (int64_t)(rng() % (5 * PER + 1)));
      poff[k + 1] = poff[k] + c;
      icum[k + 1] = icum[k] + (c + PER - 1) / PER;
      offsets[k + 1] = offsets[k] + (int64_t)(rng() % 3 ? rng() % 100 : 0);
    }
    const int64_t npairs = poff[K], items = icum[K];
    if (items > mk::walk_max_items(npairs, K, PER / 16)) return fail("grid bound", PER, npairs, items);
    if (check_list_of(icum) || check_list_of(poff)) return 1;
    int64_t next = 0;   // the first pair no item has taken yet
    for (int64_t item = 0; item < items; ++item) {
      const mk::WalkItem w = mk::walk_item<PER>(icum.data(), poff.data(), offsets.data(), K, item);
      if (w.list < 0 || w.list >= K) return fail("list", PER, item, w.list);
      if (w.p0 != next) return fail("pairs not in order", PER, item, w.p0);
      if (w.np < 1 || w.np > PER) return fail("pair count", PER, item, w.np);
      if (w.p0 < poff[w.list] || w.p0 + w.np > poff[w.list + 1]) return fail("pairs outside the list", PER, item, w.list);
      if (w.o0 != offsets[w.list] || w.nl != offsets[w.list + 1] - offsets[w.list])
        return fail("rows", PER, item, w.list);
      next += w.np;
      ++cases;
    }
    if (next != npairs) return fail("pairs not covered", PER, next, npairs);
  }
  return 0;
}

int main() {
  long long cases = 0;
  std::mt19937_64 rng(11);
  if (sweep<16>(rng, cases) || sweep<48>(rng, cases) || sweep<64>(rng, cases)) return 1;
  // runs of equal values at the front, in the middle and at the back; one list
  for (const std::vector<int64_t>& cum : {std::vector<int64_t>{0, 0, 0, 3, 3, 3, 4, 9, 9, 9}, {0, 5}, {0, 0, 1}, {0, 1, 1},
                                          {2, 2, 7, 7, 8}}) {
    if (check_list_of(cum)) return 1;
    const int K = (int)cum.size() - 1;
    if (cum[0] < cum[K]) {   // both ends: the first and the last non-empty list
      int first = 0, last = K - 1;
      while (cum[first + 1] == cum[0]) ++first;
      while (cum[last] == cum[K]) --last;
      if (mk::list_of(cum.data(), K, cum[0]) != first) return fail("list_of front", K, cum[0], first);
      if (mk::list_of(cum.data(), K, cum[K] - 1) != last) return fail("list_of back", K, cum[K] - 1, last);
    }
    ++cases;
  }
  // the small-batch rule: one block below 32768 rows a block, the budget's blocks from there on
  for (int pf = 1; pf <= 4; ++pf) {
    if (mk::walk_blocks(pf, (int64_t)32768 * pf - 1) != 1 || mk::walk_blocks(pf, (int64_t)32768 * pf) != pf)
      return fail("walk_blocks", pf, 0, 0);
    ++cases;
  }
  printf("ok %lld\n", cases);
  return 0;
}
