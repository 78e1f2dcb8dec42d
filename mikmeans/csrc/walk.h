// mikmeans — the work item of a walk over an index's lists (kernels.h IvfWalkArgs describes it):
// how a wave of the scan, the range passes and the repack finds its list, and the grid bound.
// Host and device, free of HIP types, so tests/native/walk_fuzz.cpp checks under
// g++ -fsanitize=address,undefined what only the GPU runs otherwise: the items cover every pair
// exactly once and their number is within the bound.
#pragma once
#include <stdint.h>

#include "plan.h"   // MK_HD, MK_HD_INLINE

namespace mk {

// The k in [0, K) with cum[k] <= x < cum[k + 1], for cum [K + 1] non-decreasing and
// cum[0] <= x < cum[K]: among equal values (empty lists) the last one, whose list is not empty.
MK_HD_INLINE int list_of(const int64_t* cum, int K, int64_t x) {
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct WalkItem {
  int list;
  int64_t p0;   // the item's first pair (a position in the pairs grouped by list)
  int np;       // its pairs, 1..PER
  int64_t o0;   // the list's first row (a position in the index's order)
  int nl;       // the list's rows
};

// Item `item` < icum[K] of a walk with PER pairs an item (offsets [K + 1]: where each list's rows
// start).  Pointers and K by value and PER a template argument: as the args struct by reference
// with a run-time PER this cost ivf_range_kernel up to 10 VGPRs (profiles/r11_01_index_walk.md).
template <int PER>
MK_HD_INLINE WalkItem walk_item(const int64_t* icum, const int64_t* poff, const int64_t* offsets, int K,
                                int64_t item) {
  WalkItem w;
  w.list = list_of(icum, K, item);
  w.p0 = poff[w.list] + (item - icum[w.list]) * PER;
  const int64_t left = poff[w.list + 1] - w.p0;
  w.np = (int)(left < PER ? left : PER);
  w.o0 = offsets[w.list];
  w.nl = (int)(offsets[w.list + 1] - w.o0);
  return w;
}

// The grid bound: sum_l ceil(c_l / PER) <= sum_l floor(c_l / PER) + (lists with pairs)
// <= floor(npairs / PER) + min(K, npairs), PER = 16 P
MK_HD inline int64_t walk_max_items(int64_t npairs, int64_t K, int P) {
  return npairs / (16 * P) + (K < npairs ? K : npairs);
}

// Blocks of 16 rows (or pairs) a wave takes where the kernel's register budget allows pf: one for
// a small batch, so more waves share the work (under ~2 waves per SIMD of a 256-CU part otherwise)
MK_HD inline int walk_blocks(int pf, int64_t n) { return (pf > 1 && n < (int64_t)32768 * pf) ? 1 : pf; }

}  // namespace mk
