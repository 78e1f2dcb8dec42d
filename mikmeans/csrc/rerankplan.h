// mikmeans — the launch planning of the re-rank kernel (csrc/rerank.hip): how a query's R
// candidates are cut into runs, which (query, run) a wave takes and which candidates sixteen lanes
// of it meet at every step.  Host and device, free of HIP types, so tests/native/rerank_fuzz.cpp
// checks under g++ -fsanitize=address,undefined what only the GPU runs otherwise: every
// (query, candidate) is taken by exactly one lane group of one wave.
#pragma once
#include <stdint.h>

#include "plan.h"   // MK_HD, MK_HD_INLINE

namespace mk {

constexpr int RR_NW = 4;          // waves of a workgroup, one work item each
constexpr int RR_GROUP = 16;      // lanes of one (query, candidate) pair: accumulators a_0 .. a_15
constexpr int RR_PAIRS = 4;       // pairs a wave step (64 / RR_GROUP)
constexpr int RR_STEPS = 4;       // steps whose row loads are issued together
constexpr int RR_BATCH = RR_PAIRS * RR_STEPS;   // candidates of one batch of loads
constexpr int RR_MAX_RUN = 64;    // candidates a wave takes: their ids one a lane
constexpr int RR_MIN_RUN = RR_BATCH;
// Waves from which a query's candidates are no longer cut finer: four waves a SIMD on 256 CUs.
constexpr int64_t RR_FILL_ITEMS = 4096;

// Candidates a run: RR_MAX_RUN, halved down to RR_MIN_RUN while the runs do not fill the device, so
// a single query's shortlist still runs on many CUs.  A pure function of (nq, R); no bit of the
// result depends on it.
MK_HD inline int rr_run(int64_t nq, int64_t R) {
  int run = RR_MAX_RUN;
  while (run > RR_MIN_RUN && nq * ((R + run - 1) / run) < RR_FILL_ITEMS) run /= 2;
  return run;
}
// Runs of a query
MK_HD_INLINE int64_t rr_runs(int64_t R, int run) { return (R + run - 1) / run; }
// Work items (one a wave): item = query * runs + run index; 0 where the grid would not fit a launch
MK_HD inline int64_t rr_items(int64_t nq, int64_t R, int run) {
  if (nq <= 0 || R <= 0) return 0;
  const int64_t runs = rr_runs(R, run);
  return runs > INT64_MAX / nq ? 0 : nq * runs;
}
MK_HD inline int64_t rr_grid(int64_t items) {
  const int64_t nb = (items + RR_NW - 1) / RR_NW;
  return nb > 0x7fffffff ? 0 : nb;
}
MK_HD_INLINE int64_t rr_item_query(int64_t item, int64_t runs) { return item / runs; }
// The item's first candidate and how many it takes (1 .. run)
MK_HD_INLINE int64_t rr_item_first(int64_t item, int64_t runs, int run) { return (item % runs) * run; }
MK_HD_INLINE int rr_item_count(int64_t first, int64_t R, int run) {
  return (int)(R - first < run ? R - first : run);
}
// Batches of an item's cnt candidates, and the slot (0 .. cnt) of the run that lane group `grp`
// meets at step `u` of batch `b`; a slot >= cnt is nobody's
MK_HD_INLINE int rr_batches(int cnt) { return (cnt + RR_BATCH - 1) / RR_BATCH; }
MK_HD_INLINE int rr_slot(int b, int u, int grp) { return b * RR_BATCH + u * RR_PAIRS + grp; }
// 16-byte pieces of a row of F columns, V a piece, and the rounds in which 16 lanes take them
// (lane s: pieces s, s + 16, ...)
MK_HD_INLINE int rr_pieces(int F, int V) { return (F + V - 1) / V; }
MK_HD_INLINE int rr_rounds(int pieces) { return (pieces + RR_GROUP - 1) / RR_GROUP; }

}  // namespace mk
