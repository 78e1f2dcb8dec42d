// mikmeans — the launch planning of the product-quantised scan (csrc/pq.hip): how many
// workgroups share a (query, probe) pair, which 64-row chunks of the pair's list each of their
// waves takes, and the workgroup's LDS.  Host and device, free of HIP types, so
// tests/native/pq_fuzz.cpp checks under g++ -fsanitize=address,undefined what only the GPU runs
// otherwise: every chunk of every list is taken by exactly one wave.
#pragma once
#include <stdint.h>

#include "plan.h"   // MK_HD, MK_HD_INLINE

namespace mk {

constexpr int PQ_NW = 4;             // waves of a workgroup (TK_NW)
constexpr int PQ_CHUNK = 64;         // rows of a chunk: one a lane
constexpr int PQ_KSUB = 256;         // codewords of a sub-space: one byte a code
constexpr int PQ_MAX_SPLITS = 8;     // workgroups that may share one pair
constexpr int PQ_MAX_M = 32;         // longest result (TOPK_MAX)
// Work items from which a pair is no longer split.  Measured (docs/PQ_INDEX.md): at 16000 and at
// 57000 pairs of ~10^4-row lists eight workgroups a pair still beat one by 20 to 25 %, so the pairs
// count as filling the device only from 2^20 items on -- more than a block of queries holds.
constexpr int64_t PQ_FILL_ITEMS = 1 << 20;

MK_HD inline bool pq_subvectors_ok(int M) { return M == 8 || M == 16 || M == 32 || M == 64; }

// Workgroups a pair: 1 once the pairs alone fill the device (PQ_FILL_ITEMS), doubled up to
// PQ_MAX_SPLITS below that, so a single query still runs on more CUs than it probes lists.  A pure function of npairs.
MK_HD inline int pq_scan_splits(int64_t npairs) {
  int s = 1;
  while (s < PQ_MAX_SPLITS && npairs * s < PQ_FILL_ITEMS) s *= 2;
  return s;
}

// LDS of a workgroup: the pair's table (M sub-spaces of 256 floats: M KiB) and the four waves'
// m keys for the last merge
MK_HD inline int64_t pq_lds_bytes(int M, int m) { return (int64_t)M * PQ_KSUB * 4 + (int64_t)PQ_NW * m * 8; }

// The grid: work item = pair * splits + split; 0 where it would not fit a launch
MK_HD inline int64_t pq_grid(int64_t npairs, int splits) {
  const int64_t items = npairs * splits;
  return items > 0x7fffffff ? 0 : items;
}

// The 64-row chunks of a list of nl rows
MK_HD_INLINE int64_t pq_chunks(int64_t nl) { return (nl + PQ_CHUNK - 1) / PQ_CHUNK; }
// Wave `wid` of split `split` takes the chunks first, first + stride, ... below pq_chunks(nl)
MK_HD_INLINE int64_t pq_first_chunk(int split, int wid) { return (int64_t)split * PQ_NW + wid; }
MK_HD_INLINE int64_t pq_chunk_stride(int splits) { return (int64_t)splits * PQ_NW; }

}  // namespace mk
