// mikmeans — the frame shared by the per-cluster folds over the top-k kernel's output
// (csrc/quality.hip, csrc/exemplars.hip, csrc/quantiles.hip).
//
// A fold reads idx int32 [N, m] and dist float32 [N, m] exactly as csrc/topk.hip writes them
// and adds every row into a per-cluster integer table with integer atomics only, so the table
// does not depend on the order of rows, waves, launches, row blocks or ranks.  Every fold has
// two forms that give the same table bit for bit:
//   global   FOLD_THREADS threads a workgroup, up to FOLD_MAX_BLOCKS workgroups (the rows past
//            FOLD_MAX_BLOCKS * FOLD_THREADS by the grid-stride loop), every row an atomic on
//            the global table;
//   LDS      one FOLD_LDS_THREADS workgroup per CU (up to FOLD_LDS_BLOCKS, at least
//            FOLD_LDS_ROWS rows a thread) with a private table in up to FOLD_LDS_BYTES of
//            dynamic LDS: fill, barrier, rows, barrier, flush of the words that changed.
//            Taken from FOLD_LDS_MIN_ROWS rows on, where each fold's own rule allows it.
// Which rows count: the label must lie in [0, K) (each fold checks it) and the squared distance
// must be finite; -0 counts as +0 (fold_finite, fold_bits).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mk {

constexpr int FOLD_THREADS = 256;
constexpr int FOLD_MAX_BLOCKS = 2048;
constexpr int FOLD_LDS_THREADS = 1024;
constexpr int FOLD_LDS_BLOCKS = 256;
constexpr int FOLD_LDS_ROWS = 4;
constexpr int FOLD_LDS_BYTES = 160 * 1024;
constexpr int64_t FOLD_LDS_MIN_ROWS = 8192;

// The row filter.  fold_finite: whether a row's squared distance counts at all (not NaN, not
// +-inf).  fold_bits: what a row that counts is ranked and binned by, the bit pattern of
// max(d2, +0): non-negative finite floats order as these unsigned integers, and the clamp keeps -0
// (bit pattern 0x80000000) from ordering above every other distance.  (Two functions, so that a
// fold evaluates each where its row loop needs it.)
__device__ __forceinline__ bool fold_finite(float d2) { return fabsf(d2) < __builtin_inff(); }
__device__ __forceinline__ unsigned fold_bits(float d2) { return __float_as_uint(d2 > 0.0f ? d2 : 0.0f); }

// Workgroups for N rows at rows_per_thread rows a thread, at most cap.
inline unsigned fold_grid(int64_t N, int threads, int rows_per_thread, int64_t cap) {
  const int64_t per = (int64_t)threads * rows_per_thread, want = (N + per - 1) / per;
  return (unsigned)(want < cap ? want : cap);
}

// Opt Kernel in to FOLD_LDS_BYTES of dynamic LDS (past the 64 KiB default), once per process.
template <auto Kernel>
inline void fold_lds_optin() {
  static const hipError_t once =
      hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FOLD_LDS_BYTES);
  (void)once;
}

}  // namespace mk
