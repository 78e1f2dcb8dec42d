// mikmeans — the workgroup scan and the workgroup sum of the row kernels (csrc/rows.hip, csrc/kpp.hip,
// csrc/ivf.hip's partition, the radix selects through csrc/bins.h), once.  Device only.  Every piece
// is called by all NT threads of a workgroup of NT / 64 whole waves, under uniform control flow, and
// fixes the order of every addition it makes: for f64 that order is the output's bits.
#pragma once
#include "common.h"

namespace mk {

// Inclusive scan inside a wave: v += the value of lane - o, for o = 1, 2, .. 32, where lane >= o.
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// Inclusive scan of one value per thread over the workgroup, thread order; total = the sum of all
// NT values, to every thread.  waves: NT / 64 LDS words.  Each wave scans itself and its lane 63
// publishes the wave's sum; a thread's prefix is T(0) plus the words of the waves before its own, in
// wave order, and total is the words added in wave order from the first (not from zero).  The first
// barrier makes the words visible, the second keeps them until every thread has read them: a caller
// may call again at once with the same waves.
// Callers: compact_write_kernel and scan_slices (i64), wkpp_d2_kernel and wkpp_pick_kernel (f64, 256
// threads), bins_running_count (u64, 256 threads).
template <int NT, typename T>
__device__ __forceinline__ T block_incl_scan(T v, T* waves, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = wave_incl_scan(v);
  if (lane == 63) waves[w] = v;
  __syncthreads();
  T prefix = T(0);
  total = waves[0];
#pragma unroll
  for (int j = 0; j < NT / 64; ++j) {
    const T s = waves[j];
    if (j < w) prefix += s;
    if (j > 0) total += s;
  }
  __syncthreads();
  return v + prefix;
}

// One workgroup's exclusive scan over n int64 cells, NT at a time with a running carry:
// store(i, the sum of load(0 .. i - 1)) for every i < n, ascending; returns the sum of all cells to
// every thread.  load(i) and store(i, .) run in the same thread, so a store may overwrite the cell
// its load read.  Callers: compact_scan_kernel, partition_scan_kernel (1024 threads).
template <int NT, typename Load, typename Store>
__device__ __forceinline__ int64_t scan_slices(int64_t n, Load load, Store store) {
  __shared__ int64_t waves[NT / 64];
  int64_t carry = 0;
  for (int64_t s0 = 0; s0 < n; s0 += NT) {
    const int64_t i = s0 + threadIdx.x;
    const int64_t v = i < n ? load(i) : 0;
    int64_t total;
    const int64_t incl = block_incl_scan<NT>(v, waves, total);
    if (i < n) store(i, carry + incl - v);
    carry += total;
  }
  return carry;
}

// The waves' sums of one value per thread: waves[w] = wave_sum over wave w (common.h: the xor
// butterfly 32 .. 1), visible to every thread on return (one barrier; a second call needs another
// array, or a barrier of the caller's).  One thread then combines the words with one of the two
// orders below, and the call says which.
// Callers: wdot_partial_kernel, wdot_final_kernel (sum_pairs4), kpp_d2_kernel, compact_count_kernel
// (sum_in_order).
template <int NT, typename T>
__device__ __forceinline__ void block_wave_sums(T v, T* waves) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
  __syncthreads();
}
// ((0 + w0) + w1) + ..
template <typename T>
__device__ __forceinline__ T sum_in_order(const T* waves, int n) {
  T s = T(0);
  for (int w = 0; w < n; ++w) s += waves[w];
  return s;
}
// (w0 + w1) + (w2 + w3): four waves
template <typename T>
__device__ __forceinline__ T sum_pairs4(const T* waves) {
  return (waves[0] + waves[1]) + (waves[2] + waves[3]);
}

}  // namespace mk
