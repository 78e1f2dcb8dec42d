// mikmeans — per-cluster quality table (cluster_report): the per-label reduction of the
// top-2 kernel's output.
//
// Input: idx int32 [N, m], dist float32 [N, m] exactly as csrc/topk.hip writes them (m = 1 or
// 2, read in place through the row stride m).  Row i belongs to label k = idx[i, 0] with
// a^2 = dist[i, 0] and, for m = 2, b^2 = dist[i, 1] (its second-nearest centre).  Every
// per-row quantity depends on that row alone and is added to label k's QUALITY_WORDS u64
// words with integer atomics only (no floating-point add on the reduction path), so the
// table is bitwise the same whatever order rows, waves, launches or ranks arrive in:
//
//   words 0..6   digits of sum a^2 (common.h slot_add: fixed point at 2^-64), word 7 the rows
//   words 8..14  digits of sum a, a = sqrt((double)a^2) in f64
//   word 15      rows whose a^2 is not finite; they add to no other word
//   word 16      sum llrint(s * 2^31), s = 1 - sqrt((double)a^2 / (double)b^2) in [0, 1]: the
//                simplified silhouette (s = 0 for m = 1 or b^2 = 0, s = 1 for b^2 = +inf)
//   word 17      max of a^2's bit pattern (non-negative floats order as unsigned integers)
//   words 18..23 zero
//
// The table is only ever added into: launches over row blocks accumulate.  Rows whose label is
// outside [0, K) are skipped.  Mirror: mikmeans/ops/cpu.py quality_table.
//
// One kernel, two forms (fold.h), the same words.  The global form adds every row straight into
// the global table: ~9 scattered 8-byte atomics a row, each its own memory-side request.  The
// LDS form (K <= QUALITY_LDS_MAX_K) keeps a private copy of words 0..17 of every label in the
// workgroup's LDS, adds its rows there with LDS integer atomics and flushes the non-zero words
// once at the end, lane-contiguous: K * 18 global atomics per workgroup instead of 9 per row.
// Integer sums are associative, so both give the same table bit for bit.
#include "common.h"
#include "fold.h"
#include "kernels.h"

namespace mk {

// One row's contribution to its label's words `w`.
__device__ __forceinline__ void quality_row(unsigned long long* w, float a2f, float b2f, bool second) {
  if (!fold_finite(a2f)) {
    atomicAdd(w + 15, 1ull);
    return;
  }
  const unsigned a2bits = fold_bits(a2f);         // (the clamp: -0 must not reach the maximum)
  const double a2 = (double)__uint_as_float(a2bits);
  slot_add(w, a2, 1);
  slot_add(w + 8, __builtin_sqrt(a2), 0);
  if (second && b2f > 0.0f) {                  // (a NaN or zero b^2: s = 0)
    double s = 1.0;
    if (b2f < __builtin_inff()) {
      s = 1.0 - __builtin_sqrt(a2 / (double)b2f);
      s = s > 0.0 ? s : 0.0;
    }
    const long long q = __builtin_llrint(s * 2147483648.0);
    if (q) atomicAdd(w + 16, (unsigned long long)q);
  }
  // the word only grows, so a stale (smaller) read costs one redundant atomic, never a miss
  const unsigned long long bits = a2bits;
  if (bits > __hip_atomic_load(w + 17, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(w + 17, bits);
}

template <int M, bool LDS>
__global__ __launch_bounds__(LDS ? FOLD_LDS_THREADS : FOLD_THREADS) void quality_kernel(QualityArgs a) {
  constexpr int THREADS = LDS ? FOLD_LDS_THREADS : FOLD_THREADS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* t = reinterpret_cast<unsigned long long*>(smem);   // LDS: [K][QUALITY_LDS_WORDS]
  const int nw = a.K * QUALITY_LDS_WORDS;
  if (LDS) {
    for (int i = threadIdx.x; i < nw; i += THREADS) t[i] = 0ull;
    __syncthreads();
  }
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t row = (int64_t)blockIdx.x * THREADS + threadIdx.x; row < a.N; row += stride) {
    const int k = a.idx[row * M];
    if ((unsigned)k >= (unsigned)a.K) continue;
    float a2, b2 = 0.0f;
    if (M == 2) {
      const float2 d = reinterpret_cast<const float2*>(a.dist)[row];   // one 8-byte load per row
      a2 = d.x;
      b2 = d.y;
    } else {
      a2 = a.dist[row];
    }
    // (the LDS index stays 32-bit arithmetic)
    quality_row(LDS ? t + k * QUALITY_LDS_WORDS : a.table + (int64_t)k * QUALITY_WORDS, a2, b2, M == 2);
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < nw; i += THREADS) {
      const unsigned long long v = t[i];
      if (!v) continue;
      const int k = i / QUALITY_LDS_WORDS, w = i - k * QUALITY_LDS_WORDS;
      unsigned long long* g = a.table + (int64_t)k * QUALITY_WORDS + w;
      if (w == 17) atomicMax(g, v); else atomicAdd(g, v);
    }
  }
}

template <int M>
static hipError_t launch_quality_m(const QualityArgs& a, hipStream_t s, bool lds) {
  if (lds) {
    fold_lds_optin<quality_kernel<M, true>>();
    const unsigned nb = fold_grid(a.N, FOLD_LDS_THREADS, FOLD_LDS_ROWS, FOLD_LDS_BLOCKS);
    const size_t bytes = (size_t)a.K * QUALITY_LDS_WORDS * sizeof(unsigned long long);
    hipLaunchKernelGGL((quality_kernel<M, true>), dim3(nb), dim3(FOLD_LDS_THREADS), bytes, s, a);
  } else {
    const unsigned nb = fold_grid(a.N, FOLD_THREADS, 1, FOLD_MAX_BLOCKS);
    hipLaunchKernelGGL((quality_kernel<M, false>), dim3(nb), dim3(FOLD_THREADS), 0, s, a);
  }
  return hipGetLastError();
}

bool quality_uses_lds(int64_t N, int K) { return K <= QUALITY_LDS_MAX_K && N >= FOLD_LDS_MIN_ROWS; }

hipError_t launch_quality(const QualityArgs& a, hipStream_t s, int path) {
  if (a.N <= 0) return hipSuccess;
  if (a.K <= 0 || (a.m != 1 && a.m != 2)) return hipErrorInvalidValue;
  if (path > 0 && a.K > QUALITY_LDS_MAX_K) return hipErrorInvalidValue;
  const bool lds = path < 0 ? quality_uses_lds(a.N, a.K) : path > 0;
  return a.m == 2 ? launch_quality_m<2>(a, s, lds) : launch_quality_m<1>(a, s, lds);
}

}  // namespace mk
