// mikmeans — per-cluster exemplar table (cluster_exemplars): for every cluster the m rows
// assigned to it that lie nearest its centre (or farthest from it), selected in one pass
// without sorting the rows.
//
// Input: idx int32 [N, mt], dist float32 [N, mt] exactly as csrc/topk.hip writes them; only
// column 0 is read, through the row stride mt (the ops layer passes mt = 1).  Row i belongs to
// cluster k = idx[i, 0] with a^2 = max(dist[i, 0], +0).  Rows whose label is outside [0, K) and
// rows whose distance is NaN or infinite belong to no list.
//
// Key layout.  A row's 64-bit key is hi << 32 | row: row = row0 + i, the 32-bit index of the
// row in the call's X (the launch gets its block's row0), and
//   nearest:   hi = bits(a^2)
//   farthest:  hi = 0x7F7FFFFF - bits(a^2)       (0x7F7FFFFF: the largest finite float)
// Non-negative finite floats order as unsigned integers, so in both modes a cluster's list is
// its m smallest keys, equal distances by the lower row.  Keys are unique, every key is below
// 2^63 and the empty word (all ones) is larger than every key.
//
// Table: u64 [K, m], all ones before the first launch; slot j of cluster k ends as the
// (j+1)-th smallest key of that cluster.  It is only ever min-inserted into, so launches over
// row blocks accumulate in any order and the result does not depend on the order of rows,
// waves, launches or ranks.  Mirror: mikmeans/ops/cpu.py exemplar_table.
//
// Insertion (exemplar_insert): a thread carries its key down the list,
//   for j in 0..m-1:  old = atomicMin(&L[j], key);  key = max(old, key);  stop when key is empty
// Each step leaves the smaller value in the slot and carries the larger one on, so slot j ends as
// the minimum of everything that ever reached it and everything else that reached it went on to
// slot j+1: by induction the final list is the m smallest keys, whatever the interleaving.
// Every slot only decreases, so a key that is >= a (possibly stale) read of L[m-1] can never
// be in the final list: a thread reads L[m-1] first and skips such a row, and drops a carried
// key the same way; a stale (larger) read costs one redundant atomic, never a miss.  A row
// costs at most m atomics; there is no lock, no spin and no retry loop.  (A key that meets
// itself in a slot stops: accumulating the same rows twice changes nothing.)
//
// One kernel, two forms (fold.h), the same table.  The global form inserts every row straight
// into the global table (64-bit global atomic min; after the lists have warmed up almost every
// row is turned away by the read of L[m-1]).  The LDS form (K * m <= EXEMPLAR_LDS_MAX_WORDS)
// keeps a private [K][m] table in the workgroup's LDS, inserts its rows there with the same
// chain on LDS atomics and then inserts every non-empty entry into the global table with the
// same filtered chain.  The m smallest of a union are the m smallest of the parts' m smallest,
// so both give the same table bit for bit.
// Measured (profiles/r7_02_exemplars.md): the flush is K * m inserts of up to m steps per
// workgroup on lists that all workgroups share, so the LDS form wins for short lists and few
// clusters (where the global form's rows contend on few lists) and loses beyond; the launcher
// takes it for K * m^2 <= EXEMPLAR_LDS_RULE_KMM.
#include "common.h"
#include "fold.h"
#include "kernels.h"

namespace mk {

constexpr unsigned long long EXEMPLAR_EMPTY = ~0ull;

// Min-insert `key` into the list L[0..m): see the header.
__device__ __forceinline__ void exemplar_insert(unsigned long long* L, int m, unsigned long long key) {
  unsigned long long* last = L + (m - 1);
  for (int j = 0; j < m; ++j) {
    // the slots only decrease, so a stale (larger) read costs one redundant atomic, never a miss
    if (key >= __hip_atomic_load(last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const unsigned long long old = atomicMin(L + j, key);
    if (old == key) return;
    key = old > key ? old : key;
    if (key == EXEMPLAR_EMPTY) return;
  }
}

// The key of row `row` (already offset by row0) at squared distance d2; false: the row is in no list.
__device__ __forceinline__ bool exemplar_key(float d2, unsigned row, int farthest, unsigned long long& key) {
  if (!fold_finite(d2)) return false;
  const unsigned bits = fold_bits(d2);
  const unsigned hi = farthest ? 0x7F7FFFFFu - bits : bits;
  key = ((unsigned long long)hi << 32) | row;
  return true;
}

template <bool LDS>
__global__ __launch_bounds__(LDS ? FOLD_LDS_THREADS : FOLD_THREADS) void exemplar_kernel(ExemplarArgs a) {
  constexpr int THREADS = LDS ? FOLD_LDS_THREADS : FOLD_THREADS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* t = reinterpret_cast<unsigned long long*>(smem);   // LDS: [K][m]
  const int nw = a.K * a.m;
  if (LDS) {
    for (int i = threadIdx.x; i < nw; i += THREADS) t[i] = EXEMPLAR_EMPTY;
    __syncthreads();
  }
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t row = (int64_t)blockIdx.x * THREADS + threadIdx.x; row < a.N; row += stride) {
    const int k = a.idx[row * a.mt];
    if ((unsigned)k >= (unsigned)a.K) continue;
    unsigned long long key;
    if (!exemplar_key(a.dist[row * a.mt], a.row0 + (unsigned)row, a.farthest, key)) continue;
    // (the LDS index stays 32-bit arithmetic)
    exemplar_insert(LDS ? t + k * a.m : a.table + (int64_t)k * a.m, a.m, key);
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < nw; i += THREADS) {
      const unsigned long long v = t[i];
      if (v == EXEMPLAR_EMPTY) continue;
      const int k = i / a.m;
      exemplar_insert(a.table + (int64_t)k * a.m, a.m, v);
    }
  }
}

bool exemplar_uses_lds(int64_t N, int K, int m) {
  return (int64_t)K * m <= EXEMPLAR_LDS_MAX_WORDS && (int64_t)K * m * m <= EXEMPLAR_LDS_RULE_KMM &&
         N >= FOLD_LDS_MIN_ROWS;
}

hipError_t launch_exemplars(const ExemplarArgs& a, hipStream_t s, int path) {
  if (a.N <= 0) return hipSuccess;
  if (a.K <= 0 || a.m < 1 || a.m > EXEMPLAR_MAX || a.mt < 1) return hipErrorInvalidValue;
  if ((uint64_t)a.row0 + (uint64_t)a.N > (1ull << 32)) return hipErrorInvalidValue;   // 32-bit row index
  const bool fits = (int64_t)a.K * a.m <= EXEMPLAR_LDS_MAX_WORDS;
  if (path > 0 && !fits) return hipErrorInvalidValue;
  if (path < 0 ? exemplar_uses_lds(a.N, a.K, a.m) : path > 0) {
    fold_lds_optin<exemplar_kernel<true>>();
    const unsigned nb = fold_grid(a.N, FOLD_LDS_THREADS, FOLD_LDS_ROWS, FOLD_LDS_BLOCKS);
    const size_t bytes = (size_t)a.K * a.m * sizeof(unsigned long long);
    hipLaunchKernelGGL(exemplar_kernel<true>, dim3(nb), dim3(FOLD_LDS_THREADS), bytes, s, a);
  } else {
    const unsigned nb = fold_grid(a.N, FOLD_THREADS, 1, FOLD_MAX_BLOCKS);
    hipLaunchKernelGGL(exemplar_kernel<false>, dim3(nb), dim3(FOLD_THREADS), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace mk
