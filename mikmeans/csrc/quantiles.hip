// mikmeans — per-cluster distance quantiles (cluster_quantiles): for every cluster and every
// requested q an exact order statistic of the distances of the rows assigned to it, selected
// without sorting the rows: a most-significant-digit radix select over the distance bits.
//
// Input: idx int32 [N, mt], dist float32 [N, mt] exactly as csrc/topk.hip writes them; only
// column 0 is read, through the row stride mt (the ops layer passes mt = 1).  Row i belongs to
// cluster k = idx[i, 0] with a^2 = max(dist[i, 0], +0), bits = the bit pattern of a^2.  Rows
// whose label is outside [0, K) and rows whose distance is NaN or infinite count nowhere.
//
// Non-negative finite floats order as their bit patterns, so the element at sorted position r of
// a cluster is found digit by digit, most significant first: four passes of 8-bit digits at
// shift s = 24, 16, 8, 0.  Every (cluster k, quantile j) pair carries a prefix P (the bits fixed
// so far, int32 [K, Q]) and a remaining rank R (int64 [K, Q]).
//
//   pass 0    table u64 [K, 256]: a row adds one to (k, bits >> 24); one histogram for all j.
//             Select: n_k = the sum of the cluster's bins (written to counts),
//             r = clamp(ceil(q_j * n_k) - 1, 0, n_k - 1) with the product one f64 multiply,
//             b = the smallest bin whose running count exceeds r; P = b << 24, R = r - the count
//             below b.
//   pass 1-3  table u64 [K, Q, 256]: a row adds one to (k, j, (bits >> s) & 255) for every j with
//             bits >> (s + 8) == P[k, j] >> (s + 8).  Select: b = the smallest bin whose running
//             count exceeds R; P |= b << s, R -= the count below b.
//
// After pass 3 P[k, j] is the bit pattern of the answer: a real row's a^2, no interpolation and
// no floating-point add anywhere.  A pair whose bins hold no more than R rows (an empty cluster)
// keeps P and R (pass 0 writes zeros); the caller reports NaN where counts is 0.
//
// Order-free.  The tables are only ever added into, with integer atomics: launches over row
// blocks accumulate, a multi-rank job sums the ranks' tables before each select, and the result
// does not depend on the order of rows, waves, launches, row blocks or ranks.  Mirror:
// mikmeans/ops/cpu.py quantile_hist / quantile_select.
//
// Same-address contention is the design problem: within one cluster nearly every row shares the
// top byte of its distance, so in pass 0 a whole cluster lands on one to three bins, and with
// few clusters every lane of a wave hits the same handful of addresses.  wave_add therefore
// aggregates inside the wave before the atomic: for up to `agg` rounds it takes the first
// pending lane's (list, digit) key, ballots the lanes that share it and lets that lane add their
// count; lanes still pending after the rounds (diverse keys) add one each.  Integer sums are
// associative, so every choice of `agg` gives the same table.
//
// Two kernels on the frame of fold.h, the same table.  quantile_hist_kernel adds into the global
// table (64-bit global atomic add).  quantile_hist_lds_kernel (lists = K or K * Q <=
// QUANTILE_LDS_MAX_LISTS) keeps a private [lists][256] u32 table in the workgroup's LDS, adds
// its rows there and flushes the non-zero bins with 64-bit global adds;
// a launch takes fewer than 2^32 rows, so a u32 bin cannot wrap.  Past 160 lists the same kernel
// runs banded: band b (the grid's y) holds lists [160 b, 160 b + 160), reads every row and skips
// the rows of the other bands, so the rows are swept ceil(lists / 160) times.  Integer sums are
// associative and every list is flushed by the workgroups of one band, so all forms give the
// same table bit for bit.
//
// Measured (profiles/r7_03_quantiles.md, N = 10^7).  The LDS form is taken wherever the lists
// fit: pass 0 costs 0.04 ms against 10.6 (K = 8) and 0.72 (K = 160) for the global form; the
// banded form where its sweeps cost less than the global form's atomics (kernels.h has the
// rule: pass 0 up to 26 bands, pass 1 up to 8, passes 2 and 3 never: few rows match there).  LDS
// atomics on one address need no help from the wave (every round of aggregation is a loss
// there: QUANTILE_LDS_AGG_ROUNDS = 0).  On the global form (more than 160 lists) rows in random
// order give a wave nothing to share and two rounds cost under 1 %; rows ordered by label put
// every wave on one cluster, and two rounds take pass 0 from 0.74 to 0.045 ms at K = 1024
// (QUANTILE_AGG_ROUNDS = 2; more rounds only add to the later passes, whose digits differ).
#include "bins.h"
#include "common.h"
#include "fold.h"
#include "kernels.h"

namespace mk {

// One more row in t[key] for every lane with `pending`; every lane of the wave calls it (the
// callers' loops have wave-uniform trip counts).  See the header.
template <typename T>
__device__ __forceinline__ void wave_add(T* t, unsigned key, bool pending, int rounds) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(pending);
  for (int r = 0; r < rounds && todo; ++r) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned key0 = __shfl(key, leader);
    const bool mine = pending && key == key0;
    const unsigned long long same = __ballot(mine);
    if (lane == leader) atomicAdd(t + key0, (T)__popcll(same));
    pending = pending && !mine;
    todo &= ~same;
  }
  if (pending) atomicAdd(t + key, (T)1);
}

// This workgroup's rows of one pass into t: the global table (list0 = 0, nlists = all) or the
// LDS-private one, which holds lists [list0, list0 + nlists) and skips the rows of the others.
template <typename T>
__device__ __forceinline__ void quantile_rows(const QuantileHistArgs& a, T* t, int threads, unsigned list0,
                                              unsigned nlists) {
  constexpr int U = 4;   // rows in flight per thread: the loop waits on memory, not on the adds
  const int s = 24 - 8 * a.pass;
  const int64_t stride = (int64_t)gridDim.x * threads;
  // (the trip count is the workgroup's, not the thread's: wave_add needs every lane)
  for (int64_t base = (int64_t)blockIdx.x * threads; base < a.N; base += U * stride) {
    int kk[U];
    float dd[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = base + u * stride + threadIdx.x;
      kk[u] = row < a.N ? a.idx[row * a.mt] : -1;   // (-1: outside every table)
      dd[u] = row < a.N ? a.dist[row * a.mt] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = (unsigned)kk[u] < (unsigned)a.K && fold_finite(dd[u]);
      const unsigned k = ok ? (unsigned)kk[u] : 0u;
      const unsigned bits = fold_bits(dd[u]);
      if (a.pass == 0) {
        const unsigned slot = k - list0;
        const bool hit = ok && slot < nlists;
        wave_add(t, (hit ? slot : 0u) * QUANTILE_BINS + (bits >> 24), hit, a.agg);
      } else {
        const unsigned digit = (bits >> s) & 255u;
        for (int j = 0; j < a.Q; ++j) {
          const unsigned list = k * a.Q + j, slot = list - list0;
          const bool hit = ok && slot < nlists && (bits >> (s + 8)) == ((unsigned)a.prefix[list] >> (s + 8));
          wave_add(t, (hit ? slot : 0u) * QUANTILE_BINS + digit, hit, a.agg);
        }
      }
    }
  }
}

__global__ __launch_bounds__(FOLD_THREADS) void quantile_hist_kernel(QuantileHistArgs a) {
  quantile_rows(a, a.table, FOLD_THREADS, 0u, (unsigned)quantile_lists(a.K, a.Q, a.pass));
}

// Band blockIdx.y of the lists (one band when they fit a workgroup's LDS): see kernels.h.
__global__ __launch_bounds__(FOLD_LDS_THREADS) void quantile_hist_lds_kernel(QuantileHistArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* t = reinterpret_cast<unsigned*>(smem);   // [nlists][256]
  const unsigned lists = (unsigned)quantile_lists(a.K, a.Q, a.pass);
  const unsigned list0 = blockIdx.y * QUANTILE_LDS_MAX_LISTS;
  const unsigned nlists = lists - list0 < (unsigned)QUANTILE_LDS_MAX_LISTS ? lists - list0 : QUANTILE_LDS_MAX_LISTS;
  const int nw = (int)nlists * QUANTILE_BINS;
  for (int i = threadIdx.x; i < nw; i += FOLD_LDS_THREADS) t[i] = 0u;
  __syncthreads();
  quantile_rows(a, t, FOLD_LDS_THREADS, list0, nlists);
  __syncthreads();
  unsigned long long* g = a.table + (int64_t)list0 * QUANTILE_BINS;
  for (int i = threadIdx.x; i < nw; i += FOLD_LDS_THREADS) {
    const unsigned v = t[i];
    if (v) atomicAdd(g + i, (unsigned long long)v);
  }
}

// One workgroup per cluster, one thread per bin: the running count over the bins, then the bin
// that holds rank R.
__global__ __launch_bounds__(QUANTILE_BINS) void quantile_select_kernel(QuantileSelectArgs a) {
  __shared__ unsigned long long wsum[QUANTILE_BINS / 64];
  const int k = blockIdx.x, b = threadIdx.x;
  const int s = 24 - 8 * a.pass;
  unsigned long long c = 0, incl = 0, total = 0;
  for (int j = 0; j < a.Q; ++j) {
    const int64_t pair = (int64_t)k * a.Q + j;
    // (every thread reads the pair's rank before the barriers below, its one writer writes after)
    int64_t R = a.pass ? a.rank[pair] : 0;
    if (a.pass > 0 || j == 0) {
      c = a.table[(a.pass ? pair : (int64_t)k) * QUANTILE_BINS + b];
      bins_running_count(c, wsum, incl, total);
    }
    if (a.pass == 0) {
      const int64_t n = (int64_t)total;
      R = (int64_t)__builtin_ceil(a.q[j] * (double)n) - 1;   // one f64 multiply, as the mirror's
      if (R > n - 1) R = n - 1;
      if (R < 0) R = 0;
      if (b == 0 && j == 0) a.counts[k] = n;
      if (b == 0 && n == 0) {
        a.prefix[pair] = 0;
        a.rank[pair] = 0;
      }
    }
    const unsigned long long excl = incl - c;
    if (incl > (unsigned long long)R && excl <= (unsigned long long)R) {   // at most one bin
      a.prefix[pair] = (a.pass ? a.prefix[pair] : 0) | (int32_t)((unsigned)b << s);
      a.rank[pair] = R - (int64_t)excl;
    }
  }
}

bool quantile_uses_lds(int64_t N, int64_t lists) {
  return lists <= QUANTILE_LDS_MAX_LISTS && N >= FOLD_LDS_MIN_ROWS && N < (int64_t(1) << 32);
}

int quantile_path(int64_t N, int64_t lists, int pass) {
  if (quantile_uses_lds(N, lists)) return 1;
  const int64_t most = pass == 0 ? QUANTILE_BAND_MAX_PASS0 : pass == 1 ? QUANTILE_BAND_MAX : 0;
  const bool banded = lists > QUANTILE_LDS_MAX_LISTS && quantile_bands(lists) <= most &&
                      N >= QUANTILE_BAND_MIN_ROWS && N < (int64_t(1) << 32);
  return banded ? 2 : 0;
}

hipError_t launch_quantile_hist(const QuantileHistArgs& args, hipStream_t s, int path) {
  QuantileHistArgs a = args;
  if (a.N <= 0) return hipSuccess;
  if (a.K <= 0 || a.mt < 1 || a.pass < 0 || a.pass >= QUANTILE_PASSES || a.agg < -1 || a.agg > QUANTILE_AGG_MAX)
    return hipErrorInvalidValue;
  if (a.pass > 0 && (a.Q < 1 || a.Q > QUANTILE_MAX_Q || !a.prefix)) return hipErrorInvalidValue;
  const int64_t lists = quantile_lists(a.K, a.Q, a.pass);
  if (lists > (int64_t(1) << 24)) return hipErrorInvalidValue;   // 32-bit (list, digit) keys
  const int64_t bands = quantile_bands(lists);
  if (path > 2 || (path > 0 && a.N >= (int64_t(1) << 32))) return hipErrorInvalidValue;   // u32 bins
  if ((path == 1 && bands > 1) || (path == 2 && bands > QUANTILE_BAND_LIMIT)) return hipErrorInvalidValue;
  if (path < 0) path = quantile_path(a.N, lists, a.pass);
  if (path > 0) {
    fold_lds_optin<quantile_hist_lds_kernel>();
    if (a.agg < 0) a.agg = QUANTILE_LDS_AGG_ROUNDS;
    // one workgroup per CU over all bands
    const int64_t most = FOLD_LDS_BLOCKS / bands > 0 ? FOLD_LDS_BLOCKS / bands : 1;
    const unsigned nb = fold_grid(a.N, FOLD_LDS_THREADS, FOLD_LDS_ROWS, most);
    const int64_t held = lists < QUANTILE_LDS_MAX_LISTS ? lists : QUANTILE_LDS_MAX_LISTS;
    const size_t bytes = (size_t)held * QUANTILE_BINS * sizeof(unsigned);
    hipLaunchKernelGGL(quantile_hist_lds_kernel, dim3(nb, (unsigned)bands), dim3(FOLD_LDS_THREADS), bytes, s, a);
    return hipGetLastError();
  }
  if (a.agg < 0) a.agg = QUANTILE_AGG_ROUNDS;
  const unsigned nb = fold_grid(a.N, FOLD_THREADS, 1, FOLD_MAX_BLOCKS);
  hipLaunchKernelGGL(quantile_hist_kernel, dim3(nb), dim3(FOLD_THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_quantile_select(const QuantileSelectArgs& a, hipStream_t s) {
  if (a.K <= 0) return hipSuccess;
  if (a.Q < 1 || a.Q > QUANTILE_MAX_Q || a.pass < 0 || a.pass >= QUANTILE_PASSES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(quantile_select_kernel, dim3((unsigned)a.K), dim3(QUANTILE_BINS), 0, s, a);
  return hipGetLastError();
}

}  // namespace mk
