// mikmeans — deep search (ClusterIndex.search_deep), for gfx950: the m-th smallest squared distance
// of every query over the rows of its probed lists, found without keeping a candidate, so that m
// is not bound by a register list (the scan of csrc/ivf.hip ends at TOPK_MAX = 32).
//
// A most-significant-digit radix select over bits(d2), as csrc/quantiles.hip selects a cluster's
// quantiles: up to four passes of 8-bit digits at shift s = 24, 16, 8, 0, each a histogram and a
// select.  The bits fixed so far (every lower bit set) are a radius for the range passes of
// csrc/range.hip, which collect the rows under it; the ops layer stops as soon as that radius
// lets few enough rows through (mikmeans/ops/index.py index_search_deep).
//
// 1. Histogram (ivf_hist_kernel) on the frame of ivf_range_kernel: the walk's work item, load_row
//    and tile_d2 called as the count pass calls them -- d2 is bitwise the fill's, and the method is
//    only exact because it is.  A row k < list length of a live pair counts in bin bits >> 24
//    (pass 0) or, where its bits above s + 8 are the query's prefix's, in bin (bits >> s) & 255.
//    No finiteness filter: clamp_d2 leaves +0 .. +inf or the one NaN pattern, top byte <= 0x7f.
//
//    Same-address contention is the design problem (the header of quantiles.hip): in pass 0
//    nearly every row of a query shares one to three bins, and a no-return global atomic costs a
//    CU about 50 ns a wave-instruction, so a global add per row is out.  Every wave keeps a
//    private table in LDS, one row of 256 bins per pair of its item: it zeroes it, adds with LDS
//    atomics and flushes the non-zero bins with global integer adds (pairs of one query run in
//    different waves, so the flush stays atomic).  Only the wave's own fences: no workgroup
//    barrier.  Integer sums are associative: every form gives the same table.
//
//    What the form is picked for is occupancy, not contention (docs/SEARCH_DEEP.md has the
//    numbers): the walk waits on memory, and the LDS a workgroup takes decides how many waves a
//    CU holds.  So a bin is 16 bits, two to a u32 word ([16 P][128] words, 8 KiB a pair block):
//    ds_add_u32 of 1 or 1 << 16, and the table is flushed and zeroed again every HIST_CHUNK tiles
//    (65520 rows), before a half-word could carry into its neighbour.  And a wave takes one pair
//    block (HIST_BLOCKS = 1): 32 KiB a workgroup, five workgroups a CU.  With u32 bins (64 KiB,
//    two workgroups a CU) a pass cost 1.6 times as much, with two or four pair blocks a wave
//    1.2 and 1.9 times.  Row `slot` is rotated by `slot` words: the sixteen queries of a block
//    mostly share a digit, and unrotated that digit is one LDS bank for all of them.
// 2. Select (ivf_select_kernel): one workgroup a query, one thread a bin, the running count of
//    bins.h (shared with quantile_select_kernel); kernels.h IvfSelectArgs has the rule.
#include "bins.h"
#include "dispatch.h"
#include "topk.h"

namespace mk {

constexpr int HIST_BLOCKS = 1;                  // pair blocks per wave (see the header)
constexpr int HIST_WORDS = QUANTILE_BINS / 2;   // two 16-bit bins a word
constexpr int HIST_CHUNK = 4095;                // tiles between flushes: 65520 rows, a half-word cannot carry
constexpr int hist_lds_bytes(int P) { return TK_NW * P * 16 * HIST_WORDS * 4; }
static_assert(hist_lds_bytes(HIST_BLOCKS) <= FOLD_LDS_BYTES, "the wave tables must fit a workgroup's LDS");

// What one wave wrote to its LDS table is what it reads next (no other wave touches the table)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T, int DPAD, int P>
__global__ __launch_bounds__(TK_NW * 64, 2) void ivf_hist_kernel(IvfHistArgs a) {
  constexpr int V = Elem<T>::V;
  constexpr int NQ = DPAD / 4 / V;
  constexpr bool XREG = range_xreg(NQ);
  constexpr int B = QUANTILE_BINS, W = HIST_WORDS;
  extern __shared__ __attribute__((aligned(16))) char hist_lds[];   // [TK_NW][16 P][128] u32
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t item = (int64_t)blockIdx.x * TK_NW + wid;
  if (item >= a.w.icum[a.w.K]) return;   // (wave-uniform; the kernel has no workgroup barrier)
  const WalkItem it = walk_item<P * 16>(a.w.icum, a.w.poff, a.w.offsets, a.w.K, item);
  const int nl = it.nl;
  uint32_t* tw = reinterpret_cast<uint32_t*>(hist_lds) + wid * (P * 16 * W);
  const int s = 24 - 8 * a.pass;
  const uint32_t mask = a.pass ? ~0u << (s + 8) : 0u;   // the bits a row must share with its query's prefix
  u32x4 xr[P][XREG ? NQ : 1];
  const T* xp[P];
  float xn[P];
  uint32_t pfx[P];
  bool live[P];   // (the clamped duplicates past np count nothing)
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int slot = p * 16 + r;
    live[p] = slot < it.np;
    const int64_t pid = a.w.porder[it.p0 + (live[p] ? slot : it.np - 1)];
    const int64_t q = pid / a.w.nprobe;
    load_row<T, NQ, XREG>(a.w.Q, a.w.ldq, q, a.w.qn, g, a.w.D, xr[p], xp[p], xn[p]);
    pfx[p] = a.pass ? (uint32_t)a.prefix[q] : 0u;
  }
  const int64_t t0 = a.w.toff[it.list];
  const T* pack = (const T*)a.w.pack + t0 * (NQ * 64 * V);
  const float* cn = a.w.cn + t0 * 16;
  const int nt = (nl + 15) / 16;
  for (int tc = 0; tc < nt; tc += HIST_CHUNK) {
    const int te = tc + HIST_CHUNK < nt ? tc + HIST_CHUNK : nt;
    for (int i = lane; i < P * 16 * W / 4; i += 64) reinterpret_cast<u32x4*>(tw)[i] = u32x4{0u, 0u, 0u, 0u};
    wave_lds_sync();
    for (int t = tc; t < te; ++t) {
      f32x4 d2[P];
      tile_d2<T, NQ, P, XREG>(pack, cn, t, lane, g, xr, xp, a.w.D, xn, d2);
      const int k0 = t * 16 + 4 * g;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int slot = p * 16 + r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t bits = __float_as_uint(d2[p][e]);
          const uint32_t digit = (bits >> s) & 255u;
          if (live[p] && k0 + e < nl && ((bits ^ pfx[p]) & mask) == 0u)
            atomicAdd(tw + slot * W + (((digit >> 1) + slot) & (W - 1)), 1u << (16 * (digit & 1u)));
        }
      }
    }
    wave_lds_sync();
    // the flush: pair after pair, a lane two words (four bins) of the pair's row
    for (int slot = 0; slot < it.np; ++slot) {
      const int64_t q = a.w.porder[it.p0 + slot] / a.w.nprobe;
      const uint2 v = reinterpret_cast<const uint2*>(tw)[slot * (W / 2) + lane];
      const uint32_t w0 = (uint32_t)(2 * lane - slot) & (W - 1), w1 = (uint32_t)(2 * lane + 1 - slot) & (W - 1);
      uint32_t* tq = a.table + q * B;
      if (v.x & 0xffffu) atomicAdd(tq + 2 * w0, v.x & 0xffffu);
      if (v.x >> 16) atomicAdd(tq + 2 * w0 + 1, v.x >> 16);
      if (v.y & 0xffffu) atomicAdd(tq + 2 * w1, v.y & 0xffffu);
      if (v.y >> 16) atomicAdd(tq + 2 * w1 + 1, v.y >> 16);
    }
    wave_lds_sync();   // (the next chunk's zeros come after the flush's reads)
  }
}

template <typename T, int DPAD, int P>
static hipError_t launch_ih_p(int64_t nb, const IvfHistArgs& a, hipStream_t s) {
  fold_lds_optin<ivf_hist_kernel<T, DPAD, P>>();
  hipLaunchKernelGGL((ivf_hist_kernel<T, DPAD, P>), dim3((unsigned)nb), dim3(TK_NW * 64), hist_lds_bytes(P), s, a);
  return hipGetLastError();
}

template <typename T, int DPAD>
static hipError_t launch_ih(int P, int64_t nb, const IvfHistArgs& a, hipStream_t s) {
  if (P == HIST_BLOCKS) return launch_ih_p<T, DPAD, HIST_BLOCKS>(nb, a, s);
  return hipErrorInvalidValue;
}

// Pair blocks per wave: one for every width and every batch (see the header)
int ivf_hist_blocks(int, int, int64_t npairs) { return walk_blocks(HIST_BLOCKS, npairs); }

hipError_t launch_ivf_hist(int dtype, int dpad, int P, const IvfHistArgs& a, hipStream_t s) {
  int64_t nb;
  if (const hipError_t e = ivf_walk_grid(a.w, dpad, nb); e != hipSuccess || nb == 0) return e;
  if (a.pass < 0 || a.pass >= QUANTILE_PASSES || !a.table || (a.pass > 0 && !a.prefix)) return hipErrorInvalidValue;
  return (hipError_t)for_width(dtype, dpad, [&](auto t, auto w) {
    return launch_ih<typename decltype(t)::type, decltype(w)::value>(P, nb, a, s);
  });
}

// One workgroup per query, one thread per bin: the running count over the bins, then the bin that
// holds rank R
__global__ __launch_bounds__(QUANTILE_BINS) void ivf_select_kernel(IvfSelectArgs a) {
  __shared__ unsigned long long wsum[QUANTILE_BINS / 64];
  const int64_t q = blockIdx.x;
  const int b = threadIdx.x;
  const int s = 24 - 8 * a.pass;
  // (every thread reads the query's rank and cand before the barriers below, the writers write after)
  const int64_t rank = a.pass ? a.rank[q] : 0, cand0 = a.pass ? a.cand[q] : 0;
  const unsigned long long c = a.table[q * QUANTILE_BINS + b];
  unsigned long long incl, total;
  bins_running_count(c, wsum, incl, total);
  const int64_t cand = a.pass ? cand0 : (int64_t)total;
  const int64_t found = cand < a.m ? cand : a.m;
  const int64_t R = a.pass ? rank : found - 1;
  if (a.pass == 0 && b == 0) {
    a.cand[q] = cand;
    if (cand == 0) {
      a.prefix[q] = 0;
      a.rank[q] = 0;
      a.hits[q] = 0;
    }
  }
  const int64_t excl = (int64_t)(incl - c);
  if ((int64_t)incl > R && excl <= R) {   // at most one bin (none where cand = 0)
    a.prefix[q] = (a.pass ? a.prefix[q] : 0) | (int32_t)((unsigned)b << s);
    a.rank[q] = R - excl;
    a.hits[q] = found - 1 - (R - excl) + (int64_t)c;
  }
}

hipError_t launch_ivf_select(const IvfSelectArgs& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  if (a.nq > 0x7fffffff || a.m < 1 || a.m > IVF_DEEP_MAX_M || a.pass < 0 || a.pass >= QUANTILE_PASSES)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ivf_select_kernel, dim3((unsigned)a.nq), dim3(QUANTILE_BINS), 0, s, a);
  return hipGetLastError();
}

}  // namespace mk
