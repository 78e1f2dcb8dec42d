// mikmeans — range search through the clusters (ClusterIndex.range_search / range_count), for
// gfx950: every indexed row within a radius of each query, over the lists of the query's probed
// centres.
//
// The work item (csrc/walk.h), the row pack and the tile step are the scan's (csrc/ivf.hip): a wave
// holds the queries of its item's pairs as load_row gives them and walks the list's tiles with
// tile_d2 -- so d2 is bitwise the scan's and the transform kernel's value for (query, row).  What
// differs is what is kept: no candidate list, so the result has no fixed length and is written in
// two passes with a host-side cumulative sum between them.
//
// 1. Count: a lane counts the tile entries with k < list length and bits(d2) <= bits(r2[query])
//    (d2 is clamped to +0 .. +inf or the one NaN pattern, r2 is finite and non-negative: the
//    unsigned compare of the bit patterns is the float compare, and a NaN is above every radius);
//    a query's four lanes are summed and lane r < 16 writes counts[pair id].  Pair ids are unique
//    to an item: no atomics.
// 2. Fill: the same walk -- the same arithmetic, hence the same decisions -- writes the keys
//    (d2 bits << 32 | row) of pair p at base[p] + rank, rank = the hit's position within its pair
//    in list order: the pair's running count (kept equal in its four lanes), plus the hits of the
//    lower lane groups in this tile (an inclusive scan over the groups by lane shuffles), plus the
//    lower entries of the own lane.  As in ivf.hip no position depends on an atomic's return
//    order: the key buffer is bitwise the same on every launch.  A tile's ranking is skipped
//    where no lane of the wave has a hit.  No LDS, no workgroup barrier.
//
// A long list is not split over waves.
#include "dispatch.h"
#include "topk.h"

namespace mk {

template <typename T, int DPAD, int P, bool FILL>
__global__ __launch_bounds__(TK_NW * 64, 2) void ivf_range_kernel(IvfRangeArgs a) {
  constexpr int V = Elem<T>::V;
  constexpr int NQ = DPAD / 4 / V;
  constexpr bool XREG = range_xreg(NQ);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t item = (int64_t)blockIdx.x * TK_NW + wid;
  if (item >= a.w.icum[a.w.K]) return;   // (wave-uniform; the kernel has no workgroup barrier)
  const WalkItem it = walk_item<P * 16>(a.w.icum, a.w.poff, a.w.offsets, a.w.K, item);
  const int nl = it.nl;
  u32x4 xr[P][XREG ? NQ : 1];
  const T* xp[P];
  float xn[P];
  int64_t pid[P], base[P];
  uint32_t rb[P], run[P];
  bool live[P];   // (the clamped duplicates past np count and write nothing)
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int slot = p * 16 + r;
    live[p] = slot < it.np;
    pid[p] = a.w.porder[it.p0 + (live[p] ? slot : it.np - 1)];
    const int64_t q = pid[p] / a.w.nprobe;
    load_row<T, NQ, XREG>(a.w.Q, a.w.ldq, q, a.w.qn, g, a.w.D, xr[p], xp[p], xn[p]);
    rb[p] = __float_as_uint(a.r2[q]);
    run[p] = 0u;
    base[p] = FILL ? a.base[pid[p]] : 0;
  }
  const int64_t t0 = a.w.toff[it.list];
  const T* pack = (const T*)a.w.pack + t0 * (NQ * 64 * V);
  const float* cn = a.w.cn + t0 * 16;
  const int64_t* ord = a.w.order + it.o0;
  const int nt = (nl + 15) / 16;
  for (int t = 0; t < nt; ++t) {
    f32x4 d2[P];
    tile_d2<T, NQ, P, XREG>(pack, cn, t, lane, g, xr, xp, a.w.D, xn, d2);
    const int k0 = t * 16 + 4 * g;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      uint32_t h = 0u;   // bit e: packed row k0 + e is a hit of the lane's query
#pragma unroll
      for (int e = 0; e < 4; ++e)
        h |= (live[p] && k0 + e < nl && __float_as_uint(d2[p][e]) <= rb[p]) ? (1u << e) : 0u;
      const uint32_t c = (uint32_t)__builtin_popcount(h);
      if constexpr (!FILL) {
        run[p] += c;
      } else {
        if (__builtin_amdgcn_ballot_w64(h != 0u) == 0) continue;
        uint32_t incl = c;   // the hits of lane groups 0 .. g of the query in this tile
        uint32_t u = __shfl_up(incl, 16, 64);
        if (g >= 1) incl += u;
        u = __shfl_up(incl, 32, 64);
        if (g >= 2) incl += u;
        const uint32_t all = __shfl(incl, 48 + r, 64);
        int64_t w = base[p] + run[p] + (incl - c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if ((h >> e) & 1u) {
            if (w < a.total)   // (the count pass's total; never false while the passes agree)
              a.keys[w] = (long long)(((unsigned long long)__float_as_uint(d2[p][e]) << 32) | (uint32_t)ord[k0 + e]);
            ++w;
          }
        }
        run[p] += all;
      }
    }
  }
  if constexpr (!FILL) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      uint32_t c = run[p];
      c += __shfl_xor(c, 16, 64);
      c += __shfl_xor(c, 32, 64);
      if (lane < 16 && live[p]) a.counts[pid[p]] = (int64_t)c;
    }
  }
}

template <typename T, int DPAD, int P>
static hipError_t launch_ir_p(bool fill, int64_t nb, const IvfRangeArgs& a, hipStream_t s) {
  if (fill) hipLaunchKernelGGL((ivf_range_kernel<T, DPAD, P, true>), dim3((unsigned)nb), dim3(TK_NW * 64), 0, s, a);
  else hipLaunchKernelGGL((ivf_range_kernel<T, DPAD, P, false>), dim3((unsigned)nb), dim3(TK_NW * 64), 0, s, a);
  return hipGetLastError();
}

template <typename T, int DPAD>
static hipError_t launch_ir(int P, bool fill, int64_t nb, const IvfRangeArgs& a, hipStream_t s) {
  constexpr int PF = range_blocks(DPAD / 4 / Elem<T>::V);
  if (P == 1) return launch_ir_p<T, DPAD, 1>(fill, nb, a, s);
  if (P == PF) return launch_ir_p<T, DPAD, PF>(fill, nb, a, s);
  return hipErrorInvalidValue;
}

// Pair blocks per wave: range_blocks, then walk_blocks over the pairs (the scan's rule)
int ivf_range_blocks(int dtype, int dpad, int64_t npairs) {
  return walk_blocks(range_blocks(dpad / 4 / (dtype == DT_BF16 ? 8 : 4)), npairs);
}

hipError_t launch_ivf_range(int dtype, int dpad, int P, bool fill, const IvfRangeArgs& a, hipStream_t s) {
  int64_t nb;
  if (const hipError_t e = ivf_walk_grid(a.w, dpad, nb); e != hipSuccess || nb == 0) return e;
  if (fill && a.total <= 0) return hipSuccess;
  if (a.total < 0) return hipErrorInvalidValue;
  return (hipError_t)for_width(dtype, dpad, [&](auto t, auto w) {
    return launch_ir<typename decltype(t)::type, decltype(w)::value>(P, fill, nb, a, s);
  });
}

}  // namespace mk
