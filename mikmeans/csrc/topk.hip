// mikmeans — the m nearest centres of every row (predict_topk) on the MFMA tiles.
//
// dist[i, j], idx[i, j] = the j-th smallest pair (d2[i, k], k) over the K centres, where
// d2[i, k] = clamp_d2(|x_i|^2 + |c_k|^2 - 2 x_i.c_k) (common.h: negatives to +0, NaN kept) is
// bitwise the squared distance the transform kernel stores (both come out of the one tile step
// of csrc/tile.h, over the same fragment pack), so equal distances go to
// the lower centre index and the answer is transform(squared) + a stable sort without the
// [N, K] matrix ever reaching memory.  A row or centre with a NaN or infinite coordinate gives
// inf or NaN distances, never 0; they sort behind every finite one (inf, then NaN).
//
// Each wave keeps P blocks of 16 rows in registers and walks the centre tiles as the
// transform does.  Lane (r = l & 15, g = l >> 4) ends tile t with the 4 scores of row r against
// centres 16t + 4g + {0..3}; instead of storing them it keeps, per row block, a sorted list of
// its M best (d2 bits, k) in registers: a fully unrolled insertion (static indexing, so the
// lists never move to scratch), skipped whenever no lane of the wave has a candidate under its
// current M-th best.  d2 is >= +0 or the one NaN pattern of clamp_d2, so its bit pattern orders
// as an unsigned integer and the all-ones pattern marks an empty slot (distances of +inf and
// NaN still sort in front of it, so every one of the K centres is a candidate).  A
// lane meets its centres in ascending order and a candidate goes behind every entry it does
// not beat strictly, so ties keep the lower index.  After the last tile the four lists of a row (lanes r, r + 16,
// r + 32, r + 48) go through LDS as (d2 bits << 32 | k) keys and lane r merges them in a
// rolled loop -- once per wave and row block, so its speed matters little -- writing the
// row's first m winners.
#include "dispatch.h"
#include "topk.h"   // the candidate loop and the merge (shared with csrc/ivf.hip)

namespace mk {

template <typename T, int DPAD, int P, int M>
__global__ __launch_bounds__(TK_NW * 64, 2) void topk_kernel(TopkArgs a) {
  constexpr int V = Elem<T>::V;
  constexpr int NQ = DPAD / 4 / V;
  constexpr bool XREG = topk_xreg(NQ, M);
  __shared__ unsigned long long sm[TK_NW * M * 64];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t pbase = ((int64_t)blockIdx.x * TK_NW + wid) * (P * 16);
  if (pbase >= a.N) return;   // (wave-uniform; the kernel has no workgroup barrier)
  u32x4 xr[P][XREG ? NQ : 1];
  const T* xp[P];
  float xn[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int64_t row = pbase + p * 16 + r;
    load_row<T, NQ, XREG>(a.X, a.ldx, row < a.N ? row : a.N - 1, a.xn, g, a.D, xr[p], xp[p], xn[p]);
  }
  uint32_t bv[P][M];
  int bi[P][M];
#pragma unroll
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      bv[p][j] = TK_EMPTY;
      bi[p][j] = TK_NOIDX;
    }
  }
  // (the pad tiles up to Kpad hold no centre)
  tk_scan<T, NQ, P, M, XREG>((const T*)a.pack, a.cn, 0, (a.K + 15) / 16, a.K, lane, g, xr, xp, a.D, xn, bv, bi);
  const int64_t left = a.N - pbase;
  MK_LDS unsigned long long* ws = (MK_LDS unsigned long long*)sm + wid * (M * 64);
  tk_merge_rows(ws, lane, (int)(left < P * 16 ? left : P * 16), a.m, bv, bi, [&](int p) {
    float* od = a.dist + (pbase + p * 16 + r) * a.m;
    int32_t* oi = a.idx + (pbase + p * 16 + r) * a.m;
    return [=](int j, unsigned long long best) {
      od[j] = __uint_as_float((uint32_t)(best >> 32));
      oi[j] = (int32_t)(uint32_t)best;
    };
  });
}

template <typename T, int DPAD, int P, int M>
static hipError_t launch_tk_p(const TopkArgs& a, hipStream_t s) {
  const int64_t per_wg = (int64_t)TK_NW * P * 16;
  const int64_t nb = (a.N + per_wg - 1) / per_wg;
  hipLaunchKernelGGL((topk_kernel<T, DPAD, P, M>), dim3((unsigned)nb), dim3(TK_NW * 64), 0, s, a);
  return hipGetLastError();
}

template <typename T, int DPAD, int M>
static hipError_t launch_tk_m(const TopkArgs& a, hipStream_t s) {
  constexpr int P = topk_blocks(DPAD / 4 / Elem<T>::V, M);
  // (a small batch takes one block per wave: walk.h)
  return walk_blocks(P, a.N) == 1 ? launch_tk_p<T, DPAD, 1, M>(a, s) : launch_tk_p<T, DPAD, P, M>(a, s);
}

template <typename T, int DPAD>
static hipError_t launch_tk(const TopkArgs& a, hipStream_t s) {
  return a.m <= 8 ? launch_tk_m<T, DPAD, 8>(a, s) : launch_tk_m<T, DPAD, 32>(a, s);
}

hipError_t launch_topk(int dtype, int dpad, const TopkArgs& a, hipStream_t s) {
  if (a.N <= 0) return hipSuccess;
  if (a.K <= 0 || a.m < 1 || a.m > TOPK_MAX || a.m > a.K) return hipErrorInvalidValue;
  if (a.Kpad % 16 || a.Kpad < a.K || a.D > dpad) return hipErrorInvalidValue;
  return (hipError_t)for_width(dtype, dpad, [&](auto t, auto w) {
    return launch_tk<typename decltype(t)::type, decltype(w)::value>(a, s);
  });
}

}  // namespace mk
