// mikmeans — the m nearest centres of every row (predict_topk) on the MFMA tiles.
//
// dist[i, j], idx[i, j] = the j-th smallest pair (d2[i, k], k) over the K centres, where
// d2[i, k] = clamp_d2(|x_i|^2 + |c_k|^2 - 2 x_i.c_k) (common.h: negatives to +0, NaN kept) is
// bitwise the squared distance the transform kernel stores (csrc/transform.hip: the same
// fragment pack, the same cn seeds and the same MFMA k-step order), so equal distances go to
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
#include "topk.h"   // the MFMA step, the list insertion and the merge (shared with csrc/ivf.hip)

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
    int64_t row = pbase + p * 16 + r;
    row = row < a.N ? row : a.N - 1;
    xp[p] = (const T*)a.X + row * a.ldx + g * V;
    if constexpr (XREG) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) xr[p][q] = load_piece<V>(xp[p], q, g, a.D);
    }
    xn[p] = a.xn[row];
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
  const T* pack = (const T*)a.pack;
  const int ntile = (a.K + 15) / 16;   // (the pad tiles up to Kpad hold no centre)
  for (int t = 0; t < ntile; ++t) {
    const f32x4 ci = *(const f32x4*)(a.cn + t * 16 + 4 * g);
    f32x4 acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = ci;
    const T* tp = pack + ((int64_t)t * NQ * 64 + lane) * V;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const u32x4 aq = *(const u32x4*)(tp + (int64_t)q * 64 * V);
#pragma unroll
      for (int p = 0; p < P; ++p)
        acc[p] = KMfma<T>::run(aq, XREG ? xr[p][q] : load_piece<V>(xp[p], q, g, a.D), acc[p]);
    }
    const int k0 = t * 16 + 4 * g;
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d2 = clamp_d2(xn[p] + acc[p][e]);
        // a pad centre (k >= K) is an empty candidate: the strict compare never takes it
        const uint32_t c = k0 + e < a.K ? __float_as_uint(d2) : TK_EMPTY;
        const int ck = k0 + e;
        if (__builtin_amdgcn_ballot_w64(c < bv[p][M - 1]) == 0) continue;
        tk_insert<M>(bv[p], bi[p], c, ck);
      }
    }
  }
  // merge the row's four lists: keys to LDS as [slot][lane] (conflict-free), lane r reads
  MK_LDS unsigned long long* ws = (MK_LDS unsigned long long*)sm + wid * (M * 64);
#pragma unroll
  for (int p = 0; p < P; ++p) {
    tk_stage<M>(ws, lane, bv[p], bi[p]);
    const int64_t row = pbase + p * 16 + r;
    if (g == 0 && row < a.N) {
      float* od = a.dist + row * a.m;
      int32_t* oi = a.idx + row * a.m;
      tk_merge4<M>(ws, r, a.m, [&](int j, unsigned long long best) {
        od[j] = __uint_as_float((uint32_t)(best >> 32));
        oi[j] = (int32_t)(uint32_t)best;
      });
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the next block's keys overwrite the slab
  }
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
  // a small batch takes one block per wave, so more waves share the work (under ~2 waves
  // per SIMD of a 256-CU part otherwise)
  if (P > 1 && a.N < (int64_t)32768 * P) return launch_tk_p<T, DPAD, 1, M>(a, s);
  return launch_tk_p<T, DPAD, P, M>(a, s);
}

template <typename T, int DPAD>
static hipError_t launch_tk(const TopkArgs& a, hipStream_t s) {
  return a.m <= 8 ? launch_tk_m<T, DPAD, 8>(a, s) : launch_tk_m<T, DPAD, 32>(a, s);
}

hipError_t launch_topk(int dtype, int dpad, const TopkArgs& a, hipStream_t s) {
  if (a.N <= 0) return hipSuccess;
  if (a.K <= 0 || a.m < 1 || a.m > TOPK_MAX || a.m > a.K) return hipErrorInvalidValue;
  if (a.Kpad % 16 || a.Kpad < a.K || a.D > dpad) return hipErrorInvalidValue;
  if (dtype == DT_BF16) {
    switch (dpad) {
      case 32: return launch_tk<uint16_t, 32>(a, s);
      case 64: return launch_tk<uint16_t, 64>(a, s);
      case 128: return launch_tk<uint16_t, 128>(a, s);
      case 256: return launch_tk<uint16_t, 256>(a, s);
      case 384: return launch_tk<uint16_t, 384>(a, s);
      case 512: return launch_tk<uint16_t, 512>(a, s);
      case 768: return launch_tk<uint16_t, 768>(a, s);
      case 1024: return launch_tk<uint16_t, 1024>(a, s);
    }
  } else {
    switch (dpad) {
      case 16: return launch_tk<float, 16>(a, s);
      case 32: return launch_tk<float, 32>(a, s);
      case 64: return launch_tk<float, 64>(a, s);
      case 128: return launch_tk<float, 128>(a, s);
      case 256: return launch_tk<float, 256>(a, s);
      case 384: return launch_tk<float, 384>(a, s);
      case 512: return launch_tk<float, 512>(a, s);
      case 768: return launch_tk<float, 768>(a, s);
      case 1024: return launch_tk<float, 1024>(a, s);
    }
  }
  return hipErrorInvalidValue;
}

}  // namespace mk
