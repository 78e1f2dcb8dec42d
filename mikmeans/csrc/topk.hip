// mikmeans — the m nearest centres of every row (predict_topk) on the MFMA tiles.
//
// dist[i, j], idx[i, j] = the j-th smallest pair (d2[i, k], k) over the K centres, where
// d2[i, k] = max(|x_i|^2 + |c_k|^2 - 2 x_i.c_k, 0) is bitwise the squared distance the
// transform kernel stores (csrc/transform.hip: the same fragment pack, the same cn seeds and
// the same MFMA k-step order), so equal distances go to the lower centre index and the answer
// is transform(squared) + a stable sort without the [N, K] matrix ever reaching memory.
//
// Each wave keeps P blocks of 16 rows in registers and walks the centre tiles as the
// transform does.  Lane (r = l & 15, g = l >> 4) ends tile t with the 4 scores of row r against
// centres 16t + 4g + {0..3}; instead of storing them it keeps, per row block, a sorted list of
// its M best (d2 bits, k) in registers: a fully unrolled insertion (static indexing, so the
// lists never move to scratch), skipped whenever no lane of the wave has a candidate under its
// current M-th best.  d2 >= +0, so its bit pattern orders as an unsigned integer and the
// all-ones pattern marks an empty slot (a distance of +inf still sorts in front of it).  A
// lane meets its centres in ascending order and a candidate goes behind every entry it does
// not beat strictly, so ties keep the lower index.  After the last tile the four lists of a row (lanes r, r + 16,
// r + 32, r + 48) go through LDS as (d2 bits << 32 | k) keys and lane r merges them in a
// rolled loop -- once per wave and row block, so its speed matters little -- writing the
// row's first m winners.
#include "common.h"
#include "kernels.h"

namespace mk {

template <typename T> struct KMfma;
template <> struct KMfma<uint16_t> {
  __device__ static __forceinline__ f32x4 run(const u32x4& a, const u32x4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(short8, a), __builtin_bit_cast(short8, b), c,
                                                   0, 0, 0);
  }
};
template <> struct KMfma<float> {
  __device__ static __forceinline__ f32x4 run(const u32x4& a, const u32x4& b, f32x4 c) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[e]), __uint_as_float(b[e]), c, 0, 0, 0);
    return c;
  }
};

constexpr int TK_NW = 4;                    // waves per workgroup
constexpr uint32_t TK_EMPTY = 0xffffffffu;  // list slot without a candidate (above every d2 >= 0)
constexpr int TK_NOIDX = 0x7fffffff;

// Piece q of a row for lane group g (features [(4q + g)V, +V)); zero past the row's D columns
template <int V, typename T>
__device__ __forceinline__ u32x4 load_piece(const T* rp, int q, int g, int D) {
  return (4 * q + g) * V < D ? *(const u32x4*)(rp + 4 * q * V) : u32x4{0u, 0u, 0u, 0u};
}

// Whether a wave's rows stay in registers (4 NQ VGPRs a block) beside the list: the kernel is
// held to the 256 VGPRs of two waves per SIMD, and the M = 32 insertion needs ~140 of them
// (NQ = 32 spilled 20), the M = 8 one ~50.  Past that (f32 D > 768; the long list from bf16
// D > 768 and f32 D > 384) the row fragments are fetched again for every tile (L1 / L2 hits).
constexpr bool topk_xreg(int nq, int m) { return nq <= (m > 8 ? 24 : 48); }

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
        const float d2 = fmaxf(xn[p] + acc[p][e], 0.f);
        // a pad centre (k >= K) is an empty candidate: the strict compare never takes it
        const uint32_t c = k0 + e < a.K ? __float_as_uint(d2) : TK_EMPTY;
        const int ck = k0 + e;
        if (__builtin_amdgcn_ballot_w64(c < bv[p][M - 1]) == 0) continue;
        // slot j takes its left neighbour where c goes in front of both, c itself where it
        // goes in front of slot j only (every compare against c: a displaced entry never
        // passes an equal one, which a compare-and-swap chain of the carried entry would do)
#pragma unroll
        for (int j = M - 1; j > 0; --j) {
          const bool s = c < bv[p][j], sl = c < bv[p][j - 1];
          bv[p][j] = s ? (sl ? bv[p][j - 1] : c) : bv[p][j];
          bi[p][j] = s ? (sl ? bi[p][j - 1] : ck) : bi[p][j];
        }
        const bool s0 = c < bv[p][0];
        bv[p][0] = s0 ? c : bv[p][0];
        bi[p][0] = s0 ? ck : bi[p][0];
      }
    }
  }
  // merge the row's four lists: keys to LDS as [slot][lane] (conflict-free), lane r reads
  MK_LDS unsigned long long* ws = (MK_LDS unsigned long long*)sm + wid * (M * 64);
#pragma unroll
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int j = 0; j < M; ++j) ws[j * 64 + lane] = ((unsigned long long)bv[p][j] << 32) | (uint32_t)bi[p][j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int64_t row = pbase + p * 16 + r;
    if (g == 0 && row < a.N) {
      unsigned long long hk[4];
      int hp[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        hp[q] = 0;
        hk[q] = ws[r + 16 * q];
      }
      float* od = a.dist + row * a.m;
      int32_t* oi = a.idx + row * a.m;
#pragma unroll 1
      for (int j = 0; j < a.m; ++j) {
        unsigned long long best = hk[0];
        int sel = 0;
#pragma unroll
        for (int q = 1; q < 4; ++q) {
          if (hk[q] < best) {
            best = hk[q];
            sel = q;
          }
        }
        od[j] = __uint_as_float((uint32_t)(best >> 32));
        oi[j] = (int32_t)(uint32_t)best;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (sel == q) {
            ++hp[q];
            hk[q] = hp[q] < M ? ws[hp[q] * 64 + r + 16 * q] : ~0ull;
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the next block's keys overwrite the slab
  }
}

// Row blocks per wave: the rows' fragments (4 NQ VGPRs), the list (2 M) and the accumulators
// (4) of every block within ~176 VGPRs, at most 4 blocks -- two waves per SIMD wherever the
// transform kernel has them (tests/test_gpu_topk.py reads the built code object).
constexpr int topk_blocks(int nq, int m) {
  const int p = 176 / (4 * nq + 2 * m + 4);
  return p < 1 ? 1 : (p > 4 ? 4 : p);
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
