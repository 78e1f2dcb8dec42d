// mikmeans — distances of every row to every centre (KMeans.transform) on the MFMA tiles.
//
// out[i, k] = sqrt(clamp_d2(|x_i|^2 + |c_k|^2 - 2 x_i.c_k)), written as f32 [N, K]: a negative
// sum becomes +0, a NaN or +inf one stays (common.h), so a row or centre with a NaN or infinite
// coordinate gives NaN or inf distances, never 0.  The same
// fragment-packed centres the assign kernel reads (csrc/kernels.h layout "16": -2c in the
// points' dtype, |c_q|^2 of the quantised centres in f32), so a fitted model's serving pack
// is reused and the distances are those the assign's argmin ranked: bf16 rows against
// bf16-quantised centres with f32 accumulation, f32 rows on the exact f32 MFMA.
//
// Each wave keeps P blocks of 16 rows in registers (as the assign) and walks the centre
// tiles straight from L2 (the pack is at most Kpad x 1024 x 4 B and every wave reads it in
// the same order).  Lane (r = l & 15, g = l >> 4) ends a tile with the 4 scores of row r
// against centres 16t + 4g + {0..3}: one 16-B store per lane and tile, so the [N, K] output
// -- the bound for any K >= 16 -- streams out as 64-B row segments.
// The distance itself comes out of the tile step of csrc/tile.h, which csrc/topk.hip and
// csrc/ivf.hip run too: their d2 is bitwise this kernel's.
#include "dispatch.h"
#include "kernels.h"
#include "tile.h"

namespace mk {

constexpr int TR_NW = 4;   // waves per workgroup

template <typename T, int DPAD, int P>
__global__ __launch_bounds__(TR_NW * 64) void transform_kernel(TransformArgs a) {
  constexpr int V = Elem<T>::V;
  constexpr int NQ = DPAD / 4 / V;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t pbase = ((int64_t)blockIdx.x * TR_NW + wid) * (P * 16);
  if (pbase >= a.N) return;   // (wave-uniform; no barrier below)
  u32x4 xr[P][NQ];
  const T* xp[P];
  float xn[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int64_t row = pbase + p * 16 + r;
    load_row<T, NQ, true>(a.X, a.ldx, row < a.N ? row : a.N - 1, a.xn, g, a.D, xr[p], xp[p], xn[p]);
  }
  const T* pack = (const T*)a.pack;
  const int ntile = a.Kpad / 16;
  for (int t = 0; t < ntile; ++t) {
    f32x4 d2[P];
    tile_d2<T, NQ, P, true>(pack, a.cn, t, lane, g, xr, xp, a.D, xn, d2);
    const int k0 = t * 16 + 4 * g;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int64_t row = pbase + p * 16 + r;
      if (row >= a.N) continue;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = a.squared ? d2[p][e] : __builtin_sqrtf(d2[p][e]);
      float* o = a.out + row * a.ldo + k0;
      if (k0 + 3 < a.K && (a.ldo & 3) == 0) {
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k0 + e < a.K) o[e] = v[e];
      }
    }
  }
}

template <typename T, int DPAD>
static hipError_t launch_tr(const TransformArgs& a, hipStream_t s) {
  constexpr int NQ = DPAD / 4 / Elem<T>::V;
  // rows in registers: at most 32 16-B pieces per lane (128 VGPRs), at most 8 blocks
  constexpr int P = NQ >= 32 ? 1 : (32 / NQ > 8 ? 8 : 32 / NQ);
  const int64_t per_wg = (int64_t)TR_NW * P * 16;
  const int64_t nb = (a.N + per_wg - 1) / per_wg;
  hipLaunchKernelGGL((transform_kernel<T, DPAD, P>), dim3((unsigned)nb), dim3(TR_NW * 64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_transform(int dtype, int dpad, const TransformArgs& a, hipStream_t s) {
  if (a.N <= 0 || a.K <= 0) return hipSuccess;
  if (a.Kpad % 16 || a.Kpad < a.K || a.D > dpad) return hipErrorInvalidValue;
  return (hipError_t)for_width(dtype, dpad, [&](auto t, auto w) {
    return launch_tr<typename decltype(t)::type, decltype(w)::value>(a, s);
  });
}

}  // namespace mk
