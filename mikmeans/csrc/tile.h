// mikmeans — the 16x16 MFMA tile every distance kernel multiplies on: the k-step (csrc/assign16.hip
// takes only this), the row-piece load and the tile step of the kernels that walk the
// fragment-packed centres straight from L2 (csrc/transform.hip, csrc/topk.hip, csrc/ivf.hip).
// Those three give bitwise the same squared distance for the same (row, centre) because this
// is the one place that seeds, multiplies and clamps it.
#pragma once
#include "common.h"

namespace mk {

// One k-step of 16 B per lane: 32 bf16 features in one MFMA, 16 f32 features in four
template <typename T> struct Mfma16;
template <> struct Mfma16<uint16_t> {
  __device__ static __forceinline__ f32x4 run(const u32x4& a, const u32x4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(short8, a),
                                                   __builtin_bit_cast(short8, b), c, 0, 0, 0);
  }
};
template <> struct Mfma16<float> {
  __device__ static __forceinline__ f32x4 run(const u32x4& a, const u32x4& b, f32x4 c) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[e]), __uint_as_float(b[e]), c, 0, 0, 0);
    return c;
  }
};

// Piece q of a row for lane group g (rp = the row + g V; features [(4q + g)V, +V)); zero past
// the row's D columns
template <int V, typename T>
__device__ __forceinline__ u32x4 load_piece(const T* rp, int q, int g, int D) {
  return (4 * q + g) * V < D ? *(const u32x4*)(rp + 4 * q * V) : u32x4{0u, 0u, 0u, 0u};
}

// A lane's share of row `row` of X (leading dimension ld): xp = the row + g V, its fragments
// where they stay in registers (XREG), and its |x|^2
template <typename T, int NQ, bool XREG>
__device__ __forceinline__ void load_row(const void* X, int64_t ld, int64_t row, const float* norms, int g, int D,
                                         u32x4 (&xr)[XREG ? NQ : 1], const T*& xp, float& xn) {
  constexpr int V = Elem<T>::V;
  xp = (const T*)X + row * ld + g * V;
  if constexpr (XREG) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) xr[q] = load_piece<V>(xp, q, g, D);
  }
  xn = norms[row];
}

// Tile t (16 packed rows from `pack`, their |c|^2 from `cn`) against a wave's P blocks of 16
// rows: lane (r = lane & 15, g = lane >> 4) is left with d2[p][e] = clamp_d2(|x|^2 + |c|^2 -
// 2 x.c) (common.h) of row r of block p against packed row 16t + 4g + e.  The accumulators are
// seeded with |c|^2, the NQ A-fragments multiply the blocks in q-major order and xn goes on
// last.  The rows' fragments are xr (XREG) or fetched again through xp = the row + g V (L1 / L2
// hits: the rows no longer fit the registers).
template <typename T, int NQ, int P, bool XREG>
__device__ __forceinline__ void tile_d2(const T* pack, const float* cn, int t, int lane, int g,
                                        const u32x4 (&xr)[P][XREG ? NQ : 1], const T* const (&xp)[P], int D,
                                        const float (&xn)[P], f32x4 (&d2)[P]) {
  constexpr int V = Elem<T>::V;
  const f32x4 ci = *(const f32x4*)(cn + t * 16 + 4 * g);
#pragma unroll
  for (int p = 0; p < P; ++p) d2[p] = ci;
  const T* tp = pack + ((int64_t)t * NQ * 64 + lane) * V;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const u32x4 aq = *(const u32x4*)(tp + (int64_t)q * 64 * V);
#pragma unroll
    for (int p = 0; p < P; ++p)
      d2[p] = Mfma16<T>::run(aq, XREG ? xr[p][q] : load_piece<V>(xp[p], q, g, D), d2[p]);
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int e = 0; e < 4; ++e) d2[p][e] = clamp_d2(xn[p] + d2[p][e]);
  }
}

}  // namespace mk
