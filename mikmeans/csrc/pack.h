// mikmeans — one element into the fragment-packed layout of kernels.h, shared by the centre pack
// (csrc/finalize.hip) and the index's row pack (csrc/ivf.hip), so both store the same bits and
// sum |c_q|^2 in the same order.
#pragma once
#include "common.h"
#include "kernels.h"

namespace mk {

// Packed layout (kernels.h): 16-centroid tiles; piece q of lane r+16g holds features
// [(4q+g)V, (4q+g+1)V).
template <typename T>
__device__ __forceinline__ void store_pack(void* pack, int dpad, int64_t k, int d, float v) {
  constexpr int V = Elem<T>::V;
  const int nq = dpad / (4 * V);
  const int64_t t = k >> 4;
  const int r = (int)(k & 15);
  const int g = (d / V) & 3, q = d / (4 * V);
  const int64_t off = ((t * nq + q) * 64 + r + 16 * g) * V + d % V;
  ((T*)pack)[off] = Elem<T>::from_f32(v);
}

// Feature d of packed row k: stores -2 q and adds q^2 to the lane's share of |c_q|^2 (a lane
// takes the features part, part + 8, ... in turn; the row's eight lanes are then summed by the
// xor butterfly 1, 2, 4).  q is the quantised value (bf16-rounded for bf16 points).
__device__ __forceinline__ void pack_elem(int dtype, void* pack, int dpad, int64_t k, int d, float q, float& cn) {
  cn += q * q;
  if (dtype == DT_BF16) store_pack<uint16_t>(pack, dpad, k, d, -2.f * q);
  else store_pack<float>(pack, dpad, k, d, -2.f * q);
}

}  // namespace mk
