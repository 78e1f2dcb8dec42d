// mikmeans — the running count over the 256 bins of one radix-select histogram, shared by the two
// select kernels (csrc/quantiles.hip quantile_select_kernel, csrc/deep.hip ivf_select_kernel): a
// workgroup of QUANTILE_BINS threads, thread b holding bin b's count.
#pragma once
#include "kernels.h"

namespace mk {

// incl = the count of bins 0..b, total = the count of all bins, from c = bin b's count.  A shuffle
// scan inside each wave, then the waves' sums through wsum [QUANTILE_BINS / 64] (LDS).  Every
// thread of the workgroup calls it; a caller that calls it again may do so at once (the first
// barrier keeps the previous call's wsum until every thread has read it).
__device__ __forceinline__ void bins_running_count(unsigned long long c, unsigned long long* wsum,
                                                   unsigned long long& incl, unsigned long long& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  incl = c;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  __syncthreads();                       // (the previous call's wsum has been read)
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  unsigned long long below = 0;
  total = 0;
  for (int i = 0; i < QUANTILE_BINS / 64; ++i) {
    const unsigned long long v = wsum[i];
    if (i < w) below += v;
    total += v;
  }
  incl += below;
}

}  // namespace mk
