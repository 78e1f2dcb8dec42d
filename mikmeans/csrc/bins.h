// mikmeans — the running count over the 256 bins of one radix-select histogram, shared by the two
// select kernels (csrc/quantiles.hip quantile_select_kernel, csrc/deep.hip ivf_select_kernel): a
// workgroup of QUANTILE_BINS threads, thread b holding bin b's count.
#pragma once
#include "block.h"
#include "kernels.h"

namespace mk {

// incl = the count of bins 0..b, total = the count of all bins, from c = bin b's count: block.h's
// scan, through wsum [QUANTILE_BINS / 64] (LDS).  Every thread of the workgroup calls it; a caller
// that calls it again may do so at once.
__device__ __forceinline__ void bins_running_count(unsigned long long c, unsigned long long* wsum,
                                                   unsigned long long& incl, unsigned long long& total) {
  incl = block_incl_scan<QUANTILE_BINS>(c, wsum, total);
}

}  // namespace mk
