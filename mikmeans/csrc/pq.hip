// mikmeans — the scan of a product-quantised index (build_pq_index / PQIndex.search), for gfx950.
//
// An indexed row is M bytes: code j names one of 256 codewords of sub-space j of the row's
// residual against its list's centre.  A (query, probe) pair has a table [M][256] of float32, the
// squared distances of the query's residual sub-vectors to every codeword, and the pair's
// asymmetric distance to a row is table[0][c0] + table[1][c1] + ... + table[M-1][c(M-1)], float32
// adds in exactly that order.  No MFMA: the kernel streams codes from HBM and looks them up in LDS.
//
// Work item: one workgroup of PQ_NW waves per (pair, split) (csrc/pqplan.h).  The pair's table goes
// into LDS once (plain 16-byte loads and LDS stores), then every wave walks 64-row chunks of the
// pair's list, chunk index striding over the pair's 4 * splits waves: a lane takes one row, its M
// bytes in 8- or 16-byte loads that are contiguous across the lanes, and the next chunk's loads are
// issued before this chunk's look-ups.  Look-up j reads table + j * 1024 + 4 * code_j: the lane's
// address is the code alone, the sub-space an immediate offset.  Every lane keeps a sorted
// register list of its ML best (sum bits, position in list) by tk_insert (topk.h) -- ML = 8, 16 or
// 32, the shortest that holds m -- skipped where no lane of the wave has the candidate under its
// ML-th best.
//
// Merge: a wave takes m rounds of a wave-wide minimum over its lanes' heads ((bits << 32 |
// position) as one u64; positions are unique, so one lane wins and pops its head), the four
// waves' m keys meet in LDS and wave 0 merges them the same way: out[pair][split][0..m) ascending,
// IVF_EMPTY_KEY behind the rows there are.  The caller sorts a query's nprobe * splits * m unique
// keys, so the result does not depend on the splits.
#include "common.h"
#include "kernels.h"
#include "topk.h"

namespace mk {

// a lane's row: M bytes as dwords
template <int M>
struct PqCodes {
  uint32_t w[M / 4];
};

template <int M>
__device__ __forceinline__ PqCodes<M> pq_load(const uint8_t* __restrict__ codes, int64_t row, bool ok) {
  PqCodes<M> c;
  if constexpr (M == 8) {
    uint2 v = make_uint2(0u, 0u);
    if (ok) v = *(const uint2*)(codes + row * M);
    c.w[0] = v.x;
    c.w[1] = v.y;
  } else {
#pragma unroll
    for (int q = 0; q < M / 16; ++q) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (ok) v = *(const u32x4*)(codes + row * M + 16 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) c.w[4 * q + e] = v[e];
    }
  }
  return c;
}

// the row's asymmetric distance: M look-ups summed in sub-space order (no other order: the sum is
// compared bit for bit)
template <int M>
__device__ __forceinline__ float pq_adc(const MK_LDS float* tab, const PqCodes<M>& c) {
  float acc = tab[c.w[0] & 255u];
#pragma unroll
  for (int j = 1; j < M; ++j) acc = acc + tab[j * PQ_KSUB + ((c.w[j >> 2] >> (8 * (j & 3))) & 255u)];
  return acc;
}

__device__ __forceinline__ unsigned long long pq_wave_min(unsigned long long k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(k, o, 64);
    k = u < k ? u : k;
  }
  return k;
}

template <int M, int ML>
__global__ __launch_bounds__(PQ_NW * 64, 4) void pq_scan_kernel(PqScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pq_lds[];
  MK_LDS float* tab = (MK_LDS float*)pq_lds;
  MK_LDS unsigned long long* stage = (MK_LDS unsigned long long*)(pq_lds + M * PQ_KSUB * 4);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t p = blockIdx.x / a.splits;
  const int split = (int)(blockIdx.x - p * a.splits);
  const int m = a.m;

  // the pair's table: M KiB, 4 KiB a sweep of the workgroup
  {
    const u32x4* src = (const u32x4*)(a.lut + p * (M * PQ_KSUB));
    MK_LDS u32x4* dst = (MK_LDS u32x4*)pq_lds;
#pragma unroll
    for (int i = 0; i < M * PQ_KSUB / 4 / (PQ_NW * 64); ++i) {
      const int at = i * (PQ_NW * 64) + threadIdx.x;
      dst[at] = src[at];
    }
  }
  // the pair's list; a probe outside [0, K) has no rows
  const int list = a.probes[p];
  int64_t o0 = 0, nl = 0;
  if ((unsigned)list < (unsigned)a.K) {
    o0 = a.offsets[list];
    nl = a.offsets[list + 1] - o0;
    if (o0 < 0 || nl < 0 || o0 + nl > a.n) nl = 0;
  }
  __syncthreads();

  uint32_t bv[ML];
  int bi[ML];
#pragma unroll
  for (int j = 0; j < ML; ++j) {
    bv[j] = TK_EMPTY;
    bi[j] = TK_NOIDX;
  }
  const int64_t nch = pq_chunks(nl), stride = pq_chunk_stride(a.splits);
  const uint8_t* codes = a.codes + o0 * M;
  int64_t c = pq_first_chunk(split, wid);
  if (c < nch) {
    int64_t row = c * PQ_CHUNK + lane;
    PqCodes<M> cur = pq_load<M>(codes, row, row < nl);
    for (; c < nch; c += stride) {
      const int64_t nrow = (c + stride) * PQ_CHUNK + lane;
      const PqCodes<M> nxt = pq_load<M>(codes, nrow, nrow < nl);   // (past the last chunk: no lane loads)
      const float d = pq_adc<M>(tab, cur);
      const uint32_t cand = row < nl ? __float_as_uint(d) : TK_EMPTY;
      if (__builtin_amdgcn_ballot_w64(cand < bv[ML - 1]) != 0) tk_insert<ML>(bv, bi, cand, (int)row);
      cur = nxt;
      row = nrow;
    }
  }

  // the wave's m smallest: lane j keeps round j's
  unsigned long long mine = ~0ull;
#pragma unroll 1
  for (int j = 0; j < m; ++j) {
    const unsigned long long hk = ((unsigned long long)bv[0] << 32) | (uint32_t)bi[0];
    const unsigned long long best = pq_wave_min(hk);
    if ((uint32_t)(best >> 32) == TK_EMPTY) break;   // (wave-uniform: nothing is left)
    if (lane == j) mine = best;
    if (hk == best) {
#pragma unroll
      for (int s = 0; s + 1 < ML; ++s) {
        bv[s] = bv[s + 1];
        bi[s] = bi[s + 1];
      }
      bv[ML - 1] = TK_EMPTY;
      bi[ML - 1] = TK_NOIDX;
    }
  }
  if (lane < m) stage[wid * m + lane] = mine;
  __syncthreads();
  if (wid != 0) return;

  // wave 0: the four waves' keys, two a lane (4 m <= 128)
  unsigned long long k0 = lane < 4 * m ? stage[lane] : ~0ull;
  unsigned long long k1 = lane + 64 < 4 * m ? stage[lane + 64] : ~0ull;
  mine = ~0ull;
#pragma unroll 1
  for (int j = 0; j < m; ++j) {
    const unsigned long long best = pq_wave_min(k0 < k1 ? k0 : k1);
    if ((uint32_t)(best >> 32) == TK_EMPTY) break;
    if (lane == j) mine = best;
    if (k0 == best) k0 = ~0ull;
    else if (k1 == best) k1 = ~0ull;
  }
  if (lane < m) {
    long long key = (long long)IVF_EMPTY_KEY;   // behind every key in the per-query sort
    if ((uint32_t)(mine >> 32) != TK_EMPTY)
      key = (long long)((mine & 0xffffffff00000000ull) | (uint32_t)a.order[o0 + (int64_t)(uint32_t)mine]);
    a.out[((int64_t)blockIdx.x) * m + lane] = key;
  }
}

template <int M, int ML>
static hipError_t launch_pq_ml(int64_t nb, const PqScanArgs& a, hipStream_t s) {
  fold_lds_optin<pq_scan_kernel<M, ML>>();
  hipLaunchKernelGGL((pq_scan_kernel<M, ML>), dim3((unsigned)nb), dim3(PQ_NW * 64), (size_t)pq_lds_bytes(M, a.m), s, a);
  return hipGetLastError();
}

template <int M>
static hipError_t launch_pq_m(int64_t nb, const PqScanArgs& a, hipStream_t s) {
  // (the insertion is what a row costs past its look-ups: the shortest list that holds m)
  if (a.m <= 8) return launch_pq_ml<M, 8>(nb, a, s);
  return a.m <= 16 ? launch_pq_ml<M, 16>(nb, a, s) : launch_pq_ml<M, 32>(nb, a, s);
}

hipError_t launch_pq_scan(const PqScanArgs& a, hipStream_t s) {
  if (a.npairs <= 0) return hipSuccess;
  if (a.m < 1 || a.m > PQ_MAX_M || a.splits < 1 || a.splits > PQ_MAX_SPLITS || a.K < 1 || a.n < 0)
    return hipErrorInvalidValue;
  const int64_t nb = pq_grid(a.npairs, a.splits);
  if (nb == 0) return hipErrorInvalidValue;
  switch (a.M) {
    case 8: return launch_pq_m<8>(nb, a, s);
    case 16: return launch_pq_m<16>(nb, a, s);
    case 32: return launch_pq_m<32>(nb, a, s);
    case 64: return launch_pq_m<64>(nb, a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace mk
