// mikmeans — the re-rank of a search's candidates against the rows themselves
// (PQIndex.search(refine=)), for gfx950.
//
// out[q][j] = clamp_d2(|Q[q] - X[cand[q][j]]|^2) bits << 32 | cand[q][j], IVF_EMPTY_KEY for an id
// outside [0, n).  The distance is defined bit for bit (docs/PQ_INDEX.md): the row is cut into
// 16-byte pieces of V columns, accumulator a_s (s = 0..15, from +0) takes the pieces s, s + 16, ...
// and every column of a piece in order as d = q - x, p = d * d, a_s = a_s + p -- three float32
// operations rounded one by one (this file is built with -ffp-contract=off, mikmeans/_build.py) --
// and the sixteen accumulators meet in sum16_xor's order at lane 0.  A column >= F is 0 in both
// operands, so it adds +0 to an accumulator that is never -0: nothing.
//
// No MFMA and no LDS: a gather bound by the latency of the row loads.  A wave takes a run of one
// query's candidates (csrc/rerankplan.h), loads their ids once, one a lane, and hands them to the
// lane groups by ds_bpermute.  Sixteen lanes share a (query, candidate) pair, lane s holds a_s, so
// a round of 16-byte loads is contiguous across the pair's lanes; four pairs a step, and the loads
// of four steps (a batch: sixteen rows) are issued together and before the arithmetic of the batch
// in flight.  A row pointer or stride off 16 bytes, and a last piece cut by F, take element loads
// into the same piece.
#include "common.h"
#include "kernels.h"

namespace mk {

// piece t of a row (V columns from column t V): one 16-byte load, or element loads with columns
// >= F as 0; nothing is read where !ok
template <typename T, bool VEC>
__device__ __forceinline__ u32x4 rr_piece(const T* __restrict__ row, int t, int F, bool ok) {
  constexpr int V = Elem<T>::V;
  u32x4 w = {0u, 0u, 0u, 0u};
  if (!ok) return w;
  const int c0 = t * V;
  if (VEC && c0 + V <= F) return *(const u32x4*)(row + c0);
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t lo = c0 + 2 * i < F ? (uint32_t)row[c0 + 2 * i] : 0u;
      const uint32_t hi = c0 + 2 * i + 1 < F ? (uint32_t)row[c0 + 2 * i + 1] : 0u;
      w[i] = lo | (hi << 16);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = c0 + i < F ? __float_as_uint(row[c0 + i]) : 0u;
  }
  return w;
}

constexpr uint32_t RR_NOROW = 0xffffffffu;   // (n < 2^32: no row has this id)

template <typename T, bool VEC>
__global__ __launch_bounds__(RR_NW * 64) void rerank_kernel(RerankArgs a) {
  constexpr int V = Elem<T>::V;
  const int lane = threadIdx.x & 63, sub = lane & (RR_GROUP - 1), grp = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * RR_NW + wid;
  if (item >= a.items) return;   // (wave-uniform; the kernel has no barrier)
  const int64_t q = rr_item_query(item, a.runs), first = rr_item_first(item, a.runs, a.run);
  const int cnt = rr_item_count(first, a.R, a.run);
  const int F = a.F, np = rr_pieces(F, V), rounds = rr_rounds(np), nb = rr_batches(cnt);

  // the run's ids, one a lane; an id outside [0, n) is an empty slot
  uint32_t id = RR_NOROW;
  if (lane < cnt) {
    const long long c = a.cand[q * a.R + first + lane];
    if ((unsigned long long)c < (unsigned long long)a.n) id = (uint32_t)c;
  }
  const T* __restrict__ X = (const T*)a.X;
  const T* __restrict__ qrow = (const T*)a.Q + q * a.ldq;

  // round k of batch b: the lane's piece t = sub + 16 k of the query and of the batch's four rows
  auto load = [&](int b, int k, u32x4(&x)[RR_STEPS], u32x4& qp) {
    const int t = sub + RR_GROUP * k;
    const bool in = t < np;
    qp = rr_piece<T, VEC>(qrow, t, F, in);
#pragma unroll
    for (int u = 0; u < RR_STEPS; ++u) {
      const uint32_t r = __shfl(id, rr_slot(b, u, grp), 64);   // (slot < 64 = RR_MAX_RUN)
      x[u] = rr_piece<T, VEC>(X + (int64_t)r * a.ldx, t, F, in && r != RR_NOROW);
    }
  };

  float acc[RR_STEPS];
#pragma unroll
  for (int u = 0; u < RR_STEPS; ++u) acc[u] = 0.f;
  u32x4 cx[RR_STEPS], cq;
  int b = 0, k = 0;
  load(b, k, cx, cq);
  while (b < nb) {
    int nxb = b, nxk = k + 1;
    if (nxk == rounds) {
      nxk = 0;
      ++nxb;
    }
    u32x4 nx[RR_STEPS], nq;
    if (nxb < nb) {
      load(nxb, nxk, nx, nq);   // the next round's loads, before this round's arithmetic
    } else {
      nq = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int u = 0; u < RR_STEPS; ++u) nx[u] = nq;
    }
    float qf[V];
    unpack16(cq, qf, (T*)nullptr);
#pragma unroll
    for (int u = 0; u < RR_STEPS; ++u) {
      float xf[V];
      unpack16(cx[u], xf, (T*)nullptr);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float d = __fsub_rn(qf[e], xf[e]);
        const float p = __fmul_rn(d, d);
        acc[u] = __fadd_rn(acc[u], p);
      }
    }
    if (k == rounds - 1) {
#pragma unroll
      for (int u = 0; u < RR_STEPS; ++u) {
        const float d2 = clamp_d2(sum16_xor(acc[u]));
        const int slot = rr_slot(b, u, grp);
        const uint32_t r = __shfl(id, slot, 64);
        if (sub == 0 && slot < cnt) {
          long long key = (long long)IVF_EMPTY_KEY;
          if (r != RR_NOROW) key = (long long)(((unsigned long long)__float_as_uint(d2) << 32) | r);
          a.out[q * a.R + first + slot] = key;
        }
        acc[u] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < RR_STEPS; ++u) cx[u] = nx[u];
    cq = nq;
    b = nxb;
    k = nxk;
  }
}

template <typename T>
static hipError_t launch_rerank_t(int64_t nb, bool vec, const RerankArgs& a, hipStream_t s) {
  return (hipError_t)for_flag(vec, [&](auto v) {
    hipLaunchKernelGGL((rerank_kernel<T, decltype(v)::value>), dim3((unsigned)nb), dim3(RR_NW * 64), 0, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_rerank(int dtype, const RerankArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.R <= 0) return hipSuccess;
  if (a.F < 1 || a.n < 0 || a.n >= (int64_t(1) << 32) || a.ldq < a.F || a.ldx < a.F) return hipErrorInvalidValue;
  if (a.run < RR_MIN_RUN || a.run > RR_MAX_RUN || a.runs != rr_runs(a.R, a.run) ||
      a.items != rr_items(a.nq, a.R, a.run))
    return hipErrorInvalidValue;
  const int64_t nb = rr_grid(a.items);
  if (nb == 0) return hipErrorInvalidValue;
  const int64_t es = dtype == DT_BF16 ? 2 : 4;
  const bool vec = (uintptr_t)a.Q % 16 == 0 && (uintptr_t)a.X % 16 == 0 && a.ldq * es % 16 == 0 && a.ldx * es % 16 == 0;
  return (hipError_t)for_type(dtype, [&](auto t) { return launch_rerank_t<typename decltype(t)::type>(nb, vec, a, s); });
}

}  // namespace mk
