// mikmeans — the fitted clusters as an inverted-file index (build_index / search), for gfx950.
//
// Three pieces, each in launches of its own; no workgroup ever waits for another.
//
// 1. Stable partition by label: order = the rows with a label in [0, K), label after label and
//    ascending inside a label, offsets = where each label's rows start (the stable sort of the
//    labels and the cumulative bincount).  Count, scan, scatter in the style of the compaction
//    kernels of csrc/rows.hip: a workgroup counts its contiguous rows per label in LDS, one
//    workgroup scans the [K][blocks] counts (label-major, so a label's blocks follow each other;
//    block.h scan_slices),
//    and the scatter pass recounts per wave, turns the [4 waves][K] counters into running
//    positions (block base + the waves before) and walks its rows again: the lanes of a wave that
//    share a label are found by ballots, a lane's rank among them is the mbcnt of that ballot and
//    the group's first lane moves the label's position on.  LDS atomics only count; no position
//    depends on an atomic's return order, so order is the same on every launch.  The same op
//    groups the (query, probe) pairs of a search by list.
// 2. Row pack: the indexed rows, list after list and each list padded to whole 16-row tiles, in
//    the fragment-packed layout of kernels.h with their cn -- bit for bit what the centre pack
//    (csrc/finalize.hip, pack-only) makes of the same rows: both run pack_elem (pack.h) over the
//    same features per lane and sum the eight lanes by the same butterfly.  X is read in its own
//    dtype.  An index that gains or loses rows is not packed again: the repack copies the rows
//    that stay from the old pack into a new one under the new offsets, bit for bit, and only the
//    rows new to the index go through the row pack.
// 3. Scan: a wave takes one work item of the walk over the lists (csrc/walk.h: a list and a block
//    of the pairs probing it), gathers its queries' fragments as topk_kernel holds rows, walks
//    the list's tiles straight from global memory and keeps the M best (d2 bits, position in
//    list) per lane with the insertion of topk.h; a query's four lanes merge through LDS and lane
//    r writes the pair's m keys (d2 bits << 32 | row).  d2 is bitwise the transform kernel's value
//    for (query, row) with the rows packed as centres: the one tile step of tile.h (negatives to
//    +0, NaN and +inf kept, so a query with a NaN or infinite coordinate finds no row at distance
//    0).
#include "block.h"
#include "dispatch.h"
#include "pack.h"
#include "topk.h"

namespace mk {

// ---- 1. stable partition -------------------------------------------------------------------
constexpr int PT_T = 256;            // threads of a count / scatter workgroup (4 waves)
constexpr int PT_MAX_BLOCKS = 1024;
constexpr int64_t PT_MAX_CELLS = 1 << 20;   // K * blocks: what the one-workgroup scan walks

int64_t partition_blocks(int64_t n, int K) {
  int64_t cap = PT_MAX_CELLS / (K > 0 ? K : 1);
  cap = cap < 1 ? 1 : (cap > PT_MAX_BLOCKS ? PT_MAX_BLOCKS : cap);
  const int64_t want = (n + 1023) / 1024;
  return want < 1 ? 1 : (want < cap ? want : cap);
}
// rows of a workgroup: a multiple of 256, so every wave's quarter is whole 64-row steps
static int64_t partition_block_rows(int64_t n, int64_t nb) { return ((n + nb - 1) / nb + 255) / 256 * 256; }

__global__ __launch_bounds__(PT_T) void partition_count_kernel(const int32_t* __restrict__ labels, int64_t n, int K,
                                                              int64_t block_rows, int64_t nb,
                                                              int64_t* __restrict__ cells) {
  extern __shared__ uint32_t pt_lds[];
  for (int k = threadIdx.x; k < K; k += PT_T) pt_lds[k] = 0u;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * block_rows;
  const int64_t r1 = r0 + block_rows < n ? r0 + block_rows : n;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += PT_T) {
    const int l = labels[i];
    if ((unsigned)l < (unsigned)K) atomicAdd(&pt_lds[l], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += PT_T) cells[(int64_t)k * nb + blockIdx.x] = pt_lds[k];
}

// cells (label-major counts) -> their exclusive prefix sums, in place; offsets[k] = the prefix at
// label k's first block, offsets[K] = the total.  One workgroup, fixed order.
__global__ __launch_bounds__(1024) void partition_scan_kernel(int64_t* __restrict__ cells, int64_t nb, int K,
                                                              int64_t* __restrict__ offsets) {
  const int64_t total = scan_slices<1024>(
      (int64_t)K * nb, [&](int64_t i) { return cells[i]; },
      [&](int64_t i, int64_t excl) {
        cells[i] = excl;
        if (i % nb == 0) offsets[i / nb] = excl;
      });
  if (threadIdx.x == 0) offsets[K] = total;
}

__global__ __launch_bounds__(PT_T) void partition_scatter_kernel(const int32_t* __restrict__ labels, int64_t n, int K,
                                                                int64_t block_rows, int64_t nb,
                                                                const int64_t* __restrict__ cells,
                                                                int64_t* __restrict__ order,
                                                                int64_t* __restrict__ rpos) {
  extern __shared__ uint32_t pt_lds[];   // [4 waves][K]: counts, then running positions
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int k = threadIdx.x; k < 4 * K; k += PT_T) pt_lds[k] = 0u;
  __syncthreads();
  const int64_t q = block_rows / 4;
  const int64_t r0 = (int64_t)blockIdx.x * block_rows + w * q;
  const int64_t r1 = r0 + q < n ? r0 + q : n;
  uint32_t* mine = pt_lds + (int64_t)w * K;
  for (int64_t base = r0; base < r1; base += 64) {
    const int64_t i = base + lane;
    const int l = i < r1 ? labels[i] : -1;
    if ((unsigned)l < (unsigned)K) atomicAdd(&mine[l], 1u);
  }
  __syncthreads();
  // a wave's first position of label k: the block's base, then the waves before it (fixed order)
  for (int k = threadIdx.x; k < K; k += PT_T) {
    uint32_t p = (uint32_t)cells[(int64_t)k * nb + blockIdx.x];   // (fewer than 2^32 rows)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t c = pt_lds[j * K + k];
      pt_lds[j * K + k] = p;
      p += c;
    }
  }
  __syncthreads();
  for (int64_t base = r0; base < r1; base += 64) {
    const int64_t i = base + lane;
    const int l = i < r1 ? labels[i] : -1;
    bool pend = (unsigned)l < (unsigned)K;
    unsigned long long pm;
    while ((pm = __builtin_amdgcn_ballot_w64(pend)) != 0ull) {
      const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(pm));
      const int lk = __builtin_amdgcn_readlane(l, lead);
      const bool hit = pend && l == lk;
      const unsigned long long mm = __builtin_amdgcn_ballot_w64(hit);
      const uint32_t start = mine[lk];
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
      if (hit) {
        order[start + rank] = i;
        if (rpos) rpos[i] = (int64_t)(start + rank);
      }
      if (lane == lead) mine[lk] = start + (uint32_t)__builtin_popcountll(mm);
      pend = pend && !hit;
    }
  }
}

hipError_t launch_partition(const int32_t* labels, int64_t n, int K, int64_t* order, int64_t* offsets, int64_t* cells,
                            int64_t* rpos, hipStream_t s) {
  if (K < 1 || K > PARTITION_MAX_K || n < 0 || n >= ((int64_t)1 << 32)) return hipErrorInvalidValue;
  const int64_t nb = partition_blocks(n, K), br = partition_block_rows(n, nb);
  hipError_t e = hipSuccess;
  if (n > 0) {
    e = hipMemsetAsync(order, 0xff, (size_t)n * 8, s);   // the tail past the valid rows: -1
    if (e == hipSuccess && rpos) e = hipMemsetAsync(rpos, 0xff, (size_t)n * 8, s);
    if (e != hipSuccess) return e;
  }
  fold_lds_optin<partition_scatter_kernel>();
  hipLaunchKernelGGL(partition_count_kernel, dim3((unsigned)nb), dim3(PT_T), (size_t)K * 4, s, labels, n, K, br, nb,
                     cells);
  hipLaunchKernelGGL(partition_scan_kernel, dim3(1), dim3(1024), 0, s, cells, nb, K, offsets);
  if (n > 0)
    hipLaunchKernelGGL(partition_scatter_kernel, dim3((unsigned)nb), dim3(PT_T), (size_t)K * 16, s, labels, n, K, br,
                       nb, cells, order, rpos);
  return hipGetLastError();
}

// ---- 2. row pack ---------------------------------------------------------------------------
// Eight lanes a row, 32 rows a workgroup, as finalize_kernel packs centres.  Row i of the block
// (row row0 + i of the index) goes to packed row 16 toff[k] + (its position - offsets[k]), k its
// list; rows in no list (rpos < 0) are skipped.  Pad rows and pad columns keep what the caller
// filled the buffers with (zeros, and PAD_SCORE in cn).
template <typename T>
__global__ __launch_bounds__(256) void ivf_pack_kernel(IvfPackArgs a) {
  const int kk = threadIdx.x >> 3, part = threadIdx.x & 7;
  const int64_t i = (int64_t)blockIdx.x * 32 + kk;
  float cn = 0.f;
  int64_t dst = -1;
  if (i < a.nb) {
    const int64_t row = a.row0 + i;
    const int64_t p = a.rpos[row];
    if (p >= 0) {
      const int k = a.labels[row];
      dst = a.toff[k] * 16 + (p - a.offsets[k]);
      const T* x = (const T*)a.X + i * a.ldx;
      for (int d = part; d < a.D; d += 8) {
        const float old = Elem<T>::to_f32(x[d]);
        const float q = (a.dtype == DT_BF16) ? round_bf16(old) : old;
        pack_elem(a.dtype, a.pack, a.dpad, dst, d, q, cn);
      }
    }
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) cn += __shfl_xor(cn, o, 64);
  if (part == 0 && dst >= 0) a.cn[dst] = cn;
}

hipError_t launch_ivf_pack(const IvfPackArgs& a, hipStream_t s) {
  if (a.nb <= 0) return hipSuccess;
  if (a.D > a.dpad || a.K < 1) return hipErrorInvalidValue;
  const unsigned nb = (unsigned)((a.nb + 31) / 32);
  return (hipError_t)for_type(a.dtype, [&](auto t) {
    hipLaunchKernelGGL(ivf_pack_kernel<typename decltype(t)::type>, dim3(nb), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

// ---- 2b. repack ----------------------------------------------------------------------------
// The rows that stay, from an old pack into a new one (kernels.h IvfRepackArgs): a wave takes one
// destination tile, lane r + 16 g the 16-byte pieces of lane group g of the tile's row r, so every
// store instruction of the wave writes 1 KiB in packed order and the sixteen rows of a source tile
// are read in 256-byte runs.  The wave finds its list by list_of (walk.h) over the new tile offsets
// (the grid is launched over the allocation; waves past toff[K] exit), the lane its row's id in
// the new order and, through the id's old position, its old packed row.  Bits are copied, both
// dtypes alike (a piece is 16 bytes); pad rows and the rows new to the index are not written.
// Every destination piece has one writer and nothing written is read: no atomics, no LDS, no
// barrier.
constexpr int RP_NW = 4;   // waves (destination tiles) of a workgroup

__global__ __launch_bounds__(RP_NW * 64) void ivf_repack_kernel(IvfRepackArgs a, int nq) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t t = (int64_t)blockIdx.x * RP_NW + wid;
  if (t >= a.toff[a.K] || (t + 1) * 16 > a.rows_new) return;   // (wave-uniform)
  const int k = list_of(a.toff, a.K, t);
  const int64_t p = (t - a.toff[k]) * 16 + r;
  const int64_t o0 = a.offsets[k];
  int64_t src = -1;
  if (p < a.offsets[k + 1] - o0 && o0 + p < a.n) {
    const int64_t id = a.order[o0 + p];
    if (id >= 0 && id < a.n_old) {
      const int64_t po = a.rpos_old[id], b0 = a.offsets_old[k];
      if (po >= b0 && po < a.offsets_old[k + 1]) {
        const int64_t s = a.toff_old[k] * 16 + (po - b0);
        if (s >= 0 && s < a.rows_old) src = s;
      }
    }
  }
  if (src < 0) return;
  const u32x4* from = (const u32x4*)a.pack_old + ((src >> 4) * nq * 64 + (src & 15) + 16 * g);
  u32x4* to = (u32x4*)a.pack + (t * nq * 64 + lane);
  int q = 0;
  for (; q + 4 <= nq; q += 4) {
    const u32x4 v0 = from[(q + 0) * 64], v1 = from[(q + 1) * 64], v2 = from[(q + 2) * 64], v3 = from[(q + 3) * 64];
    to[(q + 0) * 64] = v0;
    to[(q + 1) * 64] = v1;
    to[(q + 2) * 64] = v2;
    to[(q + 3) * 64] = v3;
  }
  for (; q < nq; ++q) to[q * 64] = from[q * 64];
  if (g == 0) a.cn[t * 16 + r] = a.cn_old[src];
}

hipError_t launch_ivf_repack(const IvfRepackArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.n_old <= 0 || a.rows_new <= 0 || a.rows_old <= 0) return hipSuccess;
  if (a.D > a.dpad || a.K < 1) return hipErrorInvalidValue;
  const int piece = dtype_vec(a.dtype);
  if (a.dpad % (4 * piece) != 0 || a.rows_new % 16 != 0 || a.rows_old % 16 != 0) return hipErrorInvalidValue;
  const int64_t nb = (a.rows_new / 16 + RP_NW - 1) / RP_NW;
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ivf_repack_kernel, dim3((unsigned)nb), dim3(RP_NW * 64), 0, s, a, a.dpad / (4 * piece));
  return hipGetLastError();
}

// ---- 3. scan ---------------------------------------------------------------------------------
template <typename T, int DPAD, int P, int M>
__global__ __launch_bounds__(TK_NW * 64, 2) void ivf_scan_kernel(IvfScanArgs a) {
  constexpr int V = Elem<T>::V;
  constexpr int NQ = DPAD / 4 / V;
  constexpr bool XREG = topk_xreg(NQ, M);
  __shared__ unsigned long long sm[TK_NW * M * 64];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t item = (int64_t)blockIdx.x * TK_NW + wid;
  if (item >= a.w.icum[a.w.K]) return;   // (wave-uniform; the kernel has no workgroup barrier)
  const WalkItem it = walk_item<P * 16>(a.w.icum, a.w.poff, a.w.offsets, a.w.K, item);
  u32x4 xr[P][XREG ? NQ : 1];
  const T* xp[P];
  float xn[P];
  int64_t pid[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int slot = p * 16 + r;
    pid[p] = a.w.porder[it.p0 + (slot < it.np ? slot : it.np - 1)];
    load_row<T, NQ, XREG>(a.w.Q, a.w.ldq, pid[p] / a.w.nprobe, a.w.qn, g, a.w.D, xr[p], xp[p], xn[p]);
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
  // the list's tiles; a position past its length is an empty candidate
  const int64_t t0 = a.w.toff[it.list];
  tk_scan<T, NQ, P, M, XREG>((const T*)a.w.pack + t0 * (NQ * 64 * V), a.w.cn + t0 * 16, 0, (it.nl + 15) / 16, it.nl,
                             lane, g, xr, xp, a.w.D, xn, bv, bi);
  MK_LDS unsigned long long* ws = (MK_LDS unsigned long long*)sm + wid * (M * 64);
  const int64_t* ord = a.w.order + it.o0;
  tk_merge_rows(ws, lane, it.np, a.m, bv, bi, [&](int p) {
    long long* out = a.out + pid[p] * a.m;
    return [=](int j, unsigned long long best) {
      const uint32_t bits = (uint32_t)(best >> 32);
      // an empty slot: the largest int64, behind every key in the per-query sort
      out[j] = bits == TK_EMPTY ? (long long)IVF_EMPTY_KEY
                                : (long long)(((unsigned long long)bits << 32) | (uint32_t)ord[(uint32_t)best]);
    };
  });
}

// The walk's launch (kernels.h): TK_NW items a workgroup over max_items, the upper bound of icum[K]
hipError_t ivf_walk_grid(const IvfWalkArgs& w, int dpad, int64_t& nb) {
  nb = 0;
  if (w.npairs <= 0 || w.max_items <= 0) return hipSuccess;
  if (w.K < 1 || w.nprobe < 1 || w.D > dpad) return hipErrorInvalidValue;
  if ((w.max_items + TK_NW - 1) / TK_NW > 0x7fffffff) return hipErrorInvalidValue;
  nb = (w.max_items + TK_NW - 1) / TK_NW;
  return hipSuccess;
}

template <typename T, int DPAD, int P, int M>
static hipError_t launch_is_p(int64_t nb, const IvfScanArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((ivf_scan_kernel<T, DPAD, P, M>), dim3((unsigned)nb), dim3(TK_NW * 64), 0, s, a);
  return hipGetLastError();
}

template <typename T, int DPAD, int M>
static hipError_t launch_is_m(int P, int64_t nb, const IvfScanArgs& a, hipStream_t s) {
  constexpr int PF = topk_blocks(DPAD / 4 / Elem<T>::V, M);
  if (P == 1) return launch_is_p<T, DPAD, 1, M>(nb, a, s);
  if (P == PF) return launch_is_p<T, DPAD, PF, M>(nb, a, s);
  return hipErrorInvalidValue;
}

template <typename T, int DPAD>
static hipError_t launch_is(int P, int64_t nb, const IvfScanArgs& a, hipStream_t s) {
  return a.m <= 8 ? launch_is_m<T, DPAD, 8>(P, nb, a, s) : launch_is_m<T, DPAD, 32>(P, nb, a, s);
}

// Pair blocks per wave: topk's rule (topk_blocks, then walk_blocks over the pairs)
int ivf_scan_blocks(int dtype, int dpad, int m, int64_t npairs) {
  const int nq = dpad / 4 / dtype_vec(dtype);
  return walk_blocks(topk_blocks(nq, m <= 8 ? 8 : 32), npairs);
}

hipError_t launch_ivf_scan(int dtype, int dpad, int P, const IvfScanArgs& a, hipStream_t s) {
  int64_t nb;
  if (const hipError_t e = ivf_walk_grid(a.w, dpad, nb); e != hipSuccess || nb == 0) return e;
  if (a.m < 1 || a.m > TOPK_MAX) return hipErrorInvalidValue;
  return (hipError_t)for_width(dtype, dpad, [&](auto t, auto w) {
    return launch_is<typename decltype(t)::type, decltype(w)::value>(P, nb, a, s);
  });
}

}  // namespace mk
