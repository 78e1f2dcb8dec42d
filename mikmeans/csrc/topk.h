// mikmeans — the pieces the register-list kernels share (csrc/topk.hip: the m nearest centres of
// every row; csrc/ivf.hip: the m nearest indexed rows of every (query, probed list) pair): the
// candidate loop over a range of tiles (the tile step of tile.h, then the per-lane sorted
// list's insertion) and the merge of a row's four lane lists through LDS.  What a kernel keeps
// to itself is how a wave finds its rows and what it writes.
#pragma once
#include "common.h"
#include "kernels.h"
#include "tile.h"

namespace mk {

constexpr int TK_NW = 4;                    // waves per workgroup
constexpr uint32_t TK_EMPTY = 0xffffffffu;  // list slot without a candidate (above every clamp_d2 value)
constexpr int TK_NOIDX = 0x7fffffff;
// (A kernel fills its lists with these itself: as one more shared helper the same two loops
// moved the register allocation of sixteen kernels by 40-50 VGPRs, profiles/r9_01_tile_frame.md.)

// Whether a wave's rows stay in registers (4 NQ VGPRs a block) beside the list: the kernel is
// held to the 256 VGPRs of two waves per SIMD, and the M = 32 insertion needs ~140 of them
// (NQ = 32 spilled 20), the M = 8 one ~50.  Past that (f32 D > 768; the long list from bf16
// D > 768 and f32 D > 384) the row fragments are fetched again for every tile (L1 / L2 hits).
constexpr bool topk_xreg(int nq, int m) { return nq <= (m > 8 ? 24 : 48); }

// Row blocks per wave: the rows' fragments (4 NQ VGPRs), the list (2 M) and the accumulators
// (4) of every block within ~176 VGPRs, at most 4 blocks -- two waves per SIMD wherever the
// transform kernel has them (tests/test_gpu_topk.py reads the built code object).
constexpr int topk_blocks(int nq, int m) {
  const int p = 176 / (4 * nq + 2 * m + 4);
  return p < 1 ? 1 : (p > 4 ? 4 : p);
}

// The walks without a list (csrc/range.hip, csrc/deep.hip).
// Whether a wave's queries stay in registers (4 NQ VGPRs a block); past that (f32 D > 768) the
// fragments are fetched again for every tile, as in topk.h
constexpr bool range_xreg(int nq) { return nq <= 48; }

// Pair blocks per wave: the queries' fragments (4 NQ VGPRs), the accumulators (4) and the
// per-block state (pair id, base, radius, count: ~8) of every block within ~176 VGPRs, at most 4
constexpr int range_blocks(int nq) {
  const int p = 176 / (4 * nq + 12);
  return p < 1 ? 1 : (p > 4 ? 4 : p);
}

// Candidate (c, ck) into a lane's sorted list (the caller has skipped it where no lane of the
// wave has c < bv[M - 1]): slot j takes its left neighbour where c goes in front of both, c
// itself where it goes in front of slot j only (every compare against c: a displaced entry
// never passes an equal one, which a compare-and-swap chain of the carried entry would do)
template <int M>
__device__ __forceinline__ void tk_insert(uint32_t (&bv)[M], int (&bi)[M], uint32_t c, int ck) {
#pragma unroll
  for (int j = M - 1; j > 0; --j) {
    const bool s = c < bv[j], sl = c < bv[j - 1];
    bv[j] = s ? (sl ? bv[j - 1] : c) : bv[j];
    bi[j] = s ? (sl ? bi[j - 1] : ck) : bi[j];
  }
  const bool s0 = c < bv[0];
  bv[0] = s0 ? c : bv[0];
  bi[0] = s0 ? ck : bi[0];
}

// A row block's lists to the wave's LDS slab as (bits << 32 | index) keys, [slot][lane]
// (conflict-free), fenced for the merging lanes
template <int M>
__device__ __forceinline__ void tk_stage(MK_LDS unsigned long long* ws, int lane, const uint32_t (&bv)[M],
                                         const int (&bi)[M]) {
#pragma unroll
  for (int j = 0; j < M; ++j) ws[j * 64 + lane] = ((unsigned long long)bv[j] << 32) | (uint32_t)bi[j];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lane r merges the four lists of its row (lanes r, r + 16, r + 32, r + 48) in a rolled loop:
// emit(j, key) for the m smallest keys in ascending order
template <int M, typename Emit>
__device__ __forceinline__ void tk_merge4(const MK_LDS unsigned long long* ws, int r, int m, Emit emit) {
  unsigned long long hk[4];
  int hp[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    hp[q] = 0;
    hk[q] = ws[r + 16 * q];
  }
#pragma unroll 1
  for (int j = 0; j < m; ++j) {
    unsigned long long best = hk[0];
    int sel = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      if (hk[q] < best) {
        best = hk[q];
        sel = q;
      }
    }
    emit(j, best);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (sel == q) {
        ++hp[q];
        hk[q] = hp[q] < M ? ws[hp[q] * 64 + r + 16 * q] : ~0ull;
      }
    }
  }
}

// The candidate loop: tiles [t0, t1) of `pack` against the wave's P row blocks, every d2 of
// tile_d2 offered to its lane's list with its packed row's number k; k >= nvalid (a pad row) is
// an empty candidate, which the strict compare never takes.  A tile's candidate is skipped
// where no lane of the wave has it under its current M-th best.
template <typename T, int NQ, int P, int M, bool XREG>
__device__ __forceinline__ void tk_scan(const T* pack, const float* cn, int t0, int t1, int nvalid, int lane, int g,
                                        const u32x4 (&xr)[P][XREG ? NQ : 1], const T* const (&xp)[P], int D,
                                        const float (&xn)[P], uint32_t (&bv)[P][M], int (&bi)[P][M]) {
  for (int t = t0; t < t1; ++t) {
    f32x4 d2[P];
    tile_d2<T, NQ, P, XREG>(pack, cn, t, lane, g, xr, xp, D, xn, d2);
    const int k0 = t * 16 + 4 * g;
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t c = k0 + e < nvalid ? __float_as_uint(d2[p][e]) : TK_EMPTY;
        const int ck = k0 + e;
        if (__builtin_amdgcn_ballot_w64(c < bv[p][M - 1]) == 0) continue;
        tk_insert<M>(bv[p], bi[p], c, ck);
      }
    }
  }
}

// The merge loop: block after block through the wave's LDS slab ws; lane r < 16 merges row
// 16p + r of the wave's first nrows rows and hands its m keys to emit_for(p)(j, key)
template <int P, int M, typename EmitFor>
__device__ __forceinline__ void tk_merge_rows(MK_LDS unsigned long long* ws, int lane, int nrows, int m,
                                              const uint32_t (&bv)[P][M], const int (&bi)[P][M], EmitFor emit_for) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    tk_stage<M>(ws, lane, bv[p], bi[p]);
    if (lane < 16 && p * 16 + lane < nrows) tk_merge4<M>(ws, lane, m, emit_for(p));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the next block's keys overwrite the slab
  }
}

}  // namespace mk
