// mikmeans — K2: nearest-centroid assignment on 16x16 MFMA tiles for gfx950
// (v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x4_f32).
//
// Pipeline: fragment-packed centroid chunks stream through an LDS ring fed by LDS-DMA
// (global_load_lds_dwordx4, no VGPR round trip); every wave keeps P blocks of 16
// points in registers and multiplies them against each 16-centroid tile:
//  * lane (r = l&15, g = l>>4) holds the B fragments of point p0+r, piece q covering
//    features [(4q+g)V, +V) (V = 16 B of elements), and the A fragments of centroid r
//    of the tile (the packed -2c), same features.  Interleaving the lane groups' pieces
//    makes each fragment load read 64 contiguous bytes per point (16 rows per wave
//    instruction); giving each lane group a contiguous quarter of the row instead made
//    every load touch 64 cache lines, and the loads cost a fixed ~27 % of the D=256
//    K=512 assign (profiles/r2_08_assign_clock_study.md);
//  * the accumulators are seeded with |c|^2 (+ the point offset below), so the output
//    D[row = 4g+reg][col = r] is the score of point r against centroid 16t+4g+reg and
//    each lane holds 4 scores of its point per tile; the 4 lane groups g merge once at
//    the end.
//
// Argmin epilogue.
//  * bf16: keys carry a 6-bit index in the low mantissa bits (tile-in-segment*4 + reg)
//    so one v_min3 tree yields (min, index): 1.5 VALU per score.  The workgroup adds
//    o = (1 + 2^-12) max |x|^2 over its 192-512 points to its LDS copy of |c|^2 once,
//    which makes every key |x-c|^2 + (o - |x|^2) > 0: among equal keys the lower index
//    then always wins (an OR of the index into a NEGATIVE float favours the higher one),
//    and the key resolution is 2^-17 of the squared distance plus the spread of |x|^2
//    inside the workgroup, not 2^-17 of |x|^2 (coarse for data far from the origin).
//    Where that spread is large (max |x|^2 > 4 min |x|^2: an outlier row, data around the
//    origin) the workgroup uses per-point offsets instead (they seed each tile's
//    accumulators, in a second instantiation of the chunk loop), so the resolution is never
//    worse than 2^-17 (|x-c|^2 + 3|x|^2).  Per-point offsets everywhere would make the keys
//    a function of the point alone, but cost 17 % at the headline shape (one process A/B,
//    round 2); workgroups are therefore aligned to the global ROW_ALIGN = 1536-row grid by
//    the callers (shard_range, streaming chunks), so near-tie resolution is the same on
//    any world size.
//  * bf16 D <= 64 with many centres (VARG): the keys' 1.5 VALU per score bound the body
//    (1-2 MFMAs per tile and block), so the main loop keeps only the running minimum value
//    (2 v_min3_u32 per tile and block: the positive scores order as their bits) and the
//    tile that lowered it (v_cmp + v_cndmask): 1.0 VALU per score.  After the loop the
//    winning tile's 4 candidate rows of every point are recomputed on the matrix cores,
//    bitwise the main loop's scores, and the first equal to the minimum is the label
//    (full fp32 resolution; 64/K extra matrix work, so K >= 2048 at D=64, >= 1024 at D=32).
//  * f32: an exact (value, index) compare per score (v_cmp + 2 v_cndmask).  The f32
//    MFMA is 16x slower per FLOP than bf16, so the epilogue is noise there and the
//    labels carry full fp32 score resolution; strict < in ascending index order keeps
//    the lowest index on exact ties.
//
// Layout "16" of the packed centroids (csrc/kernels.h):
//   element (k, d): t = k/16, r = k%16, q = d / (4V), g = (d / V) % 4
//   offset = ((t*NQ + q)*64 + r + 16*g)*V + d%V,  NQ = DPAD/(4V)
//
// The steps assign16_kernel and assign16_persist_kernel both take -- the ring DMA, the LDS
// layout, the seed rule, the packed-key tile step, the label decode -- are csrc/assign_step.h.
#include <cstdlib>
#include <type_traits>

#include "assign_step.h"   // the steps both kernels take: ring DMA, LDS layout, seed rule, tile step, label decode
#include "common.h"
#include "kernels.h"
#include "plan.h"

namespace mk {

using plan::chunk_tiles16;

// Sum of squares of one lane's 16-byte piece.
__device__ __forceinline__ float sq16(const u32x4& w, uint16_t*) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lo = bf16lo(w[i]), hi = bf16hi(w[i]);
    s = __builtin_fmaf(lo, lo, s);
    s = __builtin_fmaf(hi, hi, s);
  }
  return s;
}
__device__ __forceinline__ float sq16(const u32x4& w, float*) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) s = __builtin_fmaf(__uint_as_float(w[i]), __uint_as_float(w[i]), s);
  return s;
}

// OCC: minimum waves per SIMD the register allocation must allow (launch bounds).
// FULLD: D == DPAD, so no fragment piece needs a column check.  The per-piece check costs
// 7 % at D=256 K=512 even when every piece passes it (profiles/r2_08_assign_clock_study.md).
// VARG (bf16): value-only argmin in the main loop -- 2 v_min3_u32 fold a tile's 4 scores
// into the running minimum and v_cmp + v_cndmask record the tile that lowered it (1.0 VALU
// per score instead of the packed keys' 1.5); the row inside the winning tile is recovered
// once per point after the loop by recomputing the winning tile's candidates on the
// matrix cores (bitwise the main loop's scores), right after the chunk loop.
// (A persistent grid that carried the next block's fragments across the epilogue measured
// 13-15 % slower -- the second register set spills at 4 waves/SIMD -- and was removed,
// profiles/r4_04_persistent_grid_ab.md.)
template <typename T, int DPAD, int P, int CT_ = 0, int NBUF_ = 2, int OCC = 1, int NW_ = 4, bool FULLD = false,
          bool VARG = false, int PMAJ = 0, bool TOP2 = false, bool XV = false>
__global__ __launch_bounds__(NW_ * 64, OCC) void assign16_kernel(AssignArgs a) {
  using C = Assign16Cfg<T, DPAD, P, CT_, NBUF_, NW_>;
  constexpr bool F32 = sizeof(T) == 4;
  // exact (value, index) epilogue: f32, or bf16 scores where the full pass ranks by value (XV)
  constexpr bool EXACT = F32 || XV;
  // A fragments streamed one at a time (see the MFMA issue): rows of 384..1024 features
  constexpr bool WIDE = DPAD > 256;
  static_assert(!(VARG && F32), "value-only argmin is the bf16 epilogue");
  static_assert(!(TOP2 && VARG), "bounded E-step: keys / exact epilogues");
  static_assert(!XV || (TOP2 && !F32), "the bf16 exact epilogue stands in for VARG in the bounded E-step");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const AssignLds<C> L(smem, a.Kpad);
  const int cn_bytes = L.cn_bytes(a.Kpad);
  char *cn_lds = L.cn, *bufs = L.ring;
  // Centre split (small N): grid.y splits the chunk range; each split leaves its
  // (value, index) in a.split_keys and split_finish_kernel writes the labels.
  const int nch_all = a.Kpad / (16 * C::CT);
  const int cps = (nch_all + (int)gridDim.y - 1) / (int)gridDim.y;
  const int c0 = (int)blockIdx.y * cps;
  const int nch = c0 + cps < nch_all ? c0 + cps : nch_all;  // one past this split's last chunk
  const int ncl = nch - c0;                                    // chunks of this split
  // LDS-DMA through buffer descriptors: the per-lane part is one 32-bit voffset (lane*16)
  // and every chunk / piece offset is a scalar, so no 64-bit VGPR address stays live
  // across the main loop (the f32 and D=128 bf16 bodies are register-bound).
  const uint32_t loff = (uint32_t)lane * 16u;
  const __amdgpu_buffer_rsrc_t rC = make_rsrc(a.Cpack, (uint32_t)a.Kpad * DPAD * sizeof(T));
  const __amdgpu_buffer_rsrc_t rN = make_rsrc(a.cn, (uint32_t)a.Kpad * 4u);
  auto issue_chunk = [&](int c, int slot) { ring_issue<C>(rC, bufs, slot, c0 + c, wid, loff); };   // slot c % NBUF

  // rows this launch assigns: N, or the device count of a compacted batch (wave-uniform;
  // a workgroup past it leaves before any barrier)
  const int64_t N = a.n_dev ? min(a.N, *a.n_dev) : a.N;
  if (a.n_dev && (int64_t)blockIdx.x * C::PTS >= N) return;
  const unsigned long long t_entry = a.timeline ? __builtin_amdgcn_s_memrealtime() : 0ull;
  const int64_t pbase = (int64_t)blockIdx.x * C::PTS + (int64_t)wid * (C::P * 16);
  u32x4 xr[C::P][C::NQ];
  float xnr[C::P];
  float osr[C::P];   // (a.oseed) the rows' full-pass seed offsets, at their X rows
  // The P blocks' fragment loads go out back to back: one memory round trip (two for a
  // gathered batch: the row indices first).  vmcnt retires in order, so a block whose
  // address waited on a load issued after the previous block's fragments (the row index,
  // or a row norm under a data-dependent branch) serialised the P round trips.
  auto row_of = [&](int p) -> int64_t {
    const int64_t row = pbase + p * 16 + r;
    return row < N ? row : (N - 1);
  };
  auto load_frags = [&](int p, int64_t src) {
    const T* rp = (const T*)a.X + src * a.ldx + g * C::V;
#pragma unroll
    for (int q = 0; q < C::NQ; ++q) {   // (FULLD: no column compare, see above)
      if constexpr (FULLD) xr[p][q] = *(const u32x4*)(rp + 4 * q * C::V);
      else xr[p][q] = load_piece<C::V>(rp, q, g, a.D);
    }
  };
  auto load_block = [&]() {   // fragments (+ caller norms) of the block at pbase
    if (a.rows) {   // gathered batch: logical row -> X row
      int64_t src[C::P];
#pragma unroll
      for (int p = 0; p < C::P; ++p) src[p] = a.rows[row_of(p)];
      __builtin_amdgcn_sched_barrier(0);   // all index loads in flight before the first use
#pragma unroll
      for (int p = 0; p < C::P; ++p) load_frags(p, src[p]);
      if (!F32 && a.xn && a.scatter) {   // (scattering: the caller's norms sit at the X rows)
#pragma unroll
        for (int p = 0; p < C::P; ++p) xnr[p] = a.xn[src[p]];
      }
      if (!F32 && a.oseed) {
#pragma unroll
        for (int p = 0; p < C::P; ++p) osr[p] = a.oseed[src[p]];
      }
    } else {
#pragma unroll
      for (int p = 0; p < C::P; ++p) load_frags(p, row_of(p));
      if (!F32 && a.oseed) {
#pragma unroll
        for (int p = 0; p < C::P; ++p) osr[p] = a.oseed[row_of(p)];
      }
    }
    if (!F32 && a.xn) {
      if (!(a.rows && a.scatter)) {
#pragma unroll
        for (int p = 0; p < C::P; ++p) xnr[p] = a.xn[row_of(p)];
      }
    } else {
#pragma unroll
      for (int p = 0; p < C::P; ++p) xnr[p] = 0.f;
    }
  };
  // Early prologue (one pass over plain full bf16 rows with caller norms): the |c|^2 DMA and
  // the norms go out first, then the fragments, the epilogue's reads and the first chunk, and
  // the seed-offset reduction waits for the norms alone -- its barrier runs while the fragments
  // are still in flight (the chunk loop's first wait retires them).  A/B switch V_ASSIGN_EARLY.
  constexpr int EJ = (C::P + 3) / 4;
  constexpr bool EARLY_OK = !F32 && FULLD && C::P * C::NQ + EJ + C::NPW < 64;   // (vmcnt range)
  const bool early = EARLY_OK && a.xn && !a.rows && !a.oseed && !a.split_keys && a.epi_prefetch &&
                     a.early_prologue;
  // early: lane (r, g) loads the norm of its epilogue rows only -- block p = 4j + g -- one
  // instruction per 4 blocks instead of one per block (the prologue's vector-memory issue is
  // what takes its time, profiles/r5_45_assign_prologue_study.md); lanes past the last block
  // repeat it (harmless to the max / min)
  // ... and with the per-fit table (a.gstats) the group's max / min |x|^2 come by scalar load: no reduction,
  // no exchange and no barrier stand between the norms' landing and the chunk loop
  constexpr bool TAB_OK = EARLY_OK && DPAD == 128 && C::PTS == GSTATS_ROWS && !VARG && !TOP2;   // (the headline geometry)
  const bool tab = TAB_OK && early && a.gstats;
  float gmax = 0.f, gmin = 3.0e38f;
  float xg[EJ];
  if (early) {
    if constexpr (TAB_OK) {
      if (tab) gstats_load(a.gstats, blockIdx.x, gmax, gmin);
    }
    cn_issue<C>(rN, cn_lds, cn_bytes, wid, loff);
#pragma unroll
    for (int j = 0; j < EJ; ++j) xg[j] = a.xn[row_of(4 * j + g < C::P ? 4 * j + g : C::P - 1)];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < C::P; ++p) load_frags(p, row_of(p));
    __builtin_amdgcn_sched_barrier(0);
  } else {
    load_block();
  }
  // (timeline) every row load issued: issue time vs landing time separates a full request
  // queue from memory latency
  const unsigned long long t_issued = a.timeline ? __builtin_amdgcn_s_memrealtime() : 0ull;
  // (one pass) the epilogue's per-row inputs, fetched with the fragments so their memory round
  // trip hides under the prologue's instead of opening the epilogue (~2 us of a workgroup's
  // ~50 us at D=128, scripts/assign_timeline.py): lane (r, g) stores the rows of the blocks
  // p = 4j + g, so it keeps their old label and caller norm -- two registers per 4 blocks
  int eold[EJ];
  float exn[EJ];
  const bool eread = !a.split_keys && a.epi_prefetch;
  if (eread) {
#pragma unroll
    for (int j = 0; j < EJ; ++j) {
      const int pg = 4 * j + g;
      const int64_t i = pbase + pg * 16 + r;
      const bool mine = pg < C::P && i < N;
      const int64_t oi = mine && a.scatter ? a.rows[i] : i;
      if (early) {   // (one load per j whatever the lane: the prologue's wait counts them)
        const int v = a.labels[i < N ? i : N - 1];
        eold[j] = mine && a.track_changed ? v : -2;
      } else {
        eold[j] = mine && a.track_changed ? a.labels[oi] : -2;
      }
      if (F32 || !a.xn) {
        exn[j] = mine && a.xn ? a.xn[oi] : 0.f;
      } else if (early) {   // (loaded per lane group above)
        exn[j] = xg[j];
      } else {   // (bf16: the prologue loaded them, xnr[p] = xn at block p's rows)
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * j + q < C::P && q == g) v = xnr[4 * j + q];
        exn[j] = v;
      }
    }
  }
  // per-wave (inertia, changed) totals, in LDS after the offsets
  double* wacc = L.wacc();
  {
    // |c|^2 and the first centre chunk by LDS-DMA, issued after the fragments so no wait for a
    // fragment address (the gathered row indices) also waits for them.
    __builtin_amdgcn_sched_barrier(0);
    if (!early) cn_issue<C>(rN, cn_lds, cn_bytes, wid, loff);
    issue_chunk(0, 0);
    unsigned long long t_frag = 0ull;
    if (early) {
      // the norms and |c|^2 landed; younger: the fragments, one label load per 4 blocks and
      // the first chunk (all issued unconditionally)
      if constexpr (EARLY_OK) wait_vmcnt<C::P * C::NQ + EJ + C::NPW>();
    } else {
      if (a.timeline) {   // (diagnostic: the fragments alone, the younger DMAs (<= 5 at Kpad <= 1024) may fly)
        wait_vmcnt<5>();
        t_frag = __builtin_amdgcn_s_memrealtime();
      }
      wait_vmcnt<0>();  // retire the fragments before the LDS-DMA loop (its vmcnt waits count chunks)
    }
    const unsigned long long t_landed = a.timeline ? __builtin_amdgcn_s_memrealtime() : 0ull;

    // bf16 seed offset (see the header): from the caller's row norms when given (loaded with the fragments)
    // or from the fragments.  Per-point offsets o_p = (1 + 2^-12) |x_p|^2 are parked in LDS and added to each
    // tile's seed (second chunk-loop instantiation); either way a key resolves 2^-17 (|x - c|^2 + 3 |x|^2).
    float off = 0.f;
    bool ppo = false;
    float *opt = L.opt(), *xnl = L.xnl();   // [NW][16][PP] offsets, |x|^2
    if (!a.xn && (!F32 || a.slots)) {
#pragma unroll
      for (int p = 0; p < C::P; ++p) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < C::NQ; ++q) s += sq16(xr[p][q], (T*)nullptr);
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        xnr[p] = s;
      }
      if (a.slots && g == 0) {   // no caller norms: the epilogue's inertia reads them back
#pragma unroll
        for (int p = 0; p < C::P; ++p) xnl[L.row(wid, r) + p] = xnr[p];
      }
    }
    if constexpr (!F32) {
     if (a.oseed) {
      // the offsets the full pass gives these rows (launch_seed_offsets), per point: the scores
      // -- and so the labels and near-tie decisions -- are bitwise the full pass's, whichever
      // workgroup a gathered row lands in (the bounded E-step's exactness)
      ppo = true;
      if (g == 0) {
#pragma unroll
        for (int p = 0; p < C::P; ++p) opt[L.row(wid, r) + p] = osr[p];
      }
     } else {
      float mnw = 3.0e38f;
      if (tab) {   // the table's pair is the reduction's result; this wave's own |c|^2 pieces landed (its wait above)
        off = gmax;
        mnw = gmin;
      } else {
      float m = 0.f, mn = 3.0e38f;
      if (early) {   // (one norm per lane and 4 blocks: reduce over the whole wave)
#pragma unroll
        for (int j = 0; j < EJ; ++j) { m = fmaxf(m, xg[j]); mn = fminf(mn, xg[j]); }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        mn = fminf(mn, __shfl_xor(mn, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        mn = fminf(mn, __shfl_xor(mn, 32, 64));
      } else {
#pragma unroll
        for (int p = 0; p < C::P; ++p) { m = fmaxf(m, xnr[p]); mn = fminf(mn, xnr[p]); }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        m = fmaxf(m, __shfl_xor(m, o, 64));
        mn = fminf(mn, __shfl_xor(mn, o, 64));
      }
      float* red = L.red();
      if (lane == 0) { red[2 * wid] = m; red[2 * wid + 1] = mn; }
      // every wave's |c|^2 DMA has landed (its wait above); a raw barrier, so an early
      // prologue's fragments and first chunk stay in flight (__syncthreads drains vmcnt)
      wait_lgkm0();
      raw_barrier();
#pragma unroll
      for (int w = 0; w < C::NW; ++w) { off = fmaxf(off, red[2 * w]); mnw = fminf(mnw, red[2 * w + 1]); }
      }
      // The seed rule; it stands again in assign16_persist_kernel, line for line but for the thread id and
      // the parking -- change both (as a function it moved every bf16 kernel's registers, profiles/r14_01).
      ppo = __builtin_amdgcn_readfirstlane((int)(off > 4.f * mnw)) != 0;
      if (!ppo) {
        off = seed_scale(off);
        off = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(off)));
        if (tab) cn_fold_own<C>(cn_lds, cn_bytes, wid, lane, off);
        else for (int k = threadIdx.x; k < a.Kpad; k += C::NW * 64) ((float*)cn_lds)[k] += off;
      } else {
        off = 0.f;
        if (early) {
#pragma unroll
          for (int j = 0; j < EJ; ++j)
            if (4 * j + g < C::P) opt[L.row(wid, r) + 4 * j + g] = seed_scale(xg[j]);
        } else if (g == 0) {
#pragma unroll
          for (int p = 0; p < C::P; ++p) opt[L.row(wid, r) + p] = seed_scale(xnr[p]);
        }
      }
     }
      // (published by the main loop's first wait_lgkm0 + barrier)
    }

    float best[C::P], seg_best[C::P];
    int bg[C::P];
    uint32_t vb[C::P], tb[C::P];   // VARG: running minimum (bits of a positive float), its tile
    // TOP2 (bounded E-step): this lane's second-smallest score (keys: index bits included,
    // <= 2^-17 relative -- the bounds' slack covers it), merged over lanes later; the smallest
    // is the epilogue's own running minimum (min(best, seg_best)).  Keys: the segment's own
    // second-smallest m2s rides along seg_best (one v_med3 + one v_min per key, no per-tile
    // merge with the global pair) and joins m2 at the segment's end -- 12 VALU per tile and
    // block instead of 16 (the gathered bounded assign is VALU-bound).
    float m2[C::P], m2s[C::P];
#pragma unroll
    for (int p = 0; p < C::P; ++p) {
      best[p] = 3.0e38f; seg_best[p] = 3.0e38f; bg[p] = 0;
      vb[p] = 0x7f7fffffu; tb[p] = 0u;
      m2[p] = 3.0e38f; m2s[p] = 3.0e38f;
    }
    const int ngrp = nch * C::CT;   // one past the last tile (global tile numbering)
    const unsigned kmask = key6_mask();

    // The chunk loop, instantiated twice: per-point offsets (PPO, outlier workgroups) seed a
    // tile's accumulators with its points' offsets; the common instantiation has no such
    // code at all -- a per-tile branch cost 1-3 % (one-process A/B against round 2).
    auto chunk_loop = [&](auto ppo_tag) {
      constexpr bool PPO = decltype(ppo_tag)::value;
      for (int c = 0; c < ncl; ++c) {
        wait_vmcnt<0>();   // chunk c landed
        wait_lgkm0();
        raw_barrier();  // RAW for chunk c, WAR for the slot refilled next (read at c-1)
        // (the next chunk's pieces all go out right after the barrier: spreading them one group
        // per tile after that tile's epilogue measured -2.5 % at D=128, -5 % at D=256 and far
        // slower at D=64, profiles/r3_28_ab_spread_dma.log)
        if (c + 1 < ncl) issue_chunk(c + 1, (c + 1) % C::NBUF);
        const char* buf = bufs + (c % C::NBUF) * C::CHUNK_BYTES;
        // A fragments + |c|^2 of a tile from the LDS ring
        auto load_a = [&](int tl_i, u32x4* aw_, f32x4& ci_) {
          const int tile = (c0 + c) * C::CT + tl_i;
          ci_ = *(const f32x4*)(cn_lds + (tile * 16 + 4 * g) * 4);
          const char* tl = buf + tl_i * C::TILE_BYTES + lane * 16;
          if constexpr (!WIDE) {   // (wide rows read their A fragments one at a time, below)
    #pragma unroll
            for (int q = 0; q < C::NQ; ++q) aw_[q] = *(const u32x4*)(tl + q * 1024);
          }
        };
        // A_AHEAD (bf16 D=64): the next tile's fragments are read right after this tile's
        // MFMAs are issued, so their LDS latency hides under the argmin epilogue (+2 % at D=64
        // in one-process A/B, profiles/r2_08_assign_clock_study.md; no gain at D=128)
        constexpr bool A_AHEAD = !F32 && DPAD == 64;
        u32x4 awe[C::NQ];
        f32x4 cie;
        if constexpr (A_AHEAD) load_a(0, awe, cie);
    #pragma unroll
        for (int tl_i = 0; tl_i < C::CT; ++tl_i) {
          const int tile = (c0 + c) * C::CT + tl_i;
          u32x4 aw[C::NQ];
          f32x4 ci;
          if constexpr (A_AHEAD) {
    #pragma unroll
            for (int q = 0; q < C::NQ; ++q) aw[q] = awe[q];
            ci = cie;
          } else {
            load_a(tl_i, aw, ci);
          }
          f32x4 acc[C::P];
          seed_tile<C, PPO ? 1 : 0>(acc, ci, opt + L.row(wid, r));
          mfma_priority<T, 1>();
          // per-block argmin epilogue (bf16): packed 6-bit keys or the value-only running minimum
          unsigned t0 = 0, t1 = 0, t2 = 0, t3 = 0;
          if constexpr (!EXACT && !VARG) key6_indices((unsigned)(tile & 15) << 2, t0, t1, t2, t3);
          auto epi = [&](int p) {
            if constexpr (VARG) {
              // scores are positive (seed offset, see the header), so they order as their bits;
              // a tie with the running minimum keeps the earlier tile (the lower index)
              const uint32_t u0 = __float_as_uint(acc[p][0]), u1 = __float_as_uint(acc[p][1]);
              const uint32_t u2 = __float_as_uint(acc[p][2]), u3 = __float_as_uint(acc[p][3]);
              const uint32_t nb = min(min(u0, u1), min(u2, min(u3, vb[p])));
              tb[p] = nb != vb[p] ? (uint32_t)tile : tb[p];
              vb[p] = nb;
            } else if constexpr (TOP2) {
              // the segment's sorted pair (seg_best, m2s): med3 (asm, see common.h) of it and a key is the new second
              const f32x4& sv = acc[p];
              const float k[4] = {pack_key6(sv[0], kmask, t0), pack_key6(sv[1], kmask, t1), pack_key6(sv[2], kmask, t2),
                                  pack_key6(sv[3], kmask, t3)};
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                m2s[p] = med3f(seg_best[p], m2s[p], k[e]);
                seg_best[p] = min2f(seg_best[p], k[e]);
              }
            } else {
              key6_fold(acc[p], kmask, t0, t1, t2, t3, seg_best[p]);
            }
          };
          if constexpr (WIDE) {
            // wide rows (DPAD > 256): one A fragment at a time, each against the P blocks --
            // all NQ of a tile would not fit in registers beside the rows.  The reads run WPF
            // fragments ahead of the MFMAs that use them, pinned in that order: left to the
            // scheduler, each read sat right before its P MFMAs behind an lgkmcnt(0), so one
            // wave per SIMD waited out every LDS round trip (bf16 D=512: 870 TF/s against
            // 1410 at D=256, profiles/r6_43_assign_sweep.log)
            const char* tl = buf + tl_i * C::TILE_BYTES + lane * 16;
            // (2 ahead where the rows leave room for 2 waves per SIMD under 256 VGPRs: bf16 D=384
            // at 4 ahead took 265 and ran 15 % slower at one wave, r6_44_ab_wide_d384_bf16.log;
            // 1 ahead for its bounded E-step, whose second-best keys spilled at 2)
            constexpr int WPF = C::NQ < 4 ? C::NQ : (C::P * C::NQ * 4 <= 192 ? (TOP2 && C::P == 4 ? 1 : 2) : 4);
            u32x4 aq[C::NQ];
#pragma unroll
            for (int q = 0; q < WPF; ++q) aq[q] = *(const u32x4*)(tl + q * 1024);
#pragma unroll
            for (int q = 0; q < C::NQ; ++q) {
              if (q + WPF < C::NQ) aq[q + WPF] = *(const u32x4*)(tl + (q + WPF) * 1024);
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int p = 0; p < C::P; ++p) acc[p] = Mfma16<T>::run(aq[q], xr[p][q], acc[p]);
              __builtin_amdgcn_sched_barrier(0);
            }
          } else {
            // The tile's MFMAs; the same text stands in assign16_persist_kernel's run_tile: change both (as a function it
            // put s_nops into the VARG loops).  PMAJ: each block's NQ back to back, pinned; else piece-major.
            if constexpr (PMAJ) {
#pragma unroll
              for (int p = 0; p < C::P; ++p)
#pragma unroll
                for (int q = 0; q < C::NQ; ++q) {
                  acc[p] = Mfma16<T>::run(aw[q], xr[p][q], acc[p]);
                  __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
              for (int q = 0; q < C::NQ; ++q)
#pragma unroll
                for (int p = 0; p < C::P; ++p) acc[p] = Mfma16<T>::run(aw[q], xr[p][q], acc[p]);
            }
          }
          mfma_priority<T, 0>();
          if constexpr (A_AHEAD) {
            if (tl_i + 1 < C::CT) load_a(tl_i + 1, awe, cie);
            __builtin_amdgcn_sched_barrier(0);
          }
          if constexpr (EXACT) {
            // (tile*4 + reg) as wave-uniform values: the index select needs no VALU add
            const int u = tile * 4;
#pragma unroll
            for (int p = 0; p < C::P; ++p) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if constexpr (TOP2) m2[p] = __builtin_amdgcn_fmed3f(best[p], m2[p], acc[p][e]);
                const bool lt = acc[p][e] < best[p];
                best[p] = lt ? acc[p][e] : best[p];
                bg[p] = lt ? u + e : bg[p];
              }
            }
          } else {
#pragma unroll
            for (int p = 0; p < C::P; ++p) epi(p);
          }
          if constexpr (!EXACT && !VARG) {
            if ((tile & 15) == 15 || tile == ngrp - 1) {
    #pragma unroll
              for (int p = 0; p < C::P; ++p) {
                if constexpr (TOP2) {   // the two sorted pairs -> the overall second-smallest key
                  m2[p] = min3f(m2[p], m2s[p], max2f(best[p], seg_best[p]));
                  m2s[p] = 3.0e38f;
                }
                key6_segment_merge(best[p], bg[p], seg_best[p], tile);
              }
            }
          }
        }
      }
    };
    const unsigned long long t_loop = a.timeline ? __builtin_amdgcn_s_memrealtime() : 0ull;
    if (ppo) chunk_loop(std::true_type{});
    else chunk_loop(std::false_type{});
    if (a.timeline && threadIdx.x == 0 && blockIdx.y == 0) {
      unsigned long long* tl = a.timeline + (int64_t)blockIdx.x * 8;
      tl[0] = t_entry;
      tl[1] = t_loop;
      tl[2] = __builtin_amdgcn_s_memrealtime();
      timeline_ids(tl);
      tl[6] = t_landed;  // fragments, |c|^2 and the first chunk landed (wave 0)
      tl[7] = early ? t_issued : t_frag;   // early prologue: the loads' issue completed; else
                                           // (Kpad <= 1024, 4 chunk pieces per wave) the fragments landed
    }

    // VARG: merge the 4 lane groups of each point on (value, tile, group) -- the centre index
    // 16 t + 4 g + e orders like that triple -- then recover e: for the points 4m..4m+3 the
    // 16 A rows carry the 4 candidates of each (row 4g'+e = candidate e of point 4m+g'), so
    // lane (r = 4m+g, g) receives its own point's 4 candidate scores, computed exactly as in
    // the main loop (same packed -2c, same seed from the LDS |c|^2 copy, same k-step order),
    // and takes the first that equals the minimum.  4 MFMA groups per point block: 64/K of
    // the main loop's matrix work.
    uint32_t kv[C::P];
    if constexpr (VARG) {
#pragma unroll
      for (int p = 0; p < C::P; ++p) {
        uint32_t v = vb[p], tg = tb[p] * 4u + (uint32_t)g;
        merge_groups(v, tg, ShflXor{});
        vb[p] = v;
        tb[p] = tg;
      }
      const T* pack = (const T*)a.Cpack;
      int efound[C::P];
#pragma unroll
      for (int p = 0; p < C::P; ++p) efound[p] = 0;
#pragma unroll
      for (int p = 0; p < C::P; ++p) {
        // MG candidate groups in flight at once (registers: MG * NQ fragments)
        constexpr int MG = C::NQ <= 2 ? 4 : 1;
#pragma unroll
        for (int m0 = 0; m0 < 4; m0 += MG) {
          u32x4 aw[MG][C::NQ];
          f32x4 acc[MG];
#pragma unroll
          for (int mi = 0; mi < MG; ++mi) {
            const int m = m0 + mi;
            const uint32_t tga = (uint32_t)__shfl((int)tb[p], 4 * m + (r >> 2), 64);
            const int ca = (int)(tga >> 2) * 16 + (int)(tga & 3u) * 4 + (r & 3);   // A row r's centre
            const T* src = pack + ((int64_t)(ca >> 4) * C::NQ * 64 + (ca & 15) + 16 * g) * C::V;
#pragma unroll
            for (int q = 0; q < C::NQ; ++q) aw[mi][q] = *(const u32x4*)(src + (int64_t)q * 64 * C::V);
            const uint32_t tgs = (uint32_t)__shfl((int)tb[p], 4 * m + g, 64);     // output rows' point
            acc[mi] = *(const f32x4*)(cn_lds + ((int)(tgs >> 2) * 16 + (int)(tgs & 3u) * 4) * 4);
            if (ppo) {
              seed_add(acc[mi], opt[L.row(wid, r) + p]);
            }
          }
#pragma unroll
          for (int mi = 0; mi < MG; ++mi) {
#pragma unroll
            for (int q = 0; q < C::NQ; ++q) acc[mi] = Mfma16<T>::run(aw[mi][q], xr[p][q], acc[mi]);
          }
#pragma unroll
          for (int mi = 0; mi < MG; ++mi) {
            if (r == 4 * (m0 + mi) + g) {
              int e = 3;
#pragma unroll
              for (int j = 2; j >= 0; --j) e = __float_as_uint(acc[mi][j]) == vb[p] ? j : e;
              efound[p] = e;
            }
          }
        }
      }
#pragma unroll
      for (int p = 0; p < C::P; ++p) {
        const int e = __shfl(efound[p], r + 16 * (r & 3), 64);
        kv[p] = (tb[p] >> 2) * 16u + (tb[p] & 3u) * 4u + (uint32_t)e;
      }
    }

    // The block's label epilogue.  Per point: the winning (score, centre) with the 4 lane
    // groups merged, then the label / distance stores and the inertia.
    auto merged = [&](int p, int& k, float& v) {
      if constexpr (VARG) {  // merged and recovered above
        k = (int)kv[p];
        v = __uint_as_float(vb[p]);
      } else {
        if constexpr (EXACT) {  // bg = tile * 4 + reg of the first strict minimum
          k = (bg[p] >> 2) * 16 + 4 * g + (bg[p] & 3);
          v = best[p];
        } else {               // bg = segment of 16 tiles, 6-bit key
          key6_decode(best[p], bg[p], g, v, k);
        }
        merge_groups(v, k, ShflXor{});
      }
    };
    float inert = 0.f;
    int changed = 0;
    const int64_t pcur = pbase;
    // TOP2: the second-smallest score of the point, merged over its 4 lane groups like the
    // winner (two sorted pairs -> their two smallest); every lane takes part (shuffles)
    auto second = [&](int p) -> float {
      float a1 = EXACT ? best[p] : fminf(best[p], seg_best[p]), a2 = m2[p];
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        const float b1 = __shfl_xor(a1, o, 64), b2 = __shfl_xor(a2, o, 64);
        const float n2 = fminf(fmaxf(a1, b1), fminf(a2, b2));
        a1 = fminf(a1, b1);
        a2 = n2;
      }
      return EXACT ? a2 : __uint_as_float(__float_as_uint(a2) & ~63u);
    };
    // ``oi``: where the row's outputs go (its row when a gathered batch scatters, else i);
    // ``old``: the row's previous label, ``xnv``: its caller norm (read by the caller of this
    // lambda, i < N, lanes with (p & 3) == g only); ``sec``: the second-smallest score (TOP2)
    auto store = [&](int p, int64_t oi, int k, float v, int old, float xnv, float sec) {
      const float offp = ppo ? opt[L.row(wid, r) + p] : off;   // the seed offset (0: f32)
      // inertia without caller norms: the prologue parked |x|^2 of the fragments in LDS
      const float xv = (a.slots && !a.xn) ? xnl[L.row(wid, r) + p] : xnv;
      if (a.split_keys) {
        // compare the (positive) keys across splits; split_finish undoes the offset
        // (parked in mind[], which the caller provides whenever xn is given)
        atomicMin(a.split_keys + oi, split_key(v, k));
        if (a.mind) a.mind[oi] = offp;
      } else {
        v -= offp;   // back to |c|^2 - 2 x.c
        if (a.track_changed) changed += (old != k);
        a.labels[oi] = k;
        if (a.xn || a.slots) {
          // fmaxf, not common.h clamp_d2: a NaN sum becomes 0 here on purpose.  inert goes
          // through slot_add's fixed-point digits, which cannot carry a NaN; the labels, mind
          // and inertia of rows with non-finite coordinates are unspecified (the transform and
          // top-m kernels are the ones that report such rows).  The same below.
          const float d = fmaxf(xv + v, 0.f);
          inert += d;
          if (a.mind) a.mind[oi] = d;
          if constexpr (TOP2) {   // Hamerly bounds: distances to the nearest and second nearest
            a.ub[oi] = __builtin_sqrtf(d);
            a.lb[oi] = __builtin_sqrtf(fmaxf(xv + (sec - offp), 0.f));
          }
        }
      }
    };
#pragma unroll
    for (int p = 0; p < C::P; ++p) {
      int k;
      float v;
      merged(p, k, v);
      float sec = 0.f;
      if constexpr (TOP2) sec = second(p);
      const int64_t i = pcur + p * 16 + r;
      if ((p & 3) == g && i < N) {
        const int64_t oi = a.scatter ? a.rows[i] : i;
        const bool rd = !a.split_keys;
        store(p, oi, k, v, eread ? eold[p >> 2] : (rd && a.track_changed ? a.labels[oi] : -2),
              eread ? exn[p >> 2] : (rd && a.xn ? a.xn[oi] : 0.f), sec);
      }
    }
    if (a.slots && !a.split_keys) {   // the wave's totals, in its LDS slot
      const double di = wave_sum((double)inert);
      const int dc = wave_sum(changed);
      if (lane == 0) { wacc[2 * wid] = di; wacc[2 * wid + 1] = (double)dc; }
    }
  }
  if (a.timeline && threadIdx.x == 0 && blockIdx.y == 0)
    a.timeline[(int64_t)blockIdx.x * 8 + 3] = __builtin_amdgcn_s_memrealtime();
  if (a.slots && !a.split_keys) {
    // the waves' LDS totals are published by a raw barrier: __syncthreads would first drain
    // vmcnt, i.e. wait for every label / distance store of the epilogue to be acknowledged
    wait_lgkm0();
    raw_barrier();
    if (threadIdx.x == 0) slot_add_totals<C>(wacc, a.slots + (blockIdx.x % NSLOT) * SLOT_STRIDE);
  }
}

// Persistent form of the plain full bf16 pass with caller norms (the early-prologue path of
// assign16_kernel, packed keys, 4 waves per ring, 2 ring slots): min(groups, resident
// workgroups) workgroups take PTS-row groups -- the row blocks blockIdx.x names in the one-pass
// grid -- from a group counter (a static stride left the workgroups whose waves share a SIMD
// twice as long in the chunk loop to finish a third of the kernel after the others), so every group's seed offset, per-point-offset
// decision, keys and slot addends are bitwise the one-pass kernel's.  A wave slot then never
// sits in a prologue: after the last tile's MFMAs of a group are issued the fragment registers
// are dead (the label epilogue reads best / bg / seg_best only), so the next group's norms and
// fragments load into the SAME registers (no second fragment set: that spilled,
// profiles/r4_04_persistent_grid_ab.md) and fly under the label epilogue, and the centre ring
// never drains -- chunk 0 of the next pass goes out at the last chunk's barrier.
// |c|^2 is re-sent to LDS per group behind the group-end barrier and the seed offset folded into
// it as in the one-pass kernel (adding the offset per tile instead, on a pristine copy, cost
// 4 VALU a tile: the SIMDs are bound by MFMA + VALU issue, not by waiting waves).
// vmcnt order per wave and group: [chunk 0] [old labels] [norms] [P*NQ fragments] [epilogue
// stores, slot atomics] [|c|^2] [thread 0: the group counter's atomic, behind chunk 0's barrier]
// [chunk 1] ...; the epilogue's wait for the old labels is counted on the norms
// and fragments (the only younger operations that are issued unconditionally).
// With the per-fit group statistics (AssignArgs::gstats) the group top has no reduction, no exchange
// and no barrier: the group's max / min |x|^2 arrive by scalar load, issued where the group became
// known, and each wave folds the offset into the |c|^2 pieces it sent itself (assign_step.h cn_fold_own).
// A kernel of its own, not a flag of assign16_kernel: the scope is one epilogue of that
// kernel's five, and tests/test_isa_guard.py indexes assign16_kernel's template arguments.
// Group counters of the persistent kernel, {next group - G, workgroups done}, zero between
// launches; launches rotate through the slots, so launches in flight on different streams do
// not share one.
constexpr int PERSIST_CTR_SLOTS = 64;
__device__ unsigned g_persist_ctr[PERSIST_CTR_SLOTS][2];

// lane ^ o shuffles on a laundered lane id ln (fresh_tid below): the library forms' addresses are
// loop invariants, which the compiler hoisted out of the group loop and spilled
struct ShflLaundered {
  int ln;
  __device__ __forceinline__ int operator()(int v, int o) const { return __builtin_amdgcn_ds_bpermute((ln ^ o) << 2, v); }
  __device__ __forceinline__ float operator()(float v, int o) const { return __int_as_float((*this)(__float_as_int(v), o)); }
};

template <int DPAD, int P, int OCC, int PMAJ>
__global__ __launch_bounds__(256, OCC) void assign16_persist_kernel(AssignArgs a, int ngroups, int cslot) {
  using T = uint16_t;
  using C = Assign16Cfg<T, DPAD, P, 0, 2, 4>;
  constexpr int EJ = (C::P + 3) / 4;
  static_assert(C::P * C::NQ + EJ < 64, "vmcnt range");
  static_assert(EJ == 1, "one norm and one old label per lane");
  static_assert(DPAD <= 256, "narrow rows");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const AssignLds<C> L(smem, a.Kpad);
  const int cn_bytes = L.cn_bytes(a.Kpad);
  char *cn_lds = L.cn, *bufs = L.ring;
  const int ncl = a.Kpad / (16 * C::CT);
  const uint32_t loff = (uint32_t)lane * 16u;
  const __amdgpu_buffer_rsrc_t rC = make_rsrc(a.Cpack, (uint32_t)a.Kpad * DPAD * sizeof(T));
  auto issue_chunk = [&](int c, int slot) { ring_issue<C>(rC, bufs, slot, c, wid, loff); };
  const int64_t N = a.N;
  float *red = L.red(), *opt = L.opt();
  double* wacc = L.wacc();
  uint32_t *xg_lds = L.xg(), *el_lds = L.old_labels();   // one norm, one old label per thread, landed by LDS-DMA
  const unsigned kmask = key6_mask();
  const int G = (int)gridDim.x;
  int grp = (int)blockIdx.x;   // the first group; the others come from the launch's group counter
  unsigned* ctr = g_persist_ctr[cslot];
  int* nxt_lds = L.next_group();   // the next group, handed from thread 0 to the workgroup
  int s0 = 0;   // ring slot of this pass's chunk 0 (alternates when a pass has an odd chunk count)

  // A lane's part of every row, norm and label address is one 32-bit offset inside the group
  // on a scalar base (the group's first row), so no 64-bit VGPR address lives across the
  // chunk loop.
  const uint32_t rowb = (uint32_t)a.ldx * (uint32_t)sizeof(T);
  auto rows_of = [&](int gi) -> int {   // valid rows of group gi
    const int64_t left = N - (int64_t)gi * C::PTS;
    return left < C::PTS ? (int)left : C::PTS;
  };
  // (group addresses are rebuilt from a laundered thread id where they are used: as loop
  // invariants the compiler hoisted them all out of the group loop and spilled them)
  auto fresh_tid = []() -> int {
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
  };
  auto lrow_of = [&](int tid, int p) -> int { return wid * (C::P * 16) + p * 16 + (tid & 15); };   // row in the group

  // The prefetched fragment loads are inline asm, tied to the registers that hold the current
  // fragments ("+v"): as compiler-visible loads the next group's fragments were given registers
  // of their own and spilled.  The compiler's wait-count pass does not see asm loads: the wait
  // before the group's first MFMA is this kernel's (the chunk loop's vmcnt(0)), and the waits
  // the compiler inserts for its own operations only get stricter (vmcnt retires in order).
  // Nothing else may touch those registers while a load is in flight -- no copy, no spill:
  // tests/test_isa_persist.py reads the code object for that.  The norms and the old labels
  // cross the group boundary through LDS (dword LDS-DMA), not in registers, for that reason:
  // a register-carried value the compiler was free to copy before it had landed.
  auto ld128 = [](u32x4& d, uint32_t vo, const void* base) {
    asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(d) : "v"(vo), "s"(base) : "memory");
  };
  // The group counter's returning atomic, inline asm tied to its register for the same reason: as a compiler-visible
  // atomicAdd on a uniform address it became a wave-aggregated atomic whose result a v_readfirstlane read at once,
  // behind a vmcnt(0) -- one exposed round trip per group wherever it stood.  Thread 0 calls it; a chunk head's
  // vmcnt(0) retires it before the last chunk's head reads `d` (tests/test_isa_persist_counter.py reads the code
  // object: one register at every site, untouched until that wait).
  auto fetch_add1 = [](unsigned& d, unsigned* counter) {
    asm volatile("global_atomic_add %0, %1, %2, %3 sc0" : "+v"(d) : "v"(0u), "v"(1u), "s"(counter) : "memory");
  };
  auto blds4 = [](__amdgpu_buffer_rsrc_t rs, MK_LDS void* lds_base, uint32_t voff) {   // lane i -> lds_base + 4 i
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, lds_base, 4, voff, 0, 0, 0);
  };

  u32x4 xr[C::P][C::NQ];
#pragma unroll
  for (int p = 0; p < C::P; ++p)
#pragma unroll
    for (int q = 0; q < C::NQ; ++q) xr[p][q] = u32x4{0u, 0u, 0u, 0u};
  // norms, |c|^2 and fragments of group gi, rows clamped to the group's last (a group past the
  // last: the last group's loads go out again, so the waits count the same on every path;
  // nothing reads them)
  auto load_group = [&](int gi) {
    gi = gi < ngroups ? gi : ngroups - 1;
    const int nv = rows_of(gi);
    const int64_t gb = (int64_t)gi * C::PTS;
    const char* xb = (const char*)a.X + gb * (int64_t)rowb;
    // lane (r, g): the norm of its epilogue rows, block p = g (descriptor: the group's valid rows)
    const __amdgpu_buffer_rsrc_t rXn = make_rsrc(a.xn + gb, (uint32_t)nv * 4u);
    __builtin_amdgcn_sched_barrier(0);
    const int tid = fresh_tid();
    const int gg = (tid & 63) >> 4;
    blds4(rXn, (MK_LDS void*)(xg_lds + wid * 64), (uint32_t)min(lrow_of(tid, gg < C::P ? gg : C::P - 1), nv - 1) * 4u);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < C::P; ++p) {
      const uint32_t vo = (uint32_t)min(lrow_of(tid, p), nv - 1) * rowb + (uint32_t)gg * 16u;
#pragma unroll
      for (int q = 0; q < C::NQ; ++q) ld128(xr[p][q], vo + (uint32_t)q * 64u, xb);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  if (a.timeline && threadIdx.x == 0) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    a.timeline[(int64_t)grp * 8] = t;
    a.timeline[(int64_t)grp * 8 + 7] = t;
  }
  // |c|^2 by LDS-DMA: the seed offset is folded into the LDS copy per group, so every group
  // starts from a fresh copy (4 KiB at K = 1024; a pristine second copy does not fit the LDS
  // of four workgroups)
  auto issue_cn = [&]() { cn_issue<C>(make_rsrc(a.cn, (uint32_t)a.Kpad * 4u), cn_lds, cn_bytes, wid, loff); };
  // With the per-fit table (a.gstats) a group's max / min |x|^2 is a scalar load, issued where the group
  // becomes known -- here, then at the last chunk's head for the next -- and read at the group's top.
  static_assert(C::PTS == GSTATS_ROWS, "the table's groups are this kernel's");
  const bool tab = a.gstats != nullptr;
  float gmax = 0.f, gmin = 3.0e38f;
  if (tab) gstats_load(a.gstats, grp, gmax, gmin);
  issue_cn();
  issue_chunk(0, 0);
  load_group(grp);
  for (;;) {
    const int nvc = rows_of(grp);   // this group's valid rows
    int nxt = 0;            // the group after this one (>= ngroups: none), known from the last chunk on
    bool has_next = false;
    // this group's norms and this wave's pieces of |c|^2 landed (the youngest operations: the
    // fragments, issued a whole label epilogue earlier, and the epilogue's stores retire with
    // them -- a stalled wave costs little here, the SIMD is kept busy by the other three)
    wait_vmcnt<0>();
    // (timeline: the stamps are stored as they are taken, none is carried in registers; word 0,
    // entry, is the previous group's exit, and word 7 repeats it: the group's loads were issued
    // under the previous group's epilogue)
    if (a.timeline && threadIdx.x == 0) a.timeline[(int64_t)grp * 8 + 6] = __builtin_amdgcn_s_memrealtime();
    float exn[EJ];   // the epilogue's norms (xg takes the next group's under the epilogue)
    exn[0] = __uint_as_float(xg_lds[fresh_tid()]);   // (this wave's own DMA, retired by the wait above)
    // seed offset, or per-point offsets, of this group: its own wave reduction, then the shared rule
    float off = 0.f;
    bool ppo = false;
    unsigned fetched;
    {
      const int ttid = fresh_tid();
      fetched = 0u;
      const int tln = ttid & 63, tr = ttid & 15, tg = tln >> 4;
      const ShflLaundered sh{tln};
      float mnw = 3.0e38f;
      if (tab) {
        // the table's pair is the reduction's result: no exchange, no barrier (the group-end barrier already
        // stands between every wave's last read of |c|^2 and its re-send; opt is each wave's own)
        off = gmax;
        mnw = gmin;
      } else {
      float m = 0.f, mn = 3.0e38f;
#pragma unroll
      for (int j = 0; j < EJ; ++j) { m = fmaxf(m, exn[j]); mn = fminf(mn, exn[j]); }
      m = fmaxf(m, sh(m, 16));
      mn = fminf(mn, sh(mn, 16));
      m = fmaxf(m, sh(m, 32));
      mn = fminf(mn, sh(mn, 32));
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        m = fmaxf(m, sh(m, o));
        mn = fminf(mn, sh(mn, o));
      }
      if (tln == 0) { red[2 * wid] = m; red[2 * wid + 1] = mn; }
      // every wave is past the previous group's chunk loop and label epilogue here: |c|^2,
      // the offsets and the wave totals in LDS may be rewritten behind this barrier
      wait_lgkm0();
      raw_barrier();
      // (every wave's |c|^2 pieces landed before the barrier above)
#pragma unroll
      for (int w = 0; w < C::NW; ++w) { off = fmaxf(off, red[2 * w]); mnw = fminf(mnw, red[2 * w + 1]); }
      }
      // The seed rule; it stands again in assign16_kernel, line for line but for thread id and parking: change both.
      ppo = __builtin_amdgcn_readfirstlane((int)(off > 4.f * mnw)) != 0;
      // (a one-chunk pass: its only chunk head consumes the next group, so the fetch goes out here and is
      // waited for at once -- on the way into either loop copy the compiler may move `fetched`)
      if (ncl < 2) {
        if (ttid == 0) fetch_add1(fetched, ctr);
        wait_vmcnt<0>();
      }
      if (!ppo) {
        off = seed_scale(off);
        off = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(off)));
        if (tab) cn_fold_own<C>(cn_lds, cn_bytes, wid, tln, off);
        else for (int kk = ttid; kk < a.Kpad; kk += C::NW * 64) ((float*)cn_lds)[kk] += off;
      } else {
        off = 0.f;
#pragma unroll
        for (int j = 0; j < EJ; ++j)
          if (4 * j + tg < C::P) opt[L.row(wid, tr) + 4 * j + tg] = seed_scale(exn[j]);
      }
    }

    float best[C::P], seg_best[C::P];
    int bg[C::P];
#pragma unroll
    for (int p = 0; p < C::P; ++p) { best[p] = 3.0e38f; seg_best[p] = 3.0e38f; bg[p] = 0; }

    // A chunk's barrier and ring refill; the pass's last chunk sends chunk 0 of the next pass
    // (the centres are the same every pass, so the ring never drains) and the label epilogue's
    // old labels, one chunk ahead of their use.
    auto chunk_head = [&](int c, auto last_tag) -> const char* {
      // chunk c landed (c = 0: and this group's fragments; the previous epilogue's stores are
      // the only younger operations, their number varies on a ragged tail)
      wait_vmcnt<0>();
      if constexpr (decltype(last_tag)::value) {
        if (fresh_tid() == 0) *nxt_lds = G + (int)fetched;   // (the atomic returned: the wait above)
      }
      wait_lgkm0();
      raw_barrier();  // RAW for chunk c, WAR for the slot refilled next (read at c-1)
      if constexpr (!decltype(last_tag)::value) {
        // the next group: one returning atomic per group, behind chunk 0's barrier -- chunk 1's wait retires it
        // with that chunk's own pieces (same round trip), and the last chunk's head consumes it.  (Ahead of
        // chunk 0's head it was the only operation that head waited for: a round trip for the whole workgroup.)
        if (c == 0) {
          if (fresh_tid() == 0) fetch_add1(fetched, ctr);
        }
        issue_chunk(c + 1, (s0 + c + 1) & 1);
      } else {
        nxt = __builtin_amdgcn_readfirstlane(*nxt_lds);
        has_next = nxt < ngroups;
        if (tab) gstats_load(a.gstats, nxt < ngroups ? nxt : ngroups - 1, gmax, gmin);
        if (has_next) issue_chunk(0, (s0 + c + 1) & 1);
        const int tid = fresh_tid();
        const __amdgpu_buffer_rsrc_t rLo = make_rsrc(a.labels + (int64_t)grp * C::PTS, (uint32_t)nvc * 4u);
        blds4(rLo, (MK_LDS void*)(el_lds + wid * 64), (uint32_t)min(lrow_of(tid, (tid & 63) >> 4), nvc - 1) * 4u);
      }
      return bufs + ((s0 + c) & 1) * C::CHUNK_BYTES;
    };
    // One tile.  PPO: 0 / 1 = without / with per-point offsets (two copies of the chunk loop, as
    // in assign16_kernel), 2 = decided at run time -- the pass's very last tile (FINAL), a single
    // copy, so the next group's loads stand once, in straight-line code right after the pass's
    // last MFMAs (in both copies of the loop, or under a branch of a shared body, the compiler
    // kept two fragment sets alive and spilled).
    auto run_tile = [&](int c, int tl_i, const char* buf, auto ppo_tag, auto final_tag) {
      constexpr int PPO = decltype(ppo_tag)::value;
      constexpr bool FINAL = decltype(final_tag)::value;
      const int tile = c * C::CT + tl_i;
      u32x4 aw[C::NQ];
      const f32x4 ci = *(const f32x4*)(cn_lds + (tile * 16 + 4 * g) * 4);
      const char* tl = buf + tl_i * C::TILE_BYTES + lane * 16;
#pragma unroll
      for (int q = 0; q < C::NQ; ++q) aw[q] = *(const u32x4*)(tl + q * 1024);
      f32x4 acc[C::P];
      seed_tile<C, PPO>(acc, ci, opt + L.row(wid, r), ppo);
      mfma_priority<T, 1>();
      unsigned t0 = 0, t1 = 0, t2 = 0, t3 = 0;
      key6_indices((unsigned)(tile & 15) << 2, t0, t1, t2, t3);
      // The tile's MFMAs; the same text stands in assign16_kernel's chunk loop: change both (as a function it
      // put s_nops into the VARG loops).  PMAJ: each block's NQ back to back, pinned; else piece-major.
      if constexpr (PMAJ) {
#pragma unroll
        for (int p = 0; p < C::P; ++p)
#pragma unroll
          for (int q = 0; q < C::NQ; ++q) {
            acc[p] = Mfma16<T>::run(aw[q], xr[p][q], acc[p]);
            __builtin_amdgcn_sched_barrier(0);
          }
      } else {
#pragma unroll
        for (int q = 0; q < C::NQ; ++q)
#pragma unroll
          for (int p = 0; p < C::P; ++p) acc[p] = Mfma16<T>::run(aw[q], xr[p][q], acc[p]);
      }
      mfma_priority<T, 0>();
      // the pass's last MFMAs are issued: the fragment registers take the next group's rows
      if constexpr (FINAL) load_group(nxt);
#pragma unroll
      for (int p = 0; p < C::P; ++p) key6_fold(acc[p], kmask, t0, t1, t2, t3, seg_best[p]);
      if (FINAL || (tile & 15) == 15) {
#pragma unroll
        for (int p = 0; p < C::P; ++p) key6_segment_merge(best[p], bg[p], seg_best[p], tile);
      }
    };
    auto chunk_loop = [&](auto ppo_tag) {
      for (int c = 0; c + 1 < ncl; ++c) {
        const char* buf = chunk_head(c, std::false_type{});
#pragma unroll
        for (int tl_i = 0; tl_i < C::CT; ++tl_i) run_tile(c, tl_i, buf, ppo_tag, std::false_type{});
      }
      const char* buf = chunk_head(ncl - 1, std::true_type{});
#pragma unroll
      for (int tl_i = 0; tl_i + 1 < C::CT; ++tl_i) run_tile(ncl - 1, tl_i, buf, ppo_tag, std::false_type{});
    };
    if (a.timeline && threadIdx.x == 0) a.timeline[(int64_t)grp * 8 + 1] = __builtin_amdgcn_s_memrealtime();
    if (ppo) chunk_loop(std::integral_constant<int, 1>{});
    else chunk_loop(std::integral_constant<int, 0>{});
    run_tile(ncl - 1, C::CT - 1, bufs + ((s0 + ncl - 1) & 1) * C::CHUNK_BYTES, std::integral_constant<int, 2>{},
             std::true_type{});
    if (a.timeline && threadIdx.x == 0) {
      unsigned long long* tl = a.timeline + (int64_t)grp * 8;
      tl[2] = __builtin_amdgcn_s_memrealtime();
      timeline_ids(tl);
    }

    // The group's label epilogue: assign16_kernel's, packed keys with caller norms
    float inert = 0.f;
    int changed = 0;
    // the old labels landed: younger are the next group's norms and fragments
    wait_vmcnt<EJ + C::P * C::NQ>();
    const int etid = fresh_tid();
    const int eold = (int)el_lds[etid];
    const int eln = etid & 63, er = etid & 15, eg = eln >> 4;
    const ShflLaundered esh{eln};
    // (descriptors over the group's valid rows: no store can leave them)
    const __amdgpu_buffer_rsrc_t rL = make_rsrc(a.labels + (int64_t)grp * C::PTS, (uint32_t)nvc * 4u);
    const __amdgpu_buffer_rsrc_t rM = make_rsrc(a.mind ? a.mind + (int64_t)grp * C::PTS : nullptr,
                                                a.mind ? (uint32_t)nvc * 4u : 0u);
#pragma unroll
    for (int p = 0; p < C::P; ++p) {
      int k;
      float v;   // (the one-pass kernel's decode and merge, on the laundered lane id)
      key6_decode(best[p], bg[p], eg, v, k);
      merge_groups(v, k, esh);
      const int lr = lrow_of(etid, p);
      if ((p & 3) == eg && lr < nvc) {
        const float offp = ppo ? opt[L.row(wid, er) + p] : off;
        v -= offp;   // back to |c|^2 - 2 x.c
        if (a.track_changed) changed += (eold != k);
        __builtin_amdgcn_raw_buffer_store_b32((unsigned)k, rL, (uint32_t)lr * 4u, 0, 0);
        const float d = fmaxf(exn[0] + v, 0.f);   // (fmaxf on purpose: see the epilogue above)
        inert += d;
        if (a.mind) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d), rM, (uint32_t)lr * 4u, 0, 0);
      }
    }
    if (a.slots) {   // the wave's totals, in its LDS slot
      // (wave_sum's butterflies, common.h)
      double di = (double)inert;
      int dc = changed;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const long long b = __double_as_longlong(di);
        const int lo = esh((int)(unsigned)b, o), hi = esh((int)(b >> 32), o);
        di += __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
        dc += esh(dc, o);
      }
      if (eln == 0) { wacc[2 * wid] = di; wacc[2 * wid + 1] = (double)dc; }
    }
    if (a.timeline && threadIdx.x == 0) {
      const unsigned long long t = __builtin_amdgcn_s_memrealtime();
      a.timeline[(int64_t)grp * 8 + 3] = t;
      if (has_next) {
        a.timeline[(int64_t)nxt * 8] = t;
        a.timeline[(int64_t)nxt * 8 + 7] = t;
      }
    }
    // group end: the wave totals are published and every wave is past its last read of |c|^2
    // (raw barrier: the label / distance stores and the next group's loads stay in flight)
    wait_lgkm0();
    raw_barrier();
    if (has_next) issue_cn();
    if (a.slots) {
      // one slot_add per group, the one-pass workgroup's addends and slot
      if (threadIdx.x == 0) slot_add_totals<C>(wacc, a.slots + (grp % NSLOT) * SLOT_STRIDE);
    }
    if (!has_next) break;
    grp = nxt;
    s0 = (s0 + ncl) & 1;
  }
  // the last group's prefetch (a repeat of the last group's rows, nothing reads it) may still
  // be in flight into the fragment registers, which the code below is free to reuse
  wait_vmcnt<0>();
  // every workgroup arrives here after its last fetch: the last one resets the counter pair,
  // inside the launch, so a captured graph replays without a host-side reset
  if (threadIdx.x == 0 && atomicAdd(ctr + 1, 1u) == (unsigned)G - 1u) {
    atomicExch(ctr, 0u);
    atomicExch(ctr + 1, 0u);
  }
}

// Centre-split epilogue: labels, squared distances, inertia and changed count from the
// per-point minimum key the splits left; resets every key for the next call.
__global__ __launch_bounds__(256) void split_finish_kernel(AssignArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float inert = 0.f;
  int changed = 0;
  if (i < a.N) {
    const unsigned long long key = a.split_keys[i];
    a.split_keys[i] = ~0ull;
    const int k = (int)(unsigned)key;
    const float v = split_value(key) - (a.mind ? a.mind[i] : 0.f);  // minus the parked seed offset
    if (a.track_changed) changed = a.labels[i] != k;
    a.labels[i] = k;
    if (a.xn) {
      const float d = fmaxf(a.xn[i] + v, 0.f);   // (fmaxf on purpose: see the assign epilogue)
      inert = d;
      if (a.mind) a.mind[i] = d;
    }
  }
  if (a.slots) {
    __shared__ double red[8];
    const double di = wave_sum((double)inert);
    const int dc = wave_sum(changed);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[2 * w] = di; red[2 * w + 1] = (double)dc; }
    __syncthreads();
    if (threadIdx.x == 0)
      slot_add((unsigned long long*)(a.slots + (blockIdx.x % NSLOT) * SLOT_STRIDE), red[0] + red[2] + red[4] + red[6],
               (long long)(red[1] + red[3] + red[5] + red[7]));
  }
}

// Splits of the centre range for N points: enough workgroups to fill the chip when the
// point blocks alone do not (a 1k-point batch is 4 workgroups streaming all of C).
static int assign16_splits(int64_t nblk, int nch) {
  if (nblk >= 1024 || nch <= 1) return 1;
  const int64_t want = (2048 + nblk - 1) / nblk;
  const int sp = (int)(want < nch ? want : nch);
  const int cps = (nch + sp - 1) / sp;
  return (nch + cps - 1) / cps;  // no empty split (the kernel's chunk range must be non-empty)
}

// Value-only argmin (VARG) where it pays: the D<=64 bf16 bodies are VALU-bound on the packed
// keys (2 MFMAs per tile and block at D=64, 1 at D=32, against 6 epilogue VALU), and the
// recovery pass costs 64/K of the matrix work, so it is taken for K >= 2048 at D=64 and
// K >= 1024 at D=32 (scripts/varg_ab.py, profiles/r3_08_varg_ab.log: cfg4 shape +8.2 %,
// D=64 K=2048 +8.5 %, K=1024 -3.7 %; D=32 K=1024 +5.6 %, K=512 -8.8 %).
// Variant V_ASSIGN_VARG = 0/1 forces it off / on (A/B, tests).

// The epilogue a launch runs, as a tag (assign16_kernel's trailing template arguments)
template <bool VARG_, int PMAJ_, bool TOP2_, bool XV_, bool FULLD_>
struct Epi {
  static constexpr bool VARG = VARG_, TOP2 = TOP2_, XV = XV_, FULLD = FULLD_;
  static constexpr int PMAJ = PMAJ_;
};

// One instantiation's launch; its LDS attribute is set once, at its first.
template <typename T, int DPAD, typename G, typename E>
static void launch_kernel(const AssignArgs& b, const dim3& grid, size_t lds, hipStream_t s) {
  constexpr auto fn =
      assign16_kernel<T, DPAD, G::P, G::CT, G::NBUF, G::OCC, G::NW, E::FULLD, E::VARG, E::PMAJ, E::TOP2, E::XV>;
  [[maybe_unused]] static const hipError_t attr =
      hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(fn, grid, dim3(G::NW * 64), lds, s, b);
}

// The geometries that run the bounded E-step's TOP2 epilogue (assign_geometry routes every call
// with bounds to them).  With a running (min, second) pair per point block the bf16
// defaults at D = 64 / 128 / 256 spilled 400-940 VGPRs and ran 5.7x slower
// (profiles/r4_05_hamerly_ab_top2_spills.log); the state is now the second minimum alone
// (profiles/r4_16_top2_register_study.md), and D = 256 keeps 3 blocks at 8 waves per ring.
template <typename T, int DPAD, typename G>
constexpr bool top2_geom() {
  if (sizeof(T) == 4 || DPAD == 32 || DPAD > 256) return true;   // (the defaults hold it, 0 spills)
  if (DPAD == 64) return (G::P == 2 || G::P == 4) && G::OCC == 4 && G::NW == 4;
  if (DPAD == 128) return (G::P == 2 || G::P == 4) && G::OCC == 4 && G::NW == 4;
  if (DPAD == 256) return G::P == 3 && G::OCC == 2 && G::NW == 8;
  return false;
}

static unsigned long long* g_timeline = nullptr;
static int64_t g_timeline_cap = 0;
void set_assign_timeline(unsigned long long* buf, int64_t capacity) {
  g_timeline = buf;
  g_timeline_cap = buf ? capacity : 0;
}

// The persistent kernel's grid: min(groups, workgroups resident at once) -- the occupancy of
// this instantiation at this LDS size times the device's CUs, both queried once and cached --
// or `cap` workgroups (tests: several groups per workgroup at small N).
template <int DPAD, int P, int OCC, int PMAJ>
static hipError_t launch16_persist(const AssignArgs& b, int64_t nblk, size_t lds, int cap, hipStream_t s) {
  const void* fn = (const void*)assign16_persist_kernel<DPAD, P, OCC, PMAJ>;
  static size_t occ_lds = 0;
  static int occ_blocks = 0;
  static int cus[64] = {};
  if (!occ_blocks || occ_lds != lds) {
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    int nb = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, lds);
    if (e != hipSuccess) return e;
    if (nb < 1) return hipErrorInvalidValue;
    occ_blocks = nb;
    occ_lds = lds;
  }
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidValue;
  if (!cus[dev]) {
    e = hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (cus[dev] < 1) return hipErrorInvalidValue;
  }
  int64_t grid = (int64_t)occ_blocks * cus[dev];
  if (cap > 0 && cap < grid) grid = cap;
  if (nblk < grid) grid = nblk;
  static int cslot = 0;
  cslot = (cslot + 1) % PERSIST_CTR_SLOTS;
  hipLaunchKernelGGL((assign16_persist_kernel<DPAD, P, OCC, PMAJ>), dim3((unsigned)grid), dim3(256), lds, s, b,
                     (int)nblk, cslot);
  return hipGetLastError();
}

// Where the persistent kernel runs by default: the shape whose one-process A/B against the
// one-pass grid it won -- bf16 D=128 K=1024 at N=1e8, 18.18 against 18.67 ms (+2.6 %, 11
// interleaved rounds; at N=2e7 +0.3 %, inside the noise: the ~40 us a launch's slowest
// workgroups finish after the rest weigh more on a 3.7 ms kernel) -- so from 5e7 rows up
// (profiles/r7_01_persistent_assign.md).  V_ASSIGN_PERSIST = 0 / 1 forces it off / on wherever
// it applies, >= 2 also caps its grid to that many workgroups (tests).
constexpr int PERSIST_KPAD = 1024;
constexpr int64_t PERSIST_MIN_GROUPS = 196608;

// A launch of geometry G (assign_geometry's Geom tag): grid, centre splits and LDS size, the persistent kernel
// or the one-pass grid, and each run-time epilogue flag resolved once -- a constant only where its kernels are
// built: VARG for bf16 at DPAD <= 64, PMAJ at DPAD <= 256, TOP2 on the top2_geom geometries, XV with TOP2.
template <typename T, int DPAD, typename G>
static hipError_t launch16(const AssignArgs& a, hipStream_t s) {
  using C = Assign16Cfg<T, DPAD, G::P, G::CT, G::NBUF, G::NW>;
  using L = AssignLds<C>;
  constexpr bool BF = sizeof(T) == 2;
  if (a.Kpad % (16 * C::CT) != 0) return hipErrorInvalidValue;
  static_assert(L::bytes(1024, true) <= 160 * 1024, "a built geometry holds 1024 centres, persistent extra included");
  const size_t lds = L::bytes(a.Kpad, false);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  const int64_t nblk = (a.N + C::PTS - 1) / C::PTS;
  if (nblk <= 0) return hipSuccess;
  // (bounded E-step: one-pass grid, keys or exact epilogue)
  const int splits = (a.split_keys && !a.ub && !a.n_dev) ? assign16_splits(nblk, a.Kpad / (16 * C::CT)) : 1;
  AssignArgs b = a;
  if ((a.ub != nullptr) != (a.lb != nullptr) || (a.scatter && !a.rows)) return hipErrorInvalidValue;
  if (splits == 1) b.split_keys = nullptr;
  const dim3 grid((unsigned)nblk, (unsigned)splits);
  if (g_timeline && nblk <= g_timeline_cap && splits == 1) b.timeline = g_timeline;
  b.epi_prefetch = variant(V_ASSIGN_EPI) != 0;
  b.early_prologue = variant(V_ASSIGN_EARLY) != 0;
  // Plain full bf16 passes with caller norms at the headline geometry (the conditions of the
  // one-pass kernel's early prologue, no device row count, point-block-major issue): the
  // persistent kernel (default: see PERSIST_MIN_GROUPS).
  if constexpr (BF && DPAD == 128 && G::P == 4 && G::CT == chunk_tiles16(2, 128) && G::NBUF == 2 && G::OCC == 4 &&
                G::NW == 4) {
    const int pv = variant(V_ASSIGN_PERSIST);
    const int pm = variant(V_ASSIGN_PMAJ);
    const bool applies = b.xn && !b.rows && !b.oseed && !b.split_keys && !b.n_dev && !b.ub && b.epi_prefetch &&
                         b.early_prologue && b.D == DPAD && (pm < 0 || pm == 1);
    const bool dflt = b.Kpad == PERSIST_KPAD && nblk >= PERSIST_MIN_GROUPS;
    const size_t plds = L::bytes(a.Kpad, true);   // + one old label per thread
    if (applies && plds <= 160 * 1024 && (pv >= 0 ? pv != 0 : dflt))
      return launch16_persist<DPAD, G::P, G::OCC, 1>(b, nblk, plds, pv >= 2 ? pv : 0, s);
  }
  constexpr bool VARG_OK = BF && DPAD <= 64;   // D=128: -12 % at K=1024, -4 % at 2048 (r3_11)
  constexpr bool PMAJ_OK = DPAD <= 256;        // (wider: streamed A fragments, one issue order)
  bool varg = false, pmaj = false;
  if constexpr (VARG_OK) {
    const int e = variant(V_ASSIGN_VARG);
    varg = e >= 0 ? e != 0 : a.Kpad >= (DPAD == 64 ? 2048 : 1024);
  }
  if constexpr (PMAJ_OK) {
    const int e = variant(V_ASSIGN_PMAJ);
    pmaj = (e >= 0 ? e : (BF ? 1 : 0)) != 0;
  }
  for_flag(b.D == DPAD, [&](auto fd) { return for_flag(varg, [&](auto vg) { return for_flag(pmaj, [&](auto pm) {
    constexpr bool FULLD = decltype(fd)::value, VARG = VARG_OK && decltype(vg)::value;
    constexpr int PMAJ = PMAJ_OK && decltype(pm)::value ? 1 : 0;
    if (!b.ub) launch_kernel<T, DPAD, G, Epi<VARG, PMAJ, false, false, FULLD>>(b, grid, lds, s);
    // With bounds (b.ub) the VARG flag says how the FULL pass of this shape ranks: by value (the
    // value-only argmin) -> the TOP2 kernel takes the exact (value, index) epilogue (XV), else the
    // packed keys; with the full pass's seed offsets (b.oseed) its labels are then the full pass's.
    else if constexpr (top2_geom<T, DPAD, G>())   // (else unreachable: assign_geometry sends bounds to one)
      launch_kernel<T, DPAD, G, Epi<false, PMAJ, true, VARG, FULLD>>(b, grid, lds, s);
    return 0;
  }); }); });
  if (splits > 1)
    hipLaunchKernelGGL(split_finish_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, s, b);
  return hipGetLastError();
}

// Point blocks per wave of the default geometries (assign_geometry, see there).
template <typename T, int DPAD>
constexpr int p_narrow() {
  return sizeof(T) == 2 ? (DPAD == 64 ? 8 : DPAD == 256 ? 3 : 4) : (DPAD / 4 / Elem<T>::V >= 8 ? 2 : 4);
}
template <typename T, int DPAD>
constexpr int p_wide() {
  return sizeof(T) == 2 ? (DPAD == 512 || DPAD == 1024 ? 3 : DPAD <= 512 ? 4 : 2) : (DPAD <= 512 ? 2 : 1);
}

// A launch geometry as compile-time tags: waves per ring, point blocks per wave, tiles per
// chunk, ring slots, waves per SIMD the registers must allow.  The workgroup's point count
// must divide parallel/shard.py ROW_ALIGN (1536).
template <int NW_, int P_, int CT_, int NBUF_, int OCC_>
struct Geom {
  static constexpr int NW = NW_, P = P_, CT = CT_, NBUF = NBUF_, OCC = OCC_;
  static constexpr int ROWS = NW * P * 16;
  static_assert(1536 % ROWS == 0, "workgroup points must tile the shard grid");
};

// Registers of rows per lane of a wide kernel: P blocks x NQ 16-B pieces x 4
template <typename T, int DPAD>
constexpr int C_wide_rows() {
  return p_wide<T, DPAD>() * (DPAD / 4 / Elem<T>::V) * 4;
}

// The one geometry choice of the assign: f(Geom) for a launch of (T, DPAD, Kpad), bounded
// (TOP2, the bounded E-step) or not, under the A/B switches V_ASSIGN_GEOM and
// V_ASSIGN_TOP2_GEOM.  launch_assign16 launches with it and assign16_block_rows returns its
// ROWS, so the row block a bf16 seed offset is taken over is the launched workgroup by
// construction (the bounded E-step's exactness rests on it: tests/test_gpu_bounded.py).
//
// Narrow rows (DPAD <= 256): 16 KiB chunks in a 2-slot ring.  A/B on MI355X (one process,
// interleaved rounds; round 1 profiles/r1_08_*, r1_16_*, r1_17_*, round 2
// profiles/r2_04_assign_ab.md):
//  * bf16 D=128: 4 point blocks per wave at <= 128 VGPRs (4 waves/SIMD) -- 3 / 5 / 6 / 8 blocks,
//    2-3 waves/SIMD, 8/16 waves per ring, 4/8 KiB chunks x 3 slots and next-tile fragment
//    loads under the MFMAs are all slower;
//  * bf16 D=64: 8 point blocks at 3 waves/SIMD, -5 % against 4 blocks at 4; with the
//    value-only argmin (K >= 2048) 4 blocks at 4 waves are 4-9 % slower and 12 blocks at
//    2 waves 1-10 % slower (profiles/r3_10_assign_p64_ab.log);
//  * bf16 D=256: 3 point blocks at 3 waves/SIMD, -4 % against 2 at 4; streamed A fragments
//    (3, 4 or 6 blocks) and a 3-slot ring were slower too (r4_04, r5_67), and were removed;
//  * f32: the register file sets 4 (D <= 64) or 2 blocks at one wave per SIMD minimum.
//
// Wide rows (DPAD 384..1024, e.g. sentence-embedding widths): one centre tile per chunk
// (12-32 KiB), and as many point blocks as ~256 registers of rows hold -- bf16 4 blocks at
// 384 features, 2 at 768, f32 2 and 1 -- at one wave per SIMD, or two where the kernel
// stays under 256 VGPRs (D=384, D=768).  bf16 D=512 takes 3 blocks (192 registers of rows,
// 2 waves/SIMD): +18 % at K=1024 and 4096, +26 % at K=256 against 4 blocks at one wave
// (profiles/r6_45_ab_d512_*.log); bf16 D=1024 takes 3 blocks at one wave (~450 VGPRs): +1.3 %
// at K=1024, +1.9 % at 4096 against 2 (profiles/r6_53_ab_*.log).  The fragment layout, the
// seed offsets and the argmin epilogue are the narrow kernels'; only the MFMA issue reads
// the A fragments one at a time (WIDE in assign16_kernel).
template <typename T, int DPAD, typename F>
static auto assign_geometry(int kpad, bool bounded, F&& f) {
  constexpr int CT = chunk_tiles16(sizeof(T), DPAD);
  constexpr bool BF = sizeof(T) == 2;
  if constexpr (DPAD > 256) {
    static_assert(CT == 1, "wide rows: one tile per chunk");
    // rows in <= 192 registers: hold the kernel to 2 waves/SIMD (the bounded E-step's D=384
    // build took 257 VGPRs without the bound)
    return f(Geom<4, p_wide<T, DPAD>(), CT, 2, (C_wide_rows<T, DPAD>() <= 192 ? 2 : 1)>{});
  } else {
    constexpr int P = p_narrow<T, DPAD>();
    constexpr int OCC = BF ? ((DPAD == 64 || DPAD == 256) ? 3 : 4) : 1;
    [[maybe_unused]] const int gm = variant(V_ASSIGN_GEOM);
    if constexpr (BF && (DPAD == 64 || DPAD == 128)) {
      // bounded: 4 point blocks per wave (the single-register TOP2 state: 0 / 14 spilled
      // VGPRs, the latter outside the MFMA loop); a 40-iteration bounded fit at N=2e7 D=128
      // K=1024 ran 6 % faster than with 2 blocks (profiles/r4_17_top2_geom_ab.md).  A/B switch
      // V_ASSIGN_TOP2_GEOM: 0 = 2 blocks
      if (bounded) {
        if (variant(V_ASSIGN_TOP2_GEOM) != 0) return f(Geom<4, 4, CT, 2, 4>{});
        return f(Geom<4, 2, CT, 2, 4>{});
      }
    }
    if constexpr (BF && DPAD == 256) {
      // 8 waves per ring (half the per-point centre stream and per-workgroup start-up), 3 point
      // blocks at 2 waves/SIMD: the bounded E-step's geometry, and A/B switch V_ASSIGN_GEOM = 1
      if (bounded || gm == 1) return f(Geom<8, 3, CT, 2, 2>{});
    }
    if constexpr (BF && DPAD == 128) {
      // A/B switch V_ASSIGN_GEOM: 1 = 8 waves share a ring of 32 KiB chunks (a barrier
      // every 8 tiles instead of 4; where Kpad is whole such chunks), 2 = 8 waves share the
      // 16 KiB ring.  K=1024: -0.4 % / +0.1 %; K=2048: +4.9 % / +4.4 %
      // (profiles/r3_21_ab_geom128.log), near-tie labels move with the workgroup's seed
      // offset; the headline's K=1024 keeps 4 waves.  A K sweep keeps 4 waves as the default:
      // 8-wave rings measured +5.0 % at K=2048 but -5.3 % at 3072 and -5.5 % at 4096
      // (profiles/r3_33_ab_geom128_ksweep.log).
      if (gm == 1 && kpad % (16 * 8) == 0) return f(Geom<8, P, 8, 2, OCC>{});
      if (gm == 2) return f(Geom<8, P, CT, 2, OCC>{});
    }
    return f(Geom<4, P, CT, 2, OCC>{});
  }
}

int assign16_chunk_tiles(int dtype, int dpad) { return plan::assign16_chunk_tiles(dtype == DT_BF16 ? 2 : 4, dpad); }
int assign_kpad(int dtype, int dpad, int K) { return plan::assign_kpad(dtype == DT_BF16 ? 2 : 4, dpad, K); }
int assign_cn_len(int kpad) { return plan::assign_cn_len(kpad); }

int assign16_block_rows(int dtype, int dpad, int kpad) {
  int rows = 0;   // (an unknown width)
  for_width(dtype, dpad, [&](auto t, auto w) {
    return assign_geometry<typename decltype(t)::type, decltype(w)::value>(kpad, false, [&](auto g) {
      rows = decltype(g)::ROWS;
      return 0;
    });
  });
  return rows;
}

hipError_t launch_assign16(int dtype, int dpad, const AssignArgs& a, hipStream_t s) {
  return (hipError_t)for_width(dtype, dpad, [&](auto t, auto w) {
    using T = typename decltype(t)::type;
    constexpr int DPAD = decltype(w)::value;
    return assign_geometry<T, DPAD>(a.Kpad, a.ub != nullptr,
                                    [&](auto g) { return launch16<T, DPAD, decltype(g)>(a, s); });
  });
}

}  // namespace mk
