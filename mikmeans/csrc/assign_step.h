// mikmeans — the steps assign16_kernel and assign16_persist_kernel (csrc/assign16.hip) both take,
// defined once: the centre ring's DMA, the LDS layout, the seed scale, the packed-key tile step and
// the label decode.  Included by assign16.hip only: it compiles under that file's
// -fno-slp-vectorize, which the packed-seed hazard guard relies on (common.h seed_add).
// Throughout: lane = 16 g + r, wave wid of the workgroup's C::NW.
#pragma once
#include "common.h"
#include "plan.h"
#include "tile.h"   // Mfma16, the k-step
namespace mk {

// CT_: tiles per LDS chunk (0 = the 16 KiB default, which also fixes Kpad's
// granule); NBUF_: ring slots (prefetch depth NBUF-1; 2 -- the 3-slot forms measured slower).
template <typename T, int DPAD, int P_, int CT_ = 0, int NBUF_ = 2, int NW_ = 4>
struct Assign16Cfg {
  static constexpr int NW = NW_;                // waves per workgroup sharing the ring
  static constexpr int P = P_;                  // 16-point blocks per wave
  static constexpr int V = Elem<T>::V;
  static constexpr int NQ = DPAD / 4 / V;       // 16-B pieces per lane per point
  static constexpr int TILE_BYTES = NQ * 1024;  // 16 centroids x DPAD
  static constexpr int CT = CT_ ? CT_ : plan::chunk_tiles16(sizeof(T), DPAD);
  static constexpr int CHUNK_BYTES = CT * TILE_BYTES;
  static constexpr int PIECES = CHUNK_BYTES / 1024;
  static constexpr int NPW = PIECES / NW;
  static constexpr int PTS = NW * P * 16;
  static constexpr int PP = (P + 3) / 4 * 4;    // per-point offset slots per lane (LDS, f32x4 reads)
  static constexpr int OPT_BYTES = 2 * NW * 16 * PP * 4;   // offsets + gathered |x|^2
  static constexpr int NBUF = NBUF_;
  static_assert(NBUF == 2, "ring depth");
  static_assert(plan::chunk_tiles16(sizeof(T), DPAD) % CT == 0 || CT % plan::chunk_tiles16(sizeof(T), DPAD) == 0,
                "chunk and the Kpad granule must nest (a wider chunk runs only where Kpad is a multiple of it)");
  static_assert(NQ >= 1, "DPAD too small for the 16x16 layout");
  static_assert(PIECES % NW == 0, "chunk pieces must split evenly over waves");
};
// The dynamic LDS of a workgroup, for the host's size and both kernels' pointers:
//   |c|^2 [cn_bytes(Kpad)] | ring [NBUF chunks] | red | opt | xnl (= xg) | wacc | old labels
// red: a (max, min) |x|^2 pair per wave, then the persistent kernel's next-group word;
// opt / xnl: [NW][16][PP] f32 per-point seed offsets / |x|^2 of the fragments (no caller norms; the
// persistent kernel, which runs with caller norms only, lands a norm per thread there: xg);
// wacc: an (inertia, changed) f64 pair per wave; old labels: a word per thread, persistent only.
template <typename C>
struct AssignLds {
  static constexpr int RED = C::NBUF * C::CHUNK_BYTES;
  static constexpr int OPT = RED + 16 * C::NW;
  static constexpr int XNL = OPT + C::OPT_BYTES / 2;
  static constexpr int WACC = OPT + C::OPT_BYTES;
  static constexpr int OLD = WACC + 16 * C::NW;
  static constexpr int END = OLD, END_PERSIST = OLD + C::NW * 64 * 4;
  static_assert(RED % 16 == 0 && OPT % 16 == 0 && XNL % 16 == 0 && WACC % 16 == 0 && OLD % 16 == 0, "16-B regions");
  static_assert(16 * C::NW >= 2 * C::NW * 4 + 4 && C::OPT_BYTES / 2 >= C::NW * 64 * 4, "red holds the pairs and a word; xg fits xnl");
  MK_HD static constexpr int cn_bytes(int kpad) { return ((kpad * 4 + 1023) / 1024) * 1024; }
  MK_HD static constexpr size_t bytes(int kpad, bool persist) {
    return (size_t)cn_bytes(kpad) + (persist ? END_PERSIST : END);
  }
  char *cn, *ring;   // the |c|^2 copy (the seed offset folded in); the ring: chunk c of a pass in slot c % NBUF
  __device__ __forceinline__ AssignLds(char* smem, int kpad) : cn(smem), ring(smem + cn_bytes(kpad)) {}
  __device__ __forceinline__ float* red() const { return (float*)(ring + RED); }
  __device__ __forceinline__ int* next_group() const { return (int*)(red() + 2 * C::NW); }
  __device__ __forceinline__ float* opt() const { return (float*)(ring + OPT); }
  __device__ __forceinline__ float* xnl() const { return (float*)(ring + XNL); }
  __device__ __forceinline__ uint32_t* xg() const { return (uint32_t*)(ring + XNL); }
  __device__ __forceinline__ double* wacc() const { return (double*)(ring + WACC); }
  __device__ __forceinline__ uint32_t* old_labels() const { return (uint32_t*)(ring + OLD); }
  // a lane's row of opt / xnl: PP floats, 16-B aligned
  __device__ __forceinline__ static int row(int wid, int r) { return (wid * 16 + r) * C::PP; }
};
// Ring DMA.  Every lane of every wave calls these (wave wid sends the pieces wid, wid + NW, ..., lane i
// 16 B of each: loff = 16 i).  Nothing has landed on return: the caller's vmcnt wait retires this wave's pieces;
// a barrier after it makes the chunk (all of |c|^2) readable.  The slot written is past its last read (a barrier).
template <typename C>
__device__ __forceinline__ void ring_issue(__amdgpu_buffer_rsrc_t rC, char* ring, int slot, int chunk, int wid,
                                           uint32_t loff) {
  const uint32_t src = (uint32_t)chunk * C::CHUNK_BYTES;
  char* dst = ring + slot * C::CHUNK_BYTES;
#pragma unroll
  for (int i = 0; i < C::NPW; ++i) {
    const int pc = wid + i * C::NW;
    blds16(rC, (MK_LDS void*)(dst + pc * 1024), loff, src + (uint32_t)pc * 1024u);
  }
}
template <typename C>
__device__ __forceinline__ void cn_issue(__amdgpu_buffer_rsrc_t rN, char* cn_lds, int cn_bytes, int wid,
                                         uint32_t loff) {
  for (int pc = wid; pc < cn_bytes / 1024; pc += C::NW)
    blds16(rN, (MK_LDS void*)(cn_lds + pc * 1024), loff, (uint32_t)pc * 1024u);
}
// The bf16 seed scale, x (1 + 2^-12); the rule that uses it stays spelled at its two sites (see there)
__device__ __forceinline__ float seed_scale(float x) { return __builtin_fmaf(x, 2.44140625e-04f, x); }

// With the per-fit table (AssignArgs::gstats) a group's (max, min) |x|^2 is a scalar load -- gi is wave-uniform
// and the table read-only for the launch: the constant address space makes it SMEM, the pair lands in SGPRs.
__device__ __forceinline__ void gstats_load(const float* table, int64_t gi, float& mx, float& mn) {
  typedef float pair_t __attribute__((ext_vector_type(2)));
  const pair_t v = ((const __attribute__((address_space(4))) pair_t*)table)[gi];
  mx = v[0];
  mn = v[1];
}
// ... and each wave folds the seed offset into the |c|^2 pieces it sent itself (cn_issue: wid, wid + NW, ...;
// lane i 16 B of each), after its own vmcnt wait: no other wave's data is touched, so no barrier stands before
// it -- the first chunk's barrier publishes the folded copy with the chunk.
template <typename C>
__device__ __forceinline__ void cn_fold_own(char* cn_lds, int cn_bytes, int wid, int lane, float off) {
  for (int pc = wid; pc < cn_bytes / 1024; pc += C::NW) {
    f32x4* p = (f32x4*)(cn_lds + pc * 1024 + lane * 16);
    f32x4 v = *p;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += off;
    *p = v;
  }
}

// The tile step.  Every lane calls these, once per 16-centre tile, in this order.
// Seed the P accumulators with the tile's |c|^2 (ci: cn_lds rows 4 g .. 4 g + 3 of the tile).  PPO 1, or 2
// with ppo set at run time: plus the points' offsets (opt_row: the lane's row of opt, published by a barrier).
// Added BEFORE the MFMAs, which read them as src C: added to the MFMA results a v_pk_add_f32 read the registers
// early when the LDS read ahead of it returned fast -- a rare wrong label (test_gpu_kernels.py split-batch test).
template <typename C, int PPO>
__device__ __forceinline__ void seed_tile(f32x4 (&acc)[C::P], const f32x4& ci, const float* opt_row, bool ppo = false) {
#pragma unroll
  for (int p = 0; p < C::P; ++p) acc[p] = ci;
  if (PPO == 1 || (PPO == 2 && ppo)) {   // (one LDS read per tile)
#pragma unroll
    for (int p4 = 0; p4 < C::P; p4 += 4) {
      const f32x4 ov = *(const f32x4*)(opt_row + p4);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (p4 + j < C::P) seed_add(acc[p4 + j], ov[j]);
    }
  }
}
// bf16: the wave issues its MFMAs at raised priority and drops back for the epilogue, so a SIMD's arbiter
// feeds the matrix core before another wave's argmin VALU work (+0.3-5 %, profiles/r2_29_assign_setprio_ab.log).
// Nothing crosses either call; what the caller puts between <T, 1> and <T, 0> (key indices, MFMAs) runs raised.
template <typename T, int PRIO>
__device__ __forceinline__ void mfma_priority() {
  if constexpr (sizeof(T) == 2) {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(PRIO);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// 6-bit keys over a segment of 16 tiles (tile-in-segment * 4 + reg), merged with the segment id once per
// segment.  The tile's four indices as opaque SGPRs, so each key is one v_and_or_b32.  The caller writes out
// tis = (unsigned)(tile & 15) << 2: computed in a function it cost the chunk loops one more s_add per tile.
__device__ __forceinline__ void key6_indices(unsigned tis, unsigned& t0, unsigned& t1, unsigned& t2, unsigned& t3) {
  asm volatile("s_mov_b32 %0, %4\n\ts_or_b32 %1, %4, 1\n\ts_or_b32 %2, %4, 2\n\ts_or_b32 %3, %4, 3"
               : "=s"(t0), "=s"(t1), "=s"(t2), "=s"(t3) : "s"(tis) : "scc");  // s_or_b32 writes SCC
}
// A point's 4 scores of the tile as keys (kmask = key6_mask()), folded into the segment's minimum
__device__ __forceinline__ void key6_fold(const f32x4& sv, unsigned kmask, unsigned t0, unsigned t1, unsigned t2,
                                          unsigned t3, float& seg_best) {
  const float k0 = pack_key6(sv[0], kmask, t0), k1 = pack_key6(sv[1], kmask, t1);
  const float k2 = pack_key6(sv[2], kmask, t2), k3 = pack_key6(sv[3], kmask, t3);
  seg_best = min3f(min3f(k0, k1, k2), k3, seg_best);
}
// The end of a segment (its 16th tile, or the pass's last): the segment's minimum against the
// running best, by value only -- on equal (truncated) values the earlier segment keeps the lower
// centroid index (all keys are >= 0, see assign16.hip's header).
__device__ __forceinline__ void key6_segment_merge(float& best, int& bg, float& seg_best, int tile) {
  const float sv = __uint_as_float(__float_as_uint(seg_best) & ~63u);
  const float bv = __uint_as_float(__float_as_uint(best) & ~63u);
  if (sv < bv) { best = seg_best; bg = tile >> 4; }
  seg_best = 3.0e38f;
}
// The label decode.
// A lane's winning key -> (score with the seed offset still in it, centre): bg = the segment of
// 16 tiles, the key's low 6 bits = tile-in-segment * 4 + reg, the lane group g the row quad.
__device__ __forceinline__ void key6_decode(float best, int bg, int g, float& v, int& k) {
  const unsigned bits = __float_as_uint(best);
  const int idx = (int)(bits & 63u);
  k = (bg * 16 + (idx >> 2)) * 16 + 4 * g + (idx & 3);
  v = __uint_as_float(bits & ~63u);
}
// A point's 4 lane groups merged on (value, then lower index): every lane of the wave calls it
// and ends with the point's minimum.  sh(x, o) = x of lane ^ o.
template <typename V, typename K, typename Sh>
__device__ __forceinline__ void merge_groups(V& v, K& k, Sh sh) {
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const V vo = sh(v, o);
    const K ko = sh(k, o);
    if (vo < v || (vo == v && ko < k)) { v = vo; k = ko; }
  }
}
struct ShflXor {
  __device__ __forceinline__ float operator()(float v, int o) const { return __shfl_xor(v, o, 64); }
  __device__ __forceinline__ int operator()(int v, int o) const { return __shfl_xor(v, o, 64); }
  __device__ __forceinline__ uint32_t operator()(uint32_t v, int o) const { return (uint32_t)__shfl_xor((int)v, o, 64); }
};
// The waves' (inertia, changed) totals -- wacc[2 wid], wacc[2 wid + 1], stored by a lane of each and
// published by an lgkm wait + barrier -- as the workgroup's one slot_add (one thread calls it).
template <typename C>
__device__ __forceinline__ void slot_add_totals(const double* wacc, double* slot) {   // slot: group % NSLOT's
  double si = 0, sc = 0;
#pragma unroll
  for (int w = 0; w < C::NW; ++w) { si += wacc[2 * w]; sc += wacc[2 * w + 1]; }
  slot_add((unsigned long long*)slot, si, (long long)sc);
}
// (timeline) where the group ran: words 4 and 5 of its 8
__device__ __forceinline__ void timeline_ids(unsigned long long* tl) {
  tl[4] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));    // HW_ID
  tl[5] = (unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));   // XCC_ID
}

}  // namespace mk
