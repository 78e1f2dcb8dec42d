// mikmeans — the fixed-point cell of the M-step (csrc/update.hip): two columns' sums in one u64.
//
// A contribution q = rne(x * w * 2^e_col), |q| <= 2^FX_BITS, is formed by ONE fma against the
// magic constant 1.5 * 2^23, whose result's bit pattern is 0x4B400000 + q; the bit patterns of
// two adjacent columns are added as one 64-bit integer.  Modulo 2^64 the cell then holds
//   sum(q_a) + sum(q_b) * 2^32 + n * 0x4B400000 * (1 + 2^32)
// where n is the number of adds since the cell was last zeroed (counted per label), and as long
// as |sum(q)| < 2^31 for both columns the two sums decode exactly: FX_LIM adds of |q| <= 2^20.
// Host and device, free of HIP types, so tests/native/fx_fuzz.cpp checks under
// g++ -fsanitize=address,undefined the integer rule every "bitwise identical for any atomic
// order, chunking or world size" claim rests on, and that FX_LIM is tight.
#pragma once
#include <stdint.h>

#include "plan.h"   // MK_HD_INLINE, plan::FX_BITS

namespace mk {

constexpr int FX_LIM = (1 << (30 - plan::FX_BITS)) * 2 - 1;  // adds per flush: 2047 * 2^20 < 2^31
constexpr float FX_MAGIC = 12582912.0f;                      // 1.5 * 2^23, bits 0x4B400000
constexpr unsigned long long FX_MM = 0x4B4000004B400000ull;  // the magic bits in both halves
constexpr float FX_QMAX = 1048576.f;                         // 2^FX_BITS
// nadd[k]: adds since label k's last flush in bits 0..30; bit 31 = "k's slab row already
// holds a partial sum" (then a flush adds instead of storing).
constexpr unsigned NADD_MASK = 0x7fffffffu, NADD_WRITTEN = 0x80000000u;

// 1.5*2^23 + rne(v * sc), unclamped; exact while |v * sc| <= 2^22
MK_HD_INLINE float fx_raw(float v, float sc) { return __builtin_fmaf(v, sc, FX_MAGIC); }
// One contribution pair from the bit patterns of its two columns' fx_raw values
MK_HD_INLINE unsigned long long fx_pair(uint32_t b0, uint32_t b1) {
  return (unsigned long long)b0 | ((unsigned long long)b1 << 32);
}

// The two column sums of a cell that took (nadd & NADD_MASK) pairs since it was zeroed
struct FxSums { int lo; long long hi; };
MK_HD_INLINE FxSums fx_decode(unsigned long long cell, unsigned nadd) {
  const unsigned long long T = cell - (unsigned long long)(nadd & NADD_MASK) * FX_MM;
  const int lo = (int)(uint32_t)T;
  const long long hi = (long long)(T - (unsigned long long)(long long)lo) >> 32;
  return {lo, hi};
}
// A count, or a decoded pair (its hi word when `both`), into the slab: stored by the label's
// first flush, added after
MK_HD_INLINE void fx_put(long long* dst, long long v, unsigned nadd) {
  if (nadd & NADD_WRITTEN) *dst += v; else *dst = v;
}
MK_HD_INLINE void fx_put(long long* dst, FxSums t, unsigned nadd, bool both = true) {
  if (nadd & NADD_WRITTEN) { dst[0] += t.lo; if (both) dst[1] += t.hi; }
  else { dst[0] = t.lo; if (both) dst[1] = t.hi; }
}

}  // namespace mk
