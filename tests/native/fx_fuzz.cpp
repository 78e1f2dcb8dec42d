// Host sanitizer harness for the M-step's fixed-point cell, csrc/fx.h (built by
// tests/test_native_host.py with -fsanitize=address,undefined).  For n in {1, 2, FX_LIM - 1,
// FX_LIM} adds of contribution pairs at the bound (all +2^20, all -2^20, +2^20 beside -2^20 both
// ways) and uniformly random in [-2^20, 2^20], the pairs accumulated modulo 2^64 and decoded
// with n must give both column sums exactly; FX_LIM + 1 adds of +2^20 must not (the bound is
// tight); and one label flushed several times, stored by the first flush and added by the
// later ones, must total the same.  Prints "ok <cases>" or the first violation.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "fx.h"

using namespace mk;

static int fail(const char* what, long long a, long long b, long long c) {
  printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
  return 1;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {   // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
constexpr int QMAX = 1 << plan::FX_BITS;
static int rand_q() { return (int)(rng() % (2 * (uint64_t)QMAX + 1)) - QMAX; }

// The bit pattern the kernel's one fma leaves for the contribution q (the value q at scale 1)
static uint32_t bits_of(int q) {
  const float r = fx_raw((float)q, 1.0f);
  uint32_t b;
  memcpy(&b, &r, 4);
  return b;
}

struct Pattern { const char* name; int qa, qb; bool random; };
static const Pattern PATTERNS[] = {{"all +2^20", QMAX, QMAX, false},   {"all -2^20", -QMAX, -QMAX, false},
                                   {"+2^20 | -2^20", QMAX, -QMAX, false}, {"-2^20 | +2^20", -QMAX, QMAX, false},
                                   {"random", 0, 0, true}};

// n pairs of one pattern into a zeroed cell; whether decoding with n gives both sums
static bool exact(const Pattern& p, int n) {
  unsigned long long cell = 0;
  long long sa = 0, sb = 0;
  for (int i = 0; i < n; ++i) {
    const int qa = p.random ? rand_q() : p.qa, qb = p.random ? rand_q() : p.qb;
    cell += fx_pair(bits_of(qa), bits_of(qb));
    sa += qa;
    sb += qb;
  }
  // (the "slab row written" bit of the add count must not reach the decode)
  const FxSums t = fx_decode(cell, (unsigned)n), tw = fx_decode(cell, (unsigned)n | NADD_WRITTEN);
  return t.lo == sa && t.hi == sb && tw.lo == sa && tw.hi == sb;
}

int main() {
  long long cases = 0;
  static_assert(FX_LIM == 2047 && FX_QMAX == (float)QMAX, "the bound the comments argue");
  for (int q : {0, 1, -1, QMAX, -QMAX, 4 * QMAX, -4 * QMAX}) {   // the magic-constant encode, to 2^22
    if (bits_of(q) != 0x4B400000u + (uint32_t)q) return fail("encode", q, bits_of(q), 0);
    ++cases;
  }
  if (fx_pair(0x4B400000u, 0x4B400000u) != FX_MM) return fail("FX_MM", 0, 0, 0);
  for (const Pattern& p : PATTERNS)
    for (int n : {1, 2, FX_LIM - 1, FX_LIM})
      for (int trial = 0; trial < (p.random ? 200 : 1); ++trial, ++cases)
        if (!exact(p, n)) return fail(p.name, n, trial, 0);
  // FX_LIM is tight: one more add of +2^20 reaches 2^31 and wraps
  if (exact(PATTERNS[0], FX_LIM + 1)) return fail("FX_LIM + 1 adds of +2^20 decoded", FX_LIM + 1, 0, 0);
  ++cases;

  // One label through several flushes: cell and add count as the kernels keep them in LDS, the
  // slab words and the count word uninitialised memory (here: garbage) until the first flush.
  for (int trial = 0; trial < 300; ++trial, ++cases) {
    const Pattern& p = PATTERNS[trial % 5];
    const bool both = trial % 7 != 0;   // (an odd last column: the hi word is not the label's)
    const int rows = 1 + (int)(rng() % (5 * FX_LIM));
    unsigned long long cell = 0;
    unsigned nadd = 0;
    long long slab[2] = {0x0123456789abcdefll, -0x0fedcba987654321ll}, cnt = 0x5555555555555555ll;
    const long long hi0 = slab[1];
    long long sa = 0, sb = 0;
    int flushes = 0;
    int next = 1 + (int)(rng() % FX_LIM);   // flush when the add count reaches this (<= FX_LIM)
    for (int i = 0; i < rows; ++i) {
      const int qa = p.random ? rand_q() : p.qa, qb = p.random ? rand_q() : p.qb;
      cell += fx_pair(bits_of(qa), bits_of(qb));
      ++nadd;
      sa += qa;
      sb += qb;
      if ((int)(nadd & NADD_MASK) >= next || i == rows - 1) {
        fx_put(slab, fx_decode(cell, nadd), nadd, both);
        fx_put(&cnt, (long long)(nadd & NADD_MASK), nadd);
        cell = 0;
        nadd = NADD_WRITTEN;
        next = 1 + (int)(rng() % FX_LIM);
        ++flushes;
      }
    }
    if (slab[0] != sa || slab[1] != (both ? sb : hi0) || cnt != rows) return fail("store then add", trial, rows, flushes);
  }
  printf("ok %lld\n", cases);
  return 0;
}
