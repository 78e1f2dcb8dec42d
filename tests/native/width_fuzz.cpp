// Host sanitizer harness for the (dtype, padded width) dispatch of csrc/dispatch.h (built by
// tests/test_native_host.py with -fsanitize=address,undefined).  For both element sizes,
// for_width must reach a case -- with the matching type and width tags -- for exactly the
// widths plan::assign_dpad returns over D = 1..1024, and refuse every other width in 1..2048;
// for_value must do the same for an explicit list of values; for_type must reach one type tag for
// every dtype value, and for_flag the constant of its flag.  Prints "ok <cases>" or the first
// violation.
#include <stdio.h>

#include <set>

#include "dispatch.h"

static int fail(const char* what, long long a, long long b, long long c) {
  printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
  return 1;
}

int main() {
  long long cases = 0;
  for (int es : {2, 4}) {
    const int dtype = es == 2 ? mk::WIDTH_BF16 : 0;
    std::set<int> widths;
    for (int D = 1; D <= 1024; ++D) {
      const int w = mk::plan::assign_dpad(es, D);
      if (w < D) return fail("assign_dpad below D", es, D, w);
      widths.insert(w);
    }
    for (int dpad = 1; dpad <= 2048; ++dpad) {
      int calls = 0, got_es = 0, got_w = 0;
      const int r = mk::for_width(dtype, dpad, [&](auto t, auto w) {
        ++calls;
        got_es = (int)sizeof(typename decltype(t)::type);
        got_w = decltype(w)::value;
        return 0;
      });
      ++cases;
      if (widths.count(dpad)) {
        if (r != 0 || calls != 1) return fail("width not reached", es, dpad, r);
        if (got_es != es || got_w != dpad) return fail("wrong tags", es, dpad, got_w);
      } else if (r != 1 || calls != 0) {   // (1 = hipErrorInvalidValue)
        return fail("width not refused", es, dpad, r);
      }
    }
    // a case's own result comes back unchanged
    if (mk::for_width(dtype, *widths.begin(), [](auto, auto) { return 7; }) != 7) return fail("result", es, 0, 0);
  }
  // for_value: every value of a list reaches its case once, with its tag; every other value in
  // a window around the list is refused without a call
  const std::set<int> list = {0, 1, 2, 3, 8, 12, 32, 38, 64, 192, 196};
  for (int v = -64; v <= 320; ++v) {
    int calls = 0, got = -1000;
    const int r = mk::for_value<0, 1, 2, 3, 8, 12, 32, 38, 64, 192, 196>(v, [&](auto t) {
      ++calls;
      got = decltype(t)::value;
      return 0;
    });
    ++cases;
    if (list.count(v) ? (r != 0 || calls != 1 || got != v) : (r != 1 || calls != 0))
      return fail(list.count(v) ? "value not reached" : "value not refused", v, r, calls);
  }
  if (mk::for_value<5, 9>(9, [](auto) { return 7; }) != 7) return fail("value result", 9, 0, 0);
  // for_type: every dtype around the two real ones reaches exactly one type tag, bf16 for
  // WIDTH_BF16 and float otherwise (for_width's reading), and dtype_vec is that type's 16-byte piece
  for (int dtype = -8; dtype <= 8; ++dtype) {
    int calls = 0, got_es = 0;
    const int r = mk::for_type(dtype, [&](auto t) {
      ++calls;
      got_es = (int)sizeof(typename decltype(t)::type);
      return 0;
    });
    int width_es = 0;   // (256 is a width of both types)
    mk::for_width(dtype, 256, [&](auto t, auto) { return width_es = (int)sizeof(typename decltype(t)::type), 0; });
    ++cases;
    if (r != 0 || calls != 1 || got_es != (dtype == mk::WIDTH_BF16 ? 2 : 4) || got_es != width_es)
      return fail("type tag", dtype, got_es, calls);
    if (mk::dtype_vec(dtype) * got_es != 16) return fail("dtype_vec", dtype, mk::dtype_vec(dtype), got_es);
  }
  if (mk::for_type(mk::WIDTH_BF16, [](auto) { return 7; }) != 7) return fail("type result", 0, 0, 0);
  // for_flag: each flag reaches exactly its constant
  for (int b = 0; b < 2; ++b) {
    int calls = 0, got = -1;
    const int r = mk::for_flag(b != 0, [&](auto f) {
      ++calls;
      got = decltype(f)::value ? 1 : 0;
      return 0;
    });
    ++cases;
    if (r != 0 || calls != 1 || got != b) return fail("flag constant", b, got, calls);
  }
  if (mk::for_flag(true, [](auto) { return 7; }) != 7) return fail("flag result", 0, 0, 0);
  printf("ok %lld\n", cases);
  return 0;
}
