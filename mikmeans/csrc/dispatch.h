// mikmeans — the one (dtype, padded width) dispatch of the MFMA distance kernels, and the dtype,
// flag and value dispatches of every other launcher.
//
// Host only and free of HIP types, like plan.h, so tests/native/width_fuzz.cpp builds it with
// g++ -fsanitize=address,undefined.  There is no width list here: a kernel is instantiated for
// exactly the widths plan::assign_dpad pads a row to, so a new row width is added there alone.
// A launcher hands for_width a generic functor:
//
//   return (hipError_t)for_width(dtype, dpad, [&](auto t, auto w) {
//     return launch<typename decltype(t)::type, decltype(w)::value>(args, stream);
//   });
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "plan.h"

namespace mk {

constexpr int WIDTH_BF16 = 1;    // kernels.h DT_BF16 (static_assert there); any other dtype is f32
constexpr int WIDTH_MAX = 1024;  // the widest row of plan::assign_dpad
static_assert(plan::assign_dpad(4, WIDTH_MAX) == WIDTH_MAX && plan::assign_dpad(4, WIDTH_MAX + 1) == 0 &&
                  plan::assign_dpad(2, WIDTH_MAX) == WIDTH_MAX && plan::assign_dpad(2, WIDTH_MAX + 1) == 0,
              "WIDTH_MAX is plan::assign_dpad's widest row");

template <typename T> struct TypeTag { using type = T; };
template <int W> using WidthTag = std::integral_constant<int, W>;

namespace detail {
// (every padded width is a multiple of 16 elements: one 16-B piece per lane group of f32)
template <typename T, int W, typename F>
inline bool width_case(int dpad, F& f, int& r) {
  if constexpr (plan::assign_dpad(sizeof(T), W) == W) {
    if (dpad == W) {
      r = (int)f(TypeTag<T>{}, WidthTag<W>{});
      return true;
    }
  }
  return false;
}
template <typename T, typename F, size_t... I>
inline int for_width_in(int dpad, F& f, std::index_sequence<I...>) {
  int r = 1;   // hipErrorInvalidValue
  (void)(width_case<T, 16 * (int)(I + 1)>(dpad, f, r) || ...);
  return r;
}
}  // namespace detail

// f(TypeTag<T>, WidthTag<DPAD>) for the row type and padded width of (dtype, dpad), and its
// result (a hipError_t, or 0); hipErrorInvalidValue (1) for a width no kernel is built for.
template <typename F>
inline int for_width(int dtype, int dpad, F&& f) {
  constexpr auto seq = std::make_index_sequence<WIDTH_MAX / 16>{};
  if (dtype == WIDTH_BF16) return detail::for_width_in<uint16_t>(dpad, f, seq);
  return detail::for_width_in<float>(dpad, f, seq);
}

// The row type alone: f(TypeTag<T>{}) and its result, bf16 for WIDTH_BF16 and float for any other
// dtype, as for_width reads it.  And a run-time flag as a constant: f(std::bool_constant<B>{}).
template <typename F>
inline int for_type(int dtype, F&& f) {
  if (dtype == WIDTH_BF16) return (int)f(TypeTag<uint16_t>{});
  return (int)f(TypeTag<float>{});
}
template <typename F>
inline int for_flag(bool b, F&& f) {
  if (b) return (int)f(std::bool_constant<true>{});
  return (int)f(std::bool_constant<false>{});
}
// Elements of a 16-byte piece of a row of that type (common.h Elem<T>::V, for host code).
constexpr int dtype_vec(int dtype) { return dtype == WIDTH_BF16 ? 8 : 4; }

// The same for one run-time value out of an explicit list: f(std::integral_constant<int, V>{})
// for the V that equals v, and its result; hipErrorInvalidValue (1), without calling f, for a
// value not in the list -- the list is what gets built.
template <int... V, typename F>
inline int for_value(int v, F&& f) {
  int r = 1;
  (void)((v == V && ((r = (int)f(std::integral_constant<int, V>{})), true)) || ...);
  return r;
}

}  // namespace mk
