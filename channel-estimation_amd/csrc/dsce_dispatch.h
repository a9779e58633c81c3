// Run-time value -> template argument, for the launchers.  Each helper calls f
// with a compile-time constant c, which converts where a template argument is
// expected (k<c>), so the instances a launcher can reach are the values listed
// at its call site.  A nested dispatch reports its inner miss through a flag of
// the caller's:
//   bool hit = false;
//   for_value<16, 24>(mt, [&](auto MT) { hit = for_value<4, 8>(lg, [&](auto LG) { launch<MT, LG>(); }); });
#pragma once
#include <type_traits>
#include <utility>

namespace dsce {

// f(std::integral_constant<int, Vi>{}) for the listed value equal to v; returns
// whether one matched
template <int... Vs, class F>
inline bool for_value(int v, F&& f) {
    return ((v == Vs && (static_cast<void>(f(std::integral_constant<int, Vs>{})), true)) || ...);
}

// the same over Lo..Hi (both included)
template <int Lo, int Hi, class F>
inline bool for_range(int v, F&& f) {
    static_assert(Lo <= Hi, "for_range: empty range");
    if (v == Lo) return static_cast<void>(f(std::integral_constant<int, Lo>{})), true;
    if constexpr (Lo < Hi) return for_range<Lo + 1, Hi>(v, std::forward<F>(f));
    else return false;
}

// f(std::true_type{}) or f(std::false_type{})
template <class F>
inline void for_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace dsce
