// From a runtime value to a template argument: the one way a launcher picks a kernel instantiation.  Plain C++17, no HIP
// (tests/test_dispatch_cpu.py compiles it with g++).
#pragma once
#include <type_traits>

// fd_pick<V0, V1, ...>(v, f): the first candidate equal to v -- f(std::integral_constant<decltype(Vk), Vk>{}) is called, once, and
// the result is true; no candidate equal to v -- nothing is called, false.  Inside f the argument converts to its value at compile
// time (`[&](auto M) { k<M()><<<...>>>(...); }`), and only the listed candidates are instantiated.  Pickers nest, one per template
// parameter.  A ladder's last `else` is a default: map the runtime value onto a candidate first
// (`const int nc = C <= 4 ? 4 : C <= 6 ? 6 : 8;` then fd_pick<4, 6, 8>(nc, ...)), so that a picker never falls through.
template <auto... Vs, typename T, typename F>
static inline bool fd_pick(T v, F &&f)
{
    return ((v == (T)Vs ? (f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
}
