// Host side of the launchers, shared by the GEMM and the attention families: a runtime choice -> template argument, and the opt-in
// for more dynamic LDS than the default limit.
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>

namespace pplhip {

// dispatch_int<A, B, C>(v, f) calls the generic lambda f with std::integral_constant<int, V> for the V of the list that equals v (the
// last one when none does: the ladders' final `else` -- a launcher checks its supported set BEFORE it dispatches), so only the listed
// values are instantiated.
template <int V> using int_c = std::integral_constant<int, V>;
template <int V0, int... Vs, class F>
inline void dispatch_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(int_c<V0>{});
    else if (v == V0) f(int_c<V0>{});
    else dispatch_int<Vs...>(v, f);
}

// Kernels that need more dynamic LDS than the default limit: `static LdsOptIn once; if (once.first()) set_max_lds(bytes, kernels...);`
// first() is true once per device (the attribute belongs to the function ON THE CURRENT DEVICE: one flag per device, or the other ranks
// of a single-process tensor-parallel run would launch without it)
struct LdsOptIn {
    bool done[64] = {false};
    bool first() {
        int dev = 0;
        (void)hipGetDevice(&dev);
        const bool f = !done[dev & 63];
        done[dev & 63] = true;
        return f;
    }
};
template <class... Ks>
inline void set_max_lds(size_t bytes, Ks... kernels) {
    ((void)hipFuncSetAttribute((const void*)kernels, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes), ...);
}

}  // namespace pplhip
