// Run-time values -> template arguments, and the one kernel launch, for the launchers of every unit.  A launcher nests the
// dispatches it needs around one generic lambda and ends in launch(); the thresholds that pick a KMAX or a G stay in the launcher.
//   dispatch_io(io_dtype, f)              f(type_tag<float>{}) or f(type_tag<double>{})
//   dispatch_int_last<A, B, C>(id, f)     f(int_tag<ID>{}) for the listed id; C serves every unlisted id
//   dispatch_int_or<A, B, C>(id, r, f)    ... ; an unlisted id returns r
// The dispatches need no HIP (tests/cpp/dispatch_routing.cpp runs them on the host); launch() exists under hipcc only.
#pragma once
#include <cstddef>
#include <type_traits>

#include "../../include/safe_control_amd.h"

namespace sc {

template <typename T>
struct type_tag { using type = T; };
template <typename TAG>
using tag_t = typename TAG::type;
template <int V>
using int_tag = std::integral_constant<int, V>;

template <typename F>
inline auto dispatch_io(int io_dtype, F&& f) {
    if (io_dtype == SC_DTYPE_F32) return f(type_tag<float>{});
    return f(type_tag<double>{});
}

template <int ID, int... REST, typename F>
inline auto dispatch_int_last(int id, F&& f) {
    if constexpr (sizeof...(REST) == 0) return f(int_tag<ID>{});
    else {
        if (id == ID) return f(int_tag<ID>{});
        return dispatch_int_last<REST...>(id, f);
    }
}

template <int ID, int... REST, typename R, typename F>
inline R dispatch_int_or(int id, R unlisted, F&& f) {
    if (id == ID) return f(int_tag<ID>{});
    if constexpr (sizeof...(REST) > 0) return dispatch_int_or<REST...>(id, unlisted, f);
    else return unlisted;
}

#ifdef __HIPCC__
// the caller's untyped pointers become the kernel's own parameter types; everything else converts implicitly
template <typename P, typename A>
inline P kernel_arg(const A& a) {
    if constexpr (std::is_pointer_v<P> && std::is_pointer_v<A>) return static_cast<P>(a);
    else return a;
}

// Dynamic LDS above 64 KiB needs the attribute; it is per device, so it is set on every such call.  RAISE_LDS = false is for the
// kernels whose launchers never set it.
template <bool RAISE_LDS = true, typename... P, typename... A>
inline hipError_t launch(void (*kern)(P...), dim3 blocks, dim3 threads, size_t lds_bytes, hipStream_t stream, const A&... args) {
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    if (RAISE_LDS && lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, blocks, threads, lds_bytes, stream, kernel_arg<P>(args)...);
    return hipGetLastError();
}
#endif

}  // namespace sc
