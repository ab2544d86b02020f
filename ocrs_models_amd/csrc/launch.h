// Host-side launch helpers (included from common.h): the dynamic-LDS opt-in, run-time flags -> template arguments, per-launch timestamps.
// A dispatch that matches no instantiation is an error (OCRS_ERR_ARG): no launcher reaches its second stage without having launched its kernel.
#pragma once
#include <stdlib.h>
#include <atomic>
#include <type_traits>
#include <utility>

// "done once per device" flag: launchers run on the forward and on the autograd thread (doing it twice is harmless, skipping it on a second
// device is not)
struct DevOnce {
    std::atomic<unsigned long long> mask{0};
    static unsigned long long bit() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        return 1ull << (dev & 63);
    }
    bool need() const { return !(mask.load(std::memory_order_relaxed) & bit()); }
    void done() { mask.fetch_or(bit(), std::memory_order_relaxed); }
};
// Opt kernel K in to `bytes` of dynamic LDS (above the 64 KB default), once per device and instantiation -- every launch of one instantiation
// asks for the same size:   if (int rc = dyn_lds<&k<A, B>>(CC::SMEM)) return rc;
template <auto K>
static inline int dyn_lds(int bytes) {
    static DevOnce once;
    if (once.need()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return OCRS_ERR_HIP;
        once.done();
    }
    return OCRS_OK;
}

// Run-time flags as template arguments: with_bools(f, b0, b1, ...) = f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...)
//   return with_bools([&](auto g2, auto stats) { OCRS_LAUNCH_T((k<g2(), stats()>), ...); return OCRS_OK; }, g2 != nullptr, stats);
// An instantiation that does not exist is excluded inside f with `if constexpr (...) return OCRS_ERR_ARG;`.
template <class F>
static inline auto with_bools(F&& f) {
    return f();
}
template <class F, class... Bs>
static inline auto with_bools(F&& f, bool b, Bs... bs) {
    return with_bools([&](auto... cs) { return b ? f(std::true_type{}, cs...) : f(std::false_type{}, cs...); }, bs...);
}
// The ABI's dtype (0 = fp32, 1 = bf16) as a type: f(T{}) with T = float or bf16, for launchers whose two branches differ in nothing else
//   with_dtype(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(k<T>, ..., (const T*)x, ...); });
template <class F>
static inline auto with_dtype(int dtype, F&& f) {
    return dtype == 1 ? f(bf16{}) : f(float{});
}
// with_int<V0, V1, ...>(v, f): f(std::integral_constant<int, V>{}) for the V equal to v; false if there is none (f did not run)
//   int rc = OCRS_ERR_ARG;
//   with_int<8, 16>(Cout, [&](auto co) { rc = launch<co()>(...); });
template <int... Vs, class F>
static inline bool with_int(int v, F&& f) {
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// Per-launch timestamps from the dispatch packet (csrc/prof.hip): OCRS_LAUNCH_T == hipLaunchKernelGGL unless ocrs_prof_enable(1)
struct OcrsProf {
    int on, used, cap;
    hipEvent_t* ev;  // [2 * cap]: start / stop pairs
};
OcrsProf& ocrs_prof();
#define OCRS_LAUNCH_T(kernel, grid, block, smem, st, ...)                                                   \
    do {                                                                                                    \
        OcrsProf& pf_ = ocrs_prof();                                                                        \
        if (pf_.on && pf_.used < pf_.cap) {                                                                 \
            hipEvent_t e0_ = pf_.ev[2 * pf_.used], e1_ = pf_.ev[2 * pf_.used + 1];                          \
            ++pf_.used;                                                                                     \
            hipExtLaunchKernelGGL(kernel, grid, block, smem, st, e0_, e1_, 0, __VA_ARGS__);                 \
        } else {                                                                                            \
            hipLaunchKernelGGL(kernel, grid, block, smem, st, __VA_ARGS__);                                 \
        }                                                                                                   \
    } while (0)
