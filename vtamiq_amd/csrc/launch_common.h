// Host-side helpers of the launch_* functions: the per-device dynamic-LDS opt-in and the operand-format dispatch, each stated once.
#pragma once
#include <mutex>
#include <type_traits>

#include "dev_common.h"
#include "kernels.h"

namespace vtq {

// A launch with more than 64 KiB of dynamic LDS needs the kernel's limit raised first, once per (kernel, device): hipFuncSetAttribute is
// per device.  One instance (mutex + flags) per kernel: ensure_dynamic_lds<my_kernel<T, N>>(LDS).  A failed attempt is tried again by
// the next call.
template <auto Kernel>
hipError_t ensure_dynamic_lds(int bytes) {
    static std::mutex mu;
    static bool granted[64] = {false};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (!granted[dev]) {
        e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
        granted[dev] = true;
    }
    return hipSuccess;
}

// (element type, count) -> f(Tag<bf16 | f16>{}, std::integral_constant<int, count>{}); count = the terms of a Num or the planes of a
// tensor.  ACCEPT: the formats the launcher has kernels for, as an OR of the bits below -- only those are instantiated, anything
// else is hipErrorInvalidValue.  The e4m3 format of the fp8 experiment is not dispatched here (gemm.hip, elementwise.hip).
template <typename T> struct Tag { typedef T type; };
enum : unsigned { BF16_1 = 1, BF16_2 = 2, BF16_3 = 4, F16_1 = 8, F16_2 = 16, F16_3 = 32 };
template <unsigned ACCEPT, int I = 0, typename F>
hipError_t with_format(int f16_, int count, F&& f) {
    if constexpr (I == 6) return hipErrorInvalidValue;
    else {
        if constexpr ((ACCEPT >> I) & 1)
            if (f16_ == I / 3 && count == I % 3 + 1) return f(Tag<std::conditional_t<I < 3, bf16, f16>>{}, std::integral_constant<int, I % 3 + 1>{});
        return with_format<ACCEPT, I + 1>(f16_, count, f);
    }
}
template <unsigned ACCEPT, typename F>
hipError_t with_format(Num num, F&& f) { return with_format<ACCEPT>(num.f16, num.terms, f); }

}  // namespace vtq
