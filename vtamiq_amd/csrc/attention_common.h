// Device-side leaf helpers of the fused attention kernels (attention.hip, attention_varlen.hip).
// Only __forceinline__ leaves live here: the kernels' bodies stay in their own files (attention_varlen.hip's header records why), and a
// leaf lives here only if every kernel's instruction stream is what it was with the leaf written out in its file.  These four are
// (profiles/r18_launchers_isa.txt); the pieces attention_probs.hip and attention_rollout.hip have in common are not.
#pragma once
#include "dev_common.h"

namespace vtq {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
__device__ __forceinline__ s16x4 lds_tr16(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

// Split 8 probabilities into the hi / lo MFMA fragments (element j of the fragment = p[j]).
template <typename T>
__device__ __forceinline__ void split_p8(const float (&p)[8], typename Vec<T>::x8& hi, typename Vec<T>::x8& lo) {
    if constexpr (std::is_same<T, f16>::value) {
        typedef __attribute__((ext_vector_type(2))) _Float16 h2;
        uint32_t hw[4], lw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const auto hp = __builtin_amdgcn_cvt_pkrtz(p[2 * j], p[2 * j + 1]);      // truncation: hi <= p, p - hi exact in fp32
            const h2 hh = __builtin_bit_cast(h2, hp);
            hw[j] = __builtin_bit_cast(uint32_t, hp);
            // plain C++ (v_cvt_f32_f16 + v_sub): an inline-asm v_fma_mix here read v_exp results inside the hardware's
            // trans -> VALU forwarding window, which hipcc does not pad for asm operands: rare wrong lo halves (measured)
            lw[j] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(p[2 * j] - (float)hh[0], p[2 * j + 1] - (float)hh[1]));
        }
        typedef __attribute__((ext_vector_type(4))) uint32_t u4;
        hi = __builtin_bit_cast(f16x8, u4{hw[0], hw[1], hw[2], hw[3]});
        lo = __builtin_bit_cast(f16x8, u4{lw[0], lw[1], lw[2], lw[3]});
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t hb = __builtin_bit_cast(uint32_t, p[j]) & 0xFFFF0000u;     // bf16 by truncation
            const float hf = __builtin_bit_cast(float, hb);
            hi[j] = __builtin_bit_cast(bf16, (unsigned short)(hb >> 16));
            lo[j] = (bf16)(p[j] - hf);
        }
    }
}

// Two scores at a time: the exponent's argument and the row sum as packed fp32 operations (v_pk_add_f32 / v_pk_fma_f32: two lanes'
// worth of work per vector issue slot; the exponential itself has no packed form).  The row sum therefore runs as TWO partial sums
// (even / odd accumulator registers), added at the end of a tile -- every fused kernel uses this helper, so they stay bit-identical.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int NSPLIT>
__device__ __forceinline__ void exp_pair(f32x16& v, int r, float m_new, float sc, float nm, f32x2& rs2) {      // registers r, r + 1 of v
    f32x2 t = {v[r], v[r + 1]};
    if constexpr (NSPLIT == 3) t = t - f32x2{m_new, m_new};
    else t = t * f32x2{sc, sc} + f32x2{nm, nm};
    f32x2 pv = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
    v[r] = pv[0];
    v[r + 1] = pv[1];
    rs2 += pv;
}

// 3-term formats: the softmax scale (1/sqrt(64) * log2 e) is folded into Q once per query block -- q c = (hi + lo) c in fp32, split
// again -- so that scores arrive in log2 units and the exponent is exp2(s - m): one subtraction that is EXACT for the row maximum at
// any magnitude.  (The one-FMA form exp2(s c - m c) subtracts the rounded product m c: fine at ordinary logits, inf at the 1e13
// logits of a 1e7-gain model, where the fp32 reference is finite; the single-plane formats keep it behind a magnitude guard, since
// re-rounding q c to 11 bits would cost them accuracy.)
template <typename T>
__device__ __forceinline__ void prescale_q(typename Vec<T>::x8 (&qf)[2][4], float sc) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = ((float)qf[0][t][j] + (float)qf[1][t][j]) * sc;
            T a, b;
            split2<T>(v, a, b);
            qf[0][t][j] = a;
            qf[1][t][j] = b;
        }
}

}  // namespace vtq
