// Attention probabilities softmax(Q K^T / sqrt(64)) as (nseq, h, S, S) fp32: the tensor MultiHeadSelfAttention returns as its
// weights (modules/VisionTransformer/transformer.py:158-162) and the fused kernels of attention.hip never form.  forward_vit
// launches it per layer when the caller asks for attention maps (vtq_forward_vit `probs`); the scoring path never does.
//
// Bound: the store stream.  B = 32, S = 501, h = 12 is 385 MB of fp32 per layer against ~1.5 GFLOP of QK^T (twice, see below),
// so the kernel is shaped around its stores:
//   * scores come out of v_mfma_f32_32x32x16 in the Q K^T orientation (A = Q fragment, B = K fragment): the KEY index lands on the
//     lane, so one accumulator register holds 32 consecutive keys of one query row in each lane half.  A store of one register is
//     two 128-byte row segments per wave instruction -- the full-rate store shape (MI355X_MICROARCH.md: 256 contiguous bytes or two
//     128-B segments per instruction), where the fused kernels' S^T = K Q^T layout (query on the lane) would write 64 rows per
//     instruction, ~17x slower;
//   * 3-term formats: each score is q_hi k_hi + q_lo k_hi + q_hi k_lo (fp32 accumulate), as in the fused kernel.
//
// Two sweeps over the keys (recompute form), one form for every S:
//   sweep 0: per query row, running max and sum of exp2, kept PER LANE (each lane sees one key column of every 32-key block:
//            an update is one exp2 and two selects, no cross-lane traffic), combined over the 32 lanes of a row once at the end;
//   sweep 1: the same scores again, p = exp2(s - max) / sum, stored as they come out of the MFMA.
// A whole 32-row score block fits in LDS at S ~ 500 but not at S = 5001 (640 KB), and a form that kept the block would need a
// second path for long sequences; recomputing QK^T costs MFMA time the store stream hides (24 MFMAs per 8 KB written per wave).
//
// Layout: QKV operand planes of the engine ([rows][3H], planes `plane` elements apart), sequences packed S_pad rows apart with no
// padding between them.  K rows of keys >= S are clamped to row S - 1 of the sequence (read, never used: their scores are masked),
// so nothing outside the sequence's own rows is read, and no row or column outside [0, S) is written.
// Scores are in log2 units: the 3-term formats of the engine carry 1/sqrt(64) * log2 e in Q already (q_log2, engine.hip
// kQLog2Scale); otherwise the kernel multiplies the fp32 score by it.  Row max and row sum are fp32.
#include "dev_common.h"
#include "kernels.h"
#include "launch_common.h"

namespace vtq {
namespace {

constexpr int kPKT = 64;                   // keys per LDS tile (two 32-key MFMA blocks)
constexpr int kPTB = kPKT * 128;           // bytes of one tile plane: 64 keys x 64 dims x 2 B

template <typename T, int NSPLIT>
__global__ __launch_bounds__(256) void attention_probs_kernel(const T* __restrict__ qkv, int64_t plane, float* __restrict__ probs,
                                                              int S, int S_pad, int H, int q_log2) {
    typedef typename Vec<T>::x8 tx8;
    constexpr int NPL = (NSPLIT == 1) ? 1 : 2;
    __shared__ __attribute__((aligned(16))) char sk[NPL * kPTB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    const int nqb = (S + 127) / 128, nh = H / 64;
    const int qb = blockIdx.x % nqb, head = (blockIdx.x / nqb) % nh, seq = blockIdx.x / (nqb * nh);
    const int ld = 3 * H;
    const int64_t row0 = (int64_t)seq * S_pad;
    const int qw = qb * 128 + wave * 32;                     // first query row of this wave
    const bool wave_active = qw < S;

    // ---- Q fragments: A operand, lane (c, hh) holds Q[qw + c][16 t + 8 hh + j] ----------------------------------------
    tx8 qf[NPL][4];
    {
        const int qr = min(qw + c, S - 1);
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
            for (int t = 0; t < 4; ++t) qf[pl][t] = *(const tx8*)(qkv + pl * plane + (row0 + qr) * ld + head * 64 + 16 * t + 8 * hh);
    }
    const float ssc = (NSPLIT == 3 && q_log2) ? 1.0f : 0.125f * 1.4426950408889634f;

    // ---- K tile staging: 64 rows x 8 16-byte chunks per plane, rows tid / 8 and 32 + tid / 8 per thread; chunk XOR-swizzled by (row >> 1) & 7
    const int nt = (S + kPKT - 1) / kPKT;
    // (named registers, not an array: hipcc kept a [2][2] array of them in scratch)
    uint4 k00, k01, k10, k11;                                 // [plane][round]
    auto load_tile = [&](int t) {
        const int r0 = tid >> 3, r1 = 32 + (tid >> 3), ch = tid & 7;
        const T* b0 = qkv + (row0 + min(t * kPKT + r0, S - 1)) * ld + H + head * 64 + ch * 8;
        const T* b1 = qkv + (row0 + min(t * kPKT + r1, S - 1)) * ld + H + head * 64 + ch * 8;
        k00 = *(const uint4*)b0;
        k01 = *(const uint4*)b1;
        if constexpr (NPL == 2) { k10 = *(const uint4*)(b0 + plane); k11 = *(const uint4*)(b1 + plane); }
    };
    auto store_tile = [&]() {
        const int r0 = tid >> 3, r1 = 32 + (tid >> 3), ch = tid & 7;
        const int o0 = r0 * 128 + ((ch ^ ((r0 >> 1) & 7)) << 4), o1 = r1 * 128 + ((ch ^ ((r1 >> 1) & 7)) << 4);
        *(uint4*)(sk + o0) = k00;
        *(uint4*)(sk + o1) = k01;
        if constexpr (NPL == 2) { *(uint4*)(sk + kPTB + o0) = k10; *(uint4*)(sk + kPTB + o1) = k11; }
    };
    const int k_rd = c * 128, k_sw = (c >> 1) & 7;

    // per lane and accumulator register r (query row (r & 3) + 8 (r >> 2) + 4 hh): running max / sum over this lane's key columns
    float m[16], l[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { m[r] = -INFINITY; l[r] = 0.f; }

    load_tile(0);
    for (int it = 0; it < 2 * nt; ++it) {
        const int sweep = it >= nt, t = sweep ? it - nt : it;
        store_tile();
        __syncthreads();
        if (it + 1 < 2 * nt) load_tile(it + 1 < nt ? it + 1 : it + 1 - nt);      // next tile in flight during this one's MFMAs

        if (wave_active) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                f32x16 acc = zero16;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int off = kb * 32 * 128 + k_rd + (((2 * tt + hh) ^ k_sw) << 4);
                    const tx8 kf = *(const tx8*)(sk + off);
                    acc = mfma32<T>(qf[0][tt], kf, acc);
                    if constexpr (NSPLIT == 3) {
                        const tx8 kl = *(const tx8*)(sk + kPTB + off);
                        acc = mfma32<T>(qf[1][tt], kf, acc);
                        acc = mfma32<T>(qf[0][tt], kl, acc);
                    }
                }
                const int key = t * kPKT + kb * 32 + c;
                const bool kvalid = key < S;
                if (!sweep) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float s = acc[r] * ssc;
                        const float d = s - m[r];
                        const float e = __builtin_amdgcn_exp2f(-fabsf(d));           // exp2(min - max) of (s, m)
                        const bool gt = d > 0.f;
                        const float ln = gt ? fmaf(l[r], e, 1.0f) : l[r] + e;
                        l[r] = kvalid ? ln : l[r];
                        m[r] = (kvalid && gt) ? s : m[r];
                    }
                } else if (kvalid) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int q = qw + (r & 3) + 8 * (r >> 2) + 4 * hh;
                        const float p = __builtin_amdgcn_exp2f(acc[r] * ssc - m[r]) * l[r];
                        if (q < S) probs[(((int64_t)seq * nh + head) * S + q) * S + key] = p;
                    }
                }
            }
        }
        if (it + 1 == nt && wave_active) {
            // end of sweep 0: combine the 32 key columns of every row (lanes of one half), then keep max and 1 / sum
#pragma unroll
            for (int r = 0; r < 16; ++r) {
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) {
                    const float m2 = __shfl_xor(m[r], o, 64), l2 = __shfl_xor(l[r], o, 64);
                    const float mn = fmaxf(m[r], m2);
                    const float a = l[r] == 0.f ? 0.f : l[r] * __builtin_amdgcn_exp2f(m[r] - mn);
                    const float b = l2 == 0.f ? 0.f : l2 * __builtin_amdgcn_exp2f(m2 - mn);
                    l[r] = a + b;
                    m[r] = mn;
                }
                l[r] = 1.0f / l[r];
            }
        }
        __syncthreads();                                       // the tile is consumed before the next one overwrites it
    }
}

}  // namespace

hipError_t launch_attention_probs(const void* qkv, int64_t plane, float* probs, int nseq, int S, int S_pad, int H, Num num, hipStream_t s,
                                  bool q_log2) {
    if (nseq < 1 || S < 1 || S_pad < S || H % 64 || H < 64 || (num.terms != 1 && num.terms != 3) || num.f16 > 1)
        return hipErrorInvalidValue;
    const int64_t nwg = (int64_t)nseq * (H / 64) * ((S + 127) / 128);
    if (nwg > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 g((unsigned)nwg), b(256);
    const int ql = q_log2 ? 1 : 0;
    return with_format<BF16_1 | BF16_3 | F16_1 | F16_3>(num, [&](auto t, auto terms) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((attention_probs_kernel<T, terms.value>), g, b, 0, s, (const T*)qkv, plane, probs, S, S_pad, H, ql);
        return hipGetLastError();
    });
}

}  // namespace vtq
