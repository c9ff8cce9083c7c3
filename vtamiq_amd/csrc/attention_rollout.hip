// One step of attention rollout for a row vector: out = 1/2 r + 1/(2h) sum_heads r^T P_head, P = softmax(Q K^T / sqrt(64)) of one layer
// (Abnar & Zuidema, with the residual half; include/vtamiq_hip.h vtq_forward_rollout has the definition).  forward_rollout walks it from
// the last kept layer to the first; the S x S matrices are never stored: per (sequence, head, 128-row query block) the kernel forms
// the block's scores twice, as attention_probs.hip does, and keeps only the r-weighted COLUMN sums.
//
// rollout_step_kernel: the two sweeps of attention_probs.hip on the same operands (v_mfma_f32_32x32x16 in the Q K^T orientation, the
// same 1-term / 3-term score, the same q_log2 handling, the same per-lane running max / sum), so the probabilities are the ones
// forward_vit reports:
//   sweep 0: per query row i, row max m_i and row sum l_i;
//   sweep 1: w_i exp2(s_ij - m_i) with w_i = r_i / l_i, summed over the block's query rows.  The KEY index is on the lane in this
//            orientation, so the sum over a wave's 32 rows is 16 adds over the lane's own accumulator registers (ascending register
//            index) plus one add of the two lane halves; the four waves of a block meet in LDS and are added in wave order.
// Partial column sums go to part[sequence][head][block][S]; rollout_combine_kernel adds them over heads and blocks in ascending order
// and applies 1/2 r + 1/(2h) sum.  No floating-point atomics: every summation order is a function of S alone -- never of the number of
// sequences, the CU count or arrival order (the rule cls_tail.hip states for itself), so a pair's rollout does not depend on its batch.
// Query rows and keys >= S are masked (weight 0 / not stored); K and Q rows are clamped to row S - 1 of the sequence, so nothing
// outside the sequence's own rows [seq * S_pad, seq * S_pad + S) is read, and nothing outside [0, S) of a partial is written.
#include "dev_common.h"
#include "kernels.h"

namespace vtq {
namespace {

constexpr int kRKT = 64;                   // keys per LDS tile (two 32-key MFMA blocks)
constexpr int kRTB = kRKT * 128;           // bytes of one tile plane: 64 keys x 64 dims x 2 B

// r == NULL: r = e_token (the first step of a walk: the last layer)
template <typename T, int NSPLIT>
__global__ __launch_bounds__(256) void rollout_step_kernel(const T* __restrict__ qkv, int64_t plane, const float* __restrict__ r,
                                                           float* __restrict__ part, int S, int S_pad, int H, int q_log2, int token) {
    typedef typename Vec<T>::x8 tx8;
    constexpr int NPL = (NSPLIT == 1) ? 1 : 2;
    __shared__ __attribute__((aligned(16))) char sk[NPL * kRTB];
    __shared__ float cs[2][4][kRKT];                          // [tile parity][wave][key of the tile]: the waves' column sums
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    const int nqb = (S + 127) / 128, nh = H / 64;
    const int qb = blockIdx.x % nqb, head = (blockIdx.x / nqb) % nh, seq = blockIdx.x / (nqb * nh);
    const int ld = 3 * H;
    const int64_t row0 = (int64_t)seq * S_pad;
    const int qw = qb * 128 + wave * 32;                     // first query row of this wave
    const bool wave_active = qw < S;
    const int nwv = min(4, (S - qb * 128 + 31) / 32);        // waves of this block with a row < S

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

    // ---- K tile staging, as attention_probs.hip: 64 rows x 8 16-byte chunks per plane, chunk XOR-swizzled by (row >> 1) & 7
    const int nt = (S + kRKT - 1) / kRKT;
    uint4 k00, k01, k10, k11;                                 // [plane][round]
    auto load_tile = [&](int t) {
        const int r0 = tid >> 3, r1 = 32 + (tid >> 3), ch = tid & 7;
        const T* b0 = qkv + (row0 + min(t * kRKT + r0, S - 1)) * ld + H + head * 64 + ch * 8;
        const T* b1 = qkv + (row0 + min(t * kRKT + r1, S - 1)) * ld + H + head * 64 + ch * 8;
        k00 = *(const uint4*)b0;
        k01 = *(const uint4*)b1;
        if constexpr (NPL == 2) { k10 = *(const uint4*)(b0 + plane); k11 = *(const uint4*)(b1 + plane); }
    };
    auto store_tile = [&]() {
        const int r0 = tid >> 3, r1 = 32 + (tid >> 3), ch = tid & 7;
        const int o0 = r0 * 128 + ((ch ^ ((r0 >> 1) & 7)) << 4), o1 = r1 * 128 + ((ch ^ ((r1 >> 1) & 7)) << 4);
        *(uint4*)(sk + o0) = k00;
        *(uint4*)(sk + o1) = k01;
        if constexpr (NPL == 2) { *(uint4*)(sk + kRTB + o0) = k10; *(uint4*)(sk + kRTB + o1) = k11; }
    };
    const int k_rd = c * 128, k_sw = (c >> 1) & 7;

    // per lane and accumulator register j (query row (j & 3) + 8 (j >> 2) + 4 hh): running max / sum over this lane's key columns;
    // behind sweep 0, l holds the row's weight w = r / sum
    float m[16], l[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) { m[j] = -INFINITY; l[j] = 0.f; }
    float* pout = part + (((int64_t)seq * nh + head) * nqb + qb) * S;

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
                        const tx8 kl = *(const tx8*)(sk + kRTB + off);
                        acc = mfma32<T>(qf[1][tt], kf, acc);
                        acc = mfma32<T>(qf[0][tt], kl, acc);
                    }
                }
                if (!sweep) {
                    const bool kvalid = t * kRKT + kb * 32 + c < S;
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const float s = acc[j] * ssc;
                        const float d = s - m[j];
                        const float e = __builtin_amdgcn_exp2f(-fabsf(d));           // exp2(min - max) of (s, m)
                        const bool gt = d > 0.f;
                        const float ln = gt ? fmaf(l[j], e, 1.0f) : l[j] + e;
                        l[j] = kvalid ? ln : l[j];
                        m[j] = (kvalid && gt) ? s : m[j];
                    }
                } else {
                    // column sum over this wave's 32 query rows: the lane's 16 registers in ascending order, then the other lane half
                    float v = 0.f;
#pragma unroll
                    for (int j = 0; j < 16; ++j) v = fmaf(l[j], __builtin_amdgcn_exp2f(acc[j] * ssc - m[j]), v);
                    v += __shfl_xor(v, 32, 64);
                    if (hh == 0) cs[it & 1][wave][kb * 32 + c] = v;
                }
            }
        }
        if (it + 1 == nt && wave_active) {
            // end of sweep 0: combine the 32 key columns of every row (lanes of one half), then keep max and w = r / sum
#pragma unroll
            for (int j = 0; j < 16; ++j) {
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) {
                    const float m2 = __shfl_xor(m[j], o, 64), l2 = __shfl_xor(l[j], o, 64);
                    const float mn = fmaxf(m[j], m2);
                    const float a = l[j] == 0.f ? 0.f : l[j] * __builtin_amdgcn_exp2f(m[j] - mn);
                    const float b = l2 == 0.f ? 0.f : l2 * __builtin_amdgcn_exp2f(m2 - mn);
                    l[j] = a + b;
                    m[j] = mn;
                }
                const int q = qw + (j & 3) + 8 * (j >> 2) + 4 * hh;
                float rv = 0.f;                                  // rows >= S carry no weight
                if (q < S) rv = r ? r[(int64_t)seq * S + q] : (q == token ? 1.0f : 0.0f);
                l[j] = rv * (1.0f / l[j]);
            }
        }
        __syncthreads();                                       // the tile is consumed (and this tile's column sums are in LDS)
        if (sweep && tid < kRKT) {
            // the block's column sums of this tile: waves in ascending order.  cs[it & 1] is written again two barriers from here
            const int key = t * kRKT + tid;
            float v = cs[it & 1][0][tid];
            for (int w = 1; w < nwv; ++w) v += cs[it & 1][w][tid];
            if (key < S) pout[key] = v;
        }
    }
}

// out[seq][j] = 1/2 r[seq][j] + 1/(2 nh) sum_head sum_block part[seq][head][block][j], heads then blocks ascending; heads_out (may be NULL):
// [seq][head][j] = sum_block part[seq][head][block][j] (with r = e_token that is row `token` of the head's probabilities).  r == NULL: e_token.
__global__ __launch_bounds__(256) void rollout_combine_kernel(const float* __restrict__ part, const float* __restrict__ r, int token,
                                                              float* __restrict__ out, float* __restrict__ heads_out, int S, int nh, int nqb) {
    const int j = blockIdx.x * 256 + threadIdx.x, seq = blockIdx.y;
    if (j >= S) return;
    const float* p = part + (int64_t)seq * nh * nqb * S + j;
    float tot = 0.f;
    for (int h = 0; h < nh; ++h) {
        float hs = 0.f;
#pragma unroll 4
        for (int b = 0; b < nqb; ++b) hs += p[((int64_t)h * nqb + b) * S];
        if (heads_out) heads_out[((int64_t)seq * nh + h) * S + j] = hs;
        tot += hs;
    }
    const float rv = r ? r[(int64_t)seq * S + j] : (j == token ? 1.0f : 0.0f);
    out[(int64_t)seq * S + j] = 0.5f * rv + (0.5f / nh) * tot;
}

}  // namespace

hipError_t launch_rollout_step(const void* qkv, int64_t plane, const float* r, int token, float* part, float* out, float* heads_out, int nseq,
                               int S, int S_pad, int H, Num num, hipStream_t s, bool q_log2) {
    if (nseq < 1 || S < 1 || S_pad < S || H % 64 || H < 64 || (num.terms != 1 && num.terms != 3) || num.f16 > 1 || !part || !out ||
        (!r && (token < 0 || token >= S)))
        return hipErrorInvalidValue;
    const int nh = H / 64, nqb = (S + 127) / 128;
    const int64_t nwg = (int64_t)nseq * nh * nqb;
    if (nwg > 0x7fffffff || nseq > 65535) return hipErrorInvalidValue;
    const dim3 g((unsigned)nwg), b(256);
    const int ql = q_log2 ? 1 : 0;
    if (num.f16) {
        if (num.terms == 3) hipLaunchKernelGGL((rollout_step_kernel<f16, 3>), g, b, 0, s, (const f16*)qkv, plane, r, part, S, S_pad, H, ql, token);
        else hipLaunchKernelGGL((rollout_step_kernel<f16, 1>), g, b, 0, s, (const f16*)qkv, plane, r, part, S, S_pad, H, ql, token);
    } else {
        if (num.terms == 3) hipLaunchKernelGGL((rollout_step_kernel<bf16, 3>), g, b, 0, s, (const bf16*)qkv, plane, r, part, S, S_pad, H, ql, token);
        else hipLaunchKernelGGL((rollout_step_kernel<bf16, 1>), g, b, 0, s, (const bf16*)qkv, plane, r, part, S, S_pad, H, ql, token);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rollout_combine_kernel, dim3((S + 255) / 256, nseq), dim3(256), 0, s, (const float*)part, r, token, out, heads_out, S, nh, nqb);
    return hipGetLastError();
}

}  // namespace vtq
