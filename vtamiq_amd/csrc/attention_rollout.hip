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
//
// Two decodes in front of ONE body (rollout_step_block): the uniform kernels, and rollout_step_varlen_kernel / rollout_combine_varlen_kernel
// for sequences of different lengths packed back to back (vtq_forward_varlen's layout), which look their work item up in the call's attention
// block table and address r, the result and the partials like the rows.  The body sees (first row, S, block, head) and two pointers either way,
// so a sequence's bits are those of the uniform kernel at S = S_pad = S_j, whatever else the launch holds.
//
// The Q-fragment load, the K tile staging, the QK^T block and the sweep-0 update / combine are COPIES of attention_probs.hip's, by decision:
// each was tried as a __forceinline__ function of a shared header, one at a time, and each changed the instruction stream of a kernel
// here or there (profiles/r18_launchers_isa.txt).
#include "dev_common.h"
#include "kernels.h"
#include "launch_common.h"

namespace vtq {
namespace {

constexpr int kRKT = 64;                   // keys per LDS tile (two 32-key MFMA blocks)
constexpr int kRTB = kRKT * 128;           // bytes of one tile plane: 64 keys x 64 dims x 2 B

// THE step of one workgroup: query block qb (128 rows) of head `head` of the sequence that is the S rows from row0.  r: the sequence's own
// S weights (NULL: e_token, the first step of a walk: the last layer); pout: the block's S partial column sums.  Both kernels below
// decode their work item and call this, so a sequence's arithmetic -- nt, nwv, every summation order -- is a function of S alone in both.
template <typename T, int NSPLIT>
__device__ __forceinline__ void rollout_step_block(const T* __restrict__ qkv, int64_t plane, int64_t row0, int S, int qb, int head,
                                                   const float* __restrict__ r, float* __restrict__ pout, int H, int q_log2, int token) {
    typedef typename Vec<T>::x8 tx8;
    constexpr int NPL = (NSPLIT == 1) ? 1 : 2;
    __shared__ __attribute__((aligned(16))) char sk[NPL * kRTB];
    __shared__ float cs[2][4][kRKT];                          // [tile parity][wave][key of the tile]: the waves' column sums
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    const int ld = 3 * H;
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
                if (q < S) rv = r ? r[q] : (q == token ? 1.0f : 0.0f);
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

// Uniform sequences: work item blockIdx.x = (sequence, head, query block) of nseq sequences of S rows at pitch S_pad; r: [nseq][S],
// part: [sequence][head][block][S]
template <typename T, int NSPLIT>
__global__ __launch_bounds__(256) void rollout_step_kernel(const T* __restrict__ qkv, int64_t plane, const float* __restrict__ r,
                                                           float* __restrict__ part, int S, int S_pad, int H, int q_log2, int token) {
    const int nqb = (S + 127) / 128, nh = H / 64;
    const int qb = blockIdx.x % nqb, head = (blockIdx.x / nqb) % nh, seq = blockIdx.x / (nqb * nh);
    rollout_step_block<T, NSPLIT>(qkv, plane, (int64_t)seq * S_pad, S, qb, head, r ? r + (int64_t)seq * S : nullptr,
                                  part + (((int64_t)seq * nh + head) * nqb + qb) * S, H, q_log2, token);
}

// Sequences of different lengths packed back to back (the layout vtq_forward_varlen leaves in the QKV planes): work item blockIdx.x is entry
// blocks[blockIdx.x] = {first row, S_j, query block, head} of attention_varlen_blocks().  r is packed like the rows (sequence j's S_j
// weights at its first row), part is [head][block < nqb_max][R] with R the total row count: a (head, block) plane is packed like the rows
// too, so a sequence's partials lie at its first row in every plane and need no per-sequence offset table.
template <typename T, int NSPLIT>
__global__ __launch_bounds__(256) void rollout_step_varlen_kernel(const T* __restrict__ qkv, int64_t plane, const float* __restrict__ r,
                                                                  float* __restrict__ part, const int4* __restrict__ blocks, int nqb_max,
                                                                  int64_t R, int H, int q_log2, int token) {
    const int4 blk = blocks[blockIdx.x];
    const int64_t row0 = blk.x;
    rollout_step_block<T, NSPLIT>(qkv, plane, row0, blk.y, blk.z, blk.w, r ? r + row0 : nullptr,
                                  part + ((int64_t)blk.w * nqb_max + blk.z) * R + row0, H, q_log2, token);
}

// Element j of one sequence: out = 1/2 r + 1/(2 nh) sum_head sum_block p[head * hstride + block * bstride], heads then blocks ascending;
// heads_out (may be NULL): [head * S] = sum_block (with r = e_token that is row `token` of the head's probabilities).  rv: r[j] or e_token[j]
__device__ __forceinline__ void rollout_combine_one(const float* __restrict__ p, int64_t hstride, int64_t bstride, int nh, int nqb, float rv,
                                                    float* __restrict__ out, float* __restrict__ heads_out, int S) {
    float tot = 0.f;
    for (int h = 0; h < nh; ++h) {
        float hs = 0.f;
#pragma unroll 4
        for (int b = 0; b < nqb; ++b) hs += p[h * hstride + b * bstride];
        if (heads_out) heads_out[(int64_t)h * S] = hs;
        tot += hs;
    }
    *out = 0.5f * rv + (0.5f / nh) * tot;
}

// out[seq][j] = 1/2 r[seq][j] + 1/(2 nh) sum_head sum_block part[seq][head][block][j]; heads_out (may be NULL): [seq][head][j].  r == NULL: e_token.
__global__ __launch_bounds__(256) void rollout_combine_kernel(const float* __restrict__ part, const float* __restrict__ r, int token,
                                                              float* __restrict__ out, float* __restrict__ heads_out, int S, int nh, int nqb) {
    const int j = blockIdx.x * 256 + threadIdx.x, seq = blockIdx.y;
    if (j >= S) return;
    const float rv = r ? r[(int64_t)seq * S + j] : (j == token ? 1.0f : 0.0f);
    rollout_combine_one(part + (int64_t)seq * nh * nqb * S + j, (int64_t)nqb * S, S, nh, nqb, rv, out + (int64_t)seq * S + j,
                        heads_out ? heads_out + (int64_t)seq * nh * S + j : nullptr, S);
}

// The same per (sequence, 256-key chunk) of packed sequences: row0 / len = the call's tables.  r and out packed like the rows; heads_out:
// sequence j's [nh][S_j] block at nh * row0[j]; blocks b < ceil(S_j / 128) of the nqb_max planes per head are the sequence's
__global__ __launch_bounds__(256) void rollout_combine_varlen_kernel(const float* __restrict__ part, const float* __restrict__ r, int token,
                                                                     float* __restrict__ out, float* __restrict__ heads_out,
                                                                     const int* __restrict__ row0, const int* __restrict__ len, int nh,
                                                                     int nqb_max, int64_t R) {
    const int j = blockIdx.x * 256 + threadIdx.x, seq = blockIdx.y;
    const int S = len[seq];
    if (j >= S) return;
    const int64_t r0 = row0[seq];
    const float rv = r ? r[r0 + j] : (j == token ? 1.0f : 0.0f);
    rollout_combine_one(part + r0 + j, (int64_t)nqb_max * R, R, nh, (S + 127) / 128, rv, out + r0 + j,
                        heads_out ? heads_out + nh * r0 + j : nullptr, S);
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
    const hipError_t e = with_format<BF16_1 | BF16_3 | F16_1 | F16_3>(num, [&](auto t, auto terms) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((rollout_step_kernel<T, terms.value>), g, b, 0, s, (const T*)qkv, plane, r, part, S, S_pad, H, ql, token);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rollout_combine_kernel, dim3((S + 255) / 256, nseq), dim3(256), 0, s, (const float*)part, r, token, out, heads_out, S, nh, nqb);
    return hipGetLastError();
}

hipError_t launch_rollout_step_varlen(const void* qkv, int64_t plane, const float* r, int token, float* part, float* out, float* heads_out,
                                      const int* blocks, int nblocks, const int* row0, const int* len, int nseq, int S_max, int64_t R, int H,
                                      Num num, hipStream_t s, bool q_log2) {
    if (nseq < 1 || nseq > 65535 || S_max < 1 || R < nseq || nblocks < 1 || !blocks || !row0 || !len || H % 64 || H < 64 ||
        (num.terms != 1 && num.terms != 3) || num.f16 > 1 || !part || !out || (!r && token < 0))
        return hipErrorInvalidValue;
    const int nh = H / 64, nqb_max = (S_max + 127) / 128;
    const dim3 g((unsigned)nblocks), b(256);
    const int ql = q_log2 ? 1 : 0;
    const int4* bl = (const int4*)blocks;
    const hipError_t e = with_format<BF16_1 | BF16_3 | F16_1 | F16_3>(num, [&](auto t, auto terms) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((rollout_step_varlen_kernel<T, terms.value>), g, b, 0, s, (const T*)qkv, plane, r, part, bl, nqb_max, R, H, ql, token);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rollout_combine_varlen_kernel, dim3((S_max + 255) / 256, nseq), dim3(256), 0, s, (const float*)part, r, token, out, heads_out,
                       row0, len, nh, nqb_max, R);
    return hipGetLastError();
}

}  // namespace vtq
