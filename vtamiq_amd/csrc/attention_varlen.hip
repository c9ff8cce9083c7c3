// Fused attention over sequences of DIFFERENT lengths packed back to back (vtq_forward_varlen, vtq_vl_attention).
//
// The 4-wave kernel of attention.hip (see its header for the structure: 128 query rows of one (sequence, head) per workgroup, 64-key K / V
// tiles through LDS by LDS-DMA, S^T = K Q^T and O^T += V^T P^T on the 32x32x16 MFMA, online softmax in the base-2 domain), with ONE change:
// a workgroup does not decode (sequence, head, query block) from a uniform sequence length, it looks them up in a block table the host built
// from the lengths:  entry w = {first row of the sequence, its length S_j, query block, head}.  Everything behind the lookup is that
// kernel's arithmetic per query row, statement for statement -- the tile count and the masked tail from S_j, masked scores replaced by a
// select, masked V rows zeroed in the last tile's LDS image -- so a sequence's output rows have the bits vtq_k_attention gives for that
// sequence alone (nseq = 1, S = S_pad = S_j; tests/test_gpu_varlen.py).  The body is a copy, not a shared header.  The header form was
// built both ways (the body as a device function taking the decoded block; the same with the decode passed in as a functor evaluated at its
// old place): each time hipcc gave attention.hip's own attention_kernel another register allocation and instruction schedule (~7000
// changed lines of ISA), i.e. a production kernel that would have to be measured and verified again for no gain of its own.  With the copy
// attention.hip and its objects stay exactly as they were.  What the two files do share is attention_common.h: the __forceinline__ leaf
// helpers (lds_tr16, split_p8, exp_pair, prescale_q), whose move left every kernel's instruction stream as it was.
// The e4m3 output form of the fp8 experiment is not offered here (vtq_forward_varlen refuses that engine).
#include <vector>

#include "attention_common.h"
#include "dev_common.h"
#include "kernels.h"
#include "launch_common.h"

namespace vtq {
namespace {

// blocks[w] = {first row of the sequence, S_j, query block (128 rows), head} for work id w; gridDim.x = number of entries
template <typename T, int NSPLIT>
__global__ __launch_bounds__(256) void attention_varlen_kernel(const T* __restrict__ qkv, int64_t plane, T* __restrict__ out,
                                                               int64_t o_plane, const int4* __restrict__ blocks, int H, int q_log2) {
    typedef typename Vec<T>::x8 tx8;
    typedef typename Vec<T>::x4 tx4;
    constexpr int NPL = (NSPLIT == 1) ? 1 : 2;
    constexpr int KT = 64, KB = KT / 32;     // 64-key K/V tiles = two 32-key blocks; two LDS buffers
    constexpr int TB = KT * 128;             // one KT-key x 64-dim 16-bit tile
    constexpr int STAGE = TB * NPL * 2;      // K planes then V planes
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    // 1-D grid, XCD-aware: the query blocks of one (sequence, head) re-read the same K/V and are consecutive work ids, so they must share
    // an L2.  Workgroups are dealt round-robin over the 8 XCDs; remap so each XCD owns a contiguous range of work ids (bijective).
    int wid = blockIdx.x;
    {
        const int nwg = gridDim.x, q8 = nwg >> 3, r8 = nwg & 7, xcd = wid & 7, idx = wid >> 3;
        wid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    }
    const int4 blk = blocks[wid];
    const int64_t row0 = blk.x;
    const int S = blk.y, qb = blk.z, head = blk.w;
    const int ld = 3 * H;
    const int q_row = qb * 128 + wave * 32 + c;
    // a wave whose 32 query rows all lie behind the sequence (ragged last block) stages and synchronises, nothing else
    const bool wave_active = (qb * 128 + wave * 32) < S;

    // ---- Q fragments: B operand of S^T = K Q^T, element j <-> d = 16t + 8hh + j ------------------------------
    // (whole 128-row blocks are loaded: rows >= S belong to the next sequence or the slack behind the last one; they reach no output)
    tx8 qf[2][4];
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
        for (int t = 0; t < 4; ++t)
            qf[pl][t] = *(const tx8*)(qkv + pl * plane + (row0 + q_row) * ld + head * 64 + 16 * t + 8 * hh);
    if constexpr (NSPLIT == 3) { if (!q_log2) prescale_q<T>(qf, 0.125f * 1.4426950408889634f); }

    // ---- DMA source offsets (elements) of this thread for the two rounds of a 64-row tile --------------------
    uint32_t k_off[KB], v_off[KB];
#pragma unroll
    for (int r = 0; r < KB; ++r) {
        const int slot = r * 256 + tid;
        const int row = slot >> 3, s = slot & 7;
        k_off[r] = (uint32_t)(row * ld + H + head * 64 + ((s ^ ((row >> 1) & 7)) << 3));
        v_off[r] = (uint32_t)(row * ld + 2 * H + head * 64 + ((s ^ (((row >> 1) & 1) << 2)) << 3));
    }
    auto stage = [&](int t, int buf) {
        char* sb = smem + buf * STAGE + wave * 1024;
        const T* base = qkv + (row0 + (int64_t)t * KT) * ld;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
            for (int r = 0; r < KB; ++r) {
                glds16(base + pl * plane + k_off[r], sb + pl * TB + r * 4096);
                glds16(base + pl * plane + v_off[r], sb + (NPL + pl) * TB + r * 4096);
            }
    };

    // K fragment read offset: row = kb*32 + c, chunk = 2t + hh, swizzle (row>>1)&7 == (c>>1)&7
    const int k_rd = c * 128;
    const int k_sw = (c >> 1) & 7;
    // V transposed-read offsets: 16-lane group g, lane i = 4*qq + pp supplies row qq, columns 4pp..4pp+3
    const int g = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    const int v_row = 4 * (g >> 1) + qq;                                        // + kb*32 + 16*s2 (+8)
    const int v_colb = ((16 * (g & 1) + 4 * pp) * 2) ^ (((qq >> 1) & 1) << 6);  // d-block toggles bit 6 too (XOR)

    f32x16 o_acc[2];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[d][r] = 0.f;
    float m_run = -1e30f, l_run = 0.f;
    const float sc = 0.125f * 1.4426950408889634f;   // 1/sqrt(64) * log2(e)

    // two K/V buffers: tile t+1 is in flight while tile t is consumed, one barrier per tile
    const int nt = (S + KT - 1) / KT;          // the last tile runs into the next sequence's rows: keys >= S are masked
    // The masked keys' probabilities are exactly 0, but their V rows belong to the NEXT sequence: a NaN / inf there would reach this
    // sequence through 0 x NaN.  Every thread zeroes, in the LDS image of the LAST key tile, the V pieces it staged itself whose row is a
    // masked key -- after its DMA has landed (the vmcnt wait), before the barrier that publishes the tile.
    const int tail_valid = S - (nt - 1) * KT;   // real keys in the last tile (1 .. 64)
    auto zero_masked_v = [&](int buf) {
#pragma unroll
        for (int r = 0; r < KB; ++r) {
            const int row = (r * 256 + tid) >> 3;
            if (row >= tail_valid) {
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) {
                    const u32x4 z = {0u, 0u, 0u, 0u};
                    asm volatile("ds_write_b128 %0, %1" ::"v"(lds_addr(smem + buf * STAGE + (NPL + pl) * TB + r * 4096 + tid * 16)), "v"(z) : "memory");
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (nt == 1) zero_masked_v(0);
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < nt; ++t) {
        const int nxt = cur ^ 1;
        if (t + 1 < nt) stage(t + 1, nxt);
        const char* sk = smem + cur * STAGE;
        const char* sv = sk + NPL * TB;

        if (wave_active) {
        // ---- S^T[key][q] for the 64 keys of this tile ---------------------------------------------------------
        f32x16 sacc[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int off = kb * 32 * 128 + k_rd + (((2 * tt + hh) ^ k_sw) << 4);
                const tx8 kf = *(const tx8*)(sk + off);
                sacc[kb] = mfma32<T>(kf, qf[0][tt], tt == 0 ? zero16 : sacc[kb]);
                if constexpr (NSPLIT == 3) {
                    const tx8 kl = *(const tx8*)(sk + TB + off);
                    sacc[kb] = mfma32<T>(kf, qf[1][tt], sacc[kb]);
                    sacc[kb] = mfma32<T>(kl, qf[0][tt], sacc[kb]);
                }
            }
        }

        // ---- online softmax (base-2 domain; scale folded into one FMA per score) -----------------------------------
        if ((t + 1) * KT > S) {                 // wave-uniform: only the last tile holds masked keys
            int hq = 4 * hh;
            asm volatile("" : "+v"(hq));         // keeps the 31 key offsets of this rare path out of loop-invariant registers
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * KT + kb * 32 + (r & 3) + 8 * (r >> 2) + hq;
                    if (key >= S) sacc[kb][r] = -INFINITY;
                }
        }
        float mx = sacc[0][0];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, sacc[kb][r]), sacc[kb][r + 1]);   // v_max3_f32
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                                              // running max (3-term: log2 units; else raw)
        float nm = -m_new * sc;
        f32x2 rs2 = {0.f, 0.f};
        if constexpr (NSPLIT == 3) {
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; r += 2) exp_pair<NSPLIT>(sacc[kb], r, m_new, sc, nm, rs2);
        } else {
            // single plane: exp2(s c - m c) as one FMA per score while |m c| <= 64; beyond (rare; the branch is wave-uniform, the decision per
            // query row): subtract the maximum first, then the same FMA with a zero addend (attention.hip has the reasoning)
            const bool big = fabsf(nm) > 64.f;
            if (__builtin_amdgcn_ballot_w64(big)) {
                const float sub = big ? m_new : 0.f;
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sacc[kb][r] -= sub;
                nm = big ? 0.f : nm;
            }
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; r += 2) exp_pair<NSPLIT>(sacc[kb], r, m_new, sc, nm, rs2);
        }
        const float rs = rs2[0] + rs2[1];
        if (__builtin_amdgcn_ballot_w64(m_new > m_run)) {        // some row's max moved: rescale (exact; usually skipped)
            const float alpha = __builtin_amdgcn_exp2f(NSPLIT == 3 ? m_run - m_new : (m_run - m_new) * sc);
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) o_acc[d][r] *= alpha;
        }
        m_run = m_new;
        l_run += rs;

        // ---- O^T[d][q] += V^T[d][key] P^T[key][q] -------------------------------------------------------------
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                tx8 ph, pl_;
                if constexpr (NSPLIT == 1) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) ph[j] = (T)sacc[kb][8 * s2 + j];
                } else {
                    float pj[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) pj[j] = sacc[kb][8 * s2 + j];
                    split_p8<T>(pj, ph, pl_);
                }
                const int vrow = kb * 32 + 16 * s2 + v_row;
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    // byte column of (d-block, 16-column half, 4-column piece); bit 6 carries the row swizzle
                    const char* a0 = sv + vrow * 128 + (v_colb ^ (d << 6));
                    const s16x4 v0 = lds_tr16(a0);
                    const s16x4 v1 = lds_tr16(a0 + 8 * 128);
                    const tx8 vf = __builtin_bit_cast(tx8, s16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
                    o_acc[d] = mfma32<T>(vf, ph, o_acc[d]);
                    if constexpr (NSPLIT == 3) {
                        const s16x4 w0 = lds_tr16(a0 + TB);
                        const s16x4 w1 = lds_tr16(a0 + TB + 8 * 128);
                        const tx8 vl = __builtin_bit_cast(tx8, s16x8{w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]});
                        o_acc[d] = mfma32<T>(vf, pl_, o_acc[d]);
                        o_acc[d] = mfma32<T>(vl, ph, o_acc[d]);
                    }
                }
            }

        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // tile t+1 has landed
        if (t + 2 == nt) zero_masked_v(nxt);                // ... and it is the last one: its masked keys' V rows become zeros
        __syncthreads();
        cur = nxt;
    }

    // ---- normalise and write merged heads: out[row][head*64 + d], rows < S only -------------------------------------
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if constexpr (NSPLIT == 1) {
        // Single plane: staged through LDS (the K / V buffers are free: the loop ended with a barrier) -- each wave transposes its 32 rows x 128
        // bytes through its own 4 KB image (chunk index XORed with row & 7), so that every store instruction writes eight whole 128-byte row
        // segments.  Same values as direct stores.
        if (wave_active) {
            char* const o_stage = smem + wave * 4096;
            const int r_row = lane >> 3, r_chunk = lane & 7;
#pragma unroll
            for (int k = 0; k < 8; ++k) {                         // chunk k = 4 d + g4 of row c, bytes 8 hh .. 8 hh + 7
                tx4 hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = o_acc[k >> 2][4 * (k & 3) + e] * inv;
                    asm volatile("" : "+v"(v));                   // rounded product, then converted (no fused form)
                    hv[e] = (T)v;
                }
                *(tx4*)(o_stage + c * 128 + ((k ^ (c & 7)) << 4) + 8 * hh) = hv;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = r_row + 8 * k;
                const uint4 w = *(const uint4*)(o_stage + row * 128 + ((r_chunk ^ (row & 7)) << 4));
                const int qr = qb * 128 + wave * 32 + row;
                if (qr < S) *(uint4*)(out + (row0 + qr) * H + head * 64 + 8 * r_chunk) = w;
            }
        }
    } else if (q_row < S) {
        T* o = out + (row0 + q_row) * H + head * 64;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int dcol = 32 * d + 8 * g4 + 4 * hh;
                tx4 hv, lv;
#pragma unroll
                for (int e = 0; e < 4; ++e) { T a, b; split2<T>(o_acc[d][4 * g4 + e] * inv, a, b); hv[e] = a; lv[e] = b; }
                *(tx4*)(o + dcol) = hv;
                *(tx4*)(o + o_plane + dcol) = lv;
            }
    }
}

template <typename T, int NSPLIT>
hipError_t launch_varlen_t(const void* qkv, int64_t plane, void* out, int64_t o_plane, const int* blocks, int nblocks, int H, hipStream_t s,
                           bool q_log2) {
    constexpr int LDS = 2 * 2 * 64 * 128 * (NSPLIT == 1 ? 1 : 2);
    const hipError_t e = ensure_dynamic_lds<attention_varlen_kernel<T, NSPLIT>>(LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((attention_varlen_kernel<T, NSPLIT>), dim3(nblocks), dim3(256), LDS, s, (const T*)qkv, plane, (T*)out, o_plane,
                       (const int4*)blocks, H, q_log2 ? 1 : 0);
    return hipGetLastError();
}

}  // namespace

// Work id w -> {first row, S_j, query block, head}: sequences in order, then heads, then the 128-row query blocks of that (sequence, head)
// side by side -- the order the kernel's XCD remap keeps on one L2.
std::vector<int> attention_varlen_blocks(const int* seq_len, int nseq, int H) {
    std::vector<int> t;
    const int nh = H / 64;
    int64_t row0 = 0;
    for (int j = 0; j < nseq; ++j) {
        const int S = seq_len[j], nqb = (S + 127) / 128;
        for (int h = 0; h < nh; ++h)
            for (int qb = 0; qb < nqb; ++qb) { t.push_back((int)row0); t.push_back(S); t.push_back(qb); t.push_back(h); }
        row0 += S;
    }
    return t;
}

hipError_t launch_attention_varlen(const void* qkv, int64_t plane, void* out, int64_t o_plane, const int* blocks, int nblocks, int H, Num num,
                                   hipStream_t s, bool q_log2) {
    if (H % 64 || H < 64 || nblocks < 1 || !blocks || (num.terms != 1 && num.terms != 3) || num.f16 > 1) return hipErrorInvalidValue;
    if (q_log2 && num.terms != 3) return hipErrorInvalidValue;
    return with_format<BF16_1 | BF16_3 | F16_1 | F16_3>(num, [&](auto t, auto terms) {
        return launch_varlen_t<typename decltype(t)::type, terms.value>(qkv, plane, out, o_plane, blocks, nblocks, H, s, q_log2);
    });
}

}  // namespace vtq
