// Last encoder layer, CLS row only.
//
// VTAMIQ consumes token 0 of the encoder output and nothing else (modules/vtamiq/vtamiq.py:104-108), so in the LAST
// EncoderLayer (modules/VisionTransformer/transformer.py:275-285) the query, the attention output, out-proj, LayerNorm_2 and the
// MLP are needed for the 2B CLS rows alone -- and with ONE query per (sequence, head) the key and value projections of the other rows
// fold into that query ("the folded single-query attention" below), so no other row is normalised into planes or projected: the layer
// reads the fp32 residual rows once.  This file holds the row LayerNorm and that attention; the tail's five linear stages run on the
// MFMA pipe (skinny.hip).  Results are identical in exact arithmetic to running the full layer and reading row 0 (SURVEY.md 8d allows
// the pruning; bench reports executed flops).
#include "dev_common.h"
#include "kernels.h"
#include "launch_common.h"

namespace vtq {
namespace {

// LayerNorm(eps 1e-6) of gathered fp32 rows: src row r at src + r*stride; writes ln[r][H] and optionally a copy of the row.
template <int V4>
__global__ __launch_bounds__(256) void rows_ln_kernel(const float* __restrict__ src, int64_t stride, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ ln, float* __restrict__ copy,
                                                      int rows, PlaneOut po, const int* __restrict__ vl_row0) {
    constexpr int H = 256 * V4;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float4* xr = (const float4*)(src + (vl_row0 ? (int64_t)vl_row0[r] * H : r * stride));     // variable length: rows by table
    float4 v[V4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        v[i] = xr[i * 64 + lane];
        if (copy) ((float4*)(copy + (int64_t)r * H))[i * 64 + lane] = v[i];
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(s) * (1.0f / H);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
        q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / H) + 1e-6f);
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        const float4 w4 = ((const float4*)w)[i * 64 + lane], b4 = ((const float4*)b)[i * 64 + lane];
        float4 y = {v[i].x * rstd * w4.x + b4.x, v[i].y * rstd * w4.y + b4.y, v[i].z * rstd * w4.z + b4.z, v[i].w * rstd * w4.w + b4.w};
        ((float4*)(ln + (int64_t)r * H))[i * 64 + lane] = y;
        plane_store4(po, r, (i * 64 + lane) * 4, y.x, y.y, y.z, y.w);
    }
}

// ---- the folded single-query attention of the tail ------------------------------------------------------------------
// With one query per (sequence, head) the key and value projections re-associate exactly (ln_s = LayerNorm_1(x_s)):
//   score[s,h] = q_h . (W_k,h ln_s + b_k,h) = (W_k,h^T q_h) . ln_s + const(h)          const(h) drops out of the softmax
//   ctx_h      = sum_s p[s,h] (W_v,h ln_s + b_v,h) = W_v,h (sum_s p[s,h] ln_s) + b_v,h  (sum_s p = 1)
// so the tail needs neither K nor V of any row: u = W_k^T q per (sequence, head) (cls_key_fold_kernel), one streaming pass over the
// sequence's fp32 residual rows that normalises them and forms z_h = sum_s p[s,h] ln_s (cls_fold_attention_kernel, partials per
// row chunk; cls_fold_combine_kernel), and the value projection of z on the skinny MFMA path (skinny.hip, xcol64).
// Everything a result depends on -- chunk bounds, the order of every sum -- is a function of S alone: never of the number of
// sequences, the CU count or arrival order (the scores of a pair do not depend on the batch it is in).
constexpr int kFoldChunk = 64;     // rows of a sequence per partial (m, l, z)
constexpr int kFoldSub = 32;       // rows normalised into LDS at a time (two per chunk, running maximum between them)
constexpr int kFoldPad = 16;       // floats between LDS rows: the z product's B reads (4 rows x 16 columns per instruction) hit 64 different banks

// u[r][h][:] = sum_d q[r][64 h + d] * W_k[64 h + d][:]: a combination of 64 weight rows (hi [+ lo] planes as float).
// One workgroup of H threads per (head, 4 rows): the weight rows are read once for its 4 queries.  Thread (g, t) owns columns 4t .. 4t + 3
// of the 16 weight rows d = 16 g .. 16 g + 15, all requested before the first is used (one exposed latency; walking the 64 rows in one
// thread cost 45 us); the four row groups meet in LDS and are added in the order g = 0, 1, 2, 3.
template <typename T, int WPL>
__global__ __launch_bounds__(1024) void cls_key_fold_kernel(const float* __restrict__ q, const T* __restrict__ wk, int64_t w_plane, int ldw,
                                                            float* __restrict__ u, int R, int H) {
    typedef typename Vec<T>::x4 tx4;
    __shared__ float qs[4][64];
    __shared__ __attribute__((aligned(16))) float red[3][4][1024];
    const int head = blockIdx.x, nh = gridDim.x, r0 = blockIdx.y * 4;
    const int ct = H >> 2, g = threadIdx.x / ct, c = 4 * (threadIdx.x - g * ct);
    const T* wr = wk + ((int64_t)head * 64 + g * 16) * ldw + c;
    tx4 wh[16], wl[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        wh[i] = *(const tx4*)(wr + (int64_t)i * ldw);
        if constexpr (WPL == 2) wl[i] = *(const tx4*)(wr + (int64_t)i * ldw + w_plane);
    }
    if (threadIdx.x < 256) {
        const int rr = threadIdx.x >> 6, d = threadIdx.x & 63;
        qs[rr][d] = (r0 + rr < R) ? q[(int64_t)(r0 + rr) * H + head * 64 + d] : 0.f;
    }
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[rr][e] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[e] = (float)wh[i][e];
            if constexpr (WPL == 2) w[e] += (float)wl[i][e];
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float qd = qs[rr][g * 16 + i];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[rr][e] = fmaf(qd, w[e], acc[rr][e]);
        }
    }
    if (g > 0) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) *(float4*)&red[g - 1][rr][c] = float4{acc[rr][0], acc[rr][1], acc[rr][2], acc[rr][3]};
    }
    __syncthreads();
    if (g > 0) return;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 o = *(const float4*)&red[k][rr][c];
            acc[rr][0] += o.x; acc[rr][1] += o.y; acc[rr][2] += o.z; acc[rr][3] += o.w;
        }
        if (r0 + rr < R) *(float4*)(u + ((int64_t)(r0 + rr) * nh + head) * H + c) = float4{acc[rr][0], acc[rr][1], acc[rr][2], acc[rr][3]};
    }
}

// One workgroup (8 waves) per (sequence, chunk of kFoldChunk rows): partial[seq][chunk] = z[nh][H] | (m, l)[nh] with
//   m_h = max_s score[s,h],  l_h = sum_s e(score[s,h] - m_h),  z_h = sum_s e(score[s,h] - m_h) ln_s      (s over the chunk's rows < S)
// and e = exp2 (q_log2: q arrived in log2 units) or exp of 0.125 * the dot product, as the attention kernels have it.  Per kFoldSub rows:
//   1. wave w normalises rows 4w .. 4w+3 (the two-pass statistics of rows_ln_kernel) from registers into LDS; the next rows' global
//      loads are issued behind the barrier and land under the products;
//   2. scores [32 x 16 heads] = ln [32 x H] . u^T on the fp32-input MFMA (16x16x4): wave -> row block w & 1, quarter w >> 1 of H; the
//      four quarters meet in LDS in a fixed order;
//   3. running maximum per head, p = e(score - m), previous sums rescaled by e(m_old - m);
//   4. z [16 heads x H] += p^T [16 x 32] . ln [32 x H] on the same MFMA: wave w owns the 16-column blocks w, w + 8, ...; l is the
//      same product against a column of ones (wave 0), so it is summed in the same row order as z
// Rows >= S are never read (p = 0 against zero rows); no other sequence's row is touched.
template <int V4>
__global__ __launch_bounds__(512) void cls_fold_attention_kernel(const float* __restrict__ x, int64_t seq_stride, const float* __restrict__ lw,
                                                                 const float* __restrict__ lb, const float* __restrict__ u,
                                                                 float* __restrict__ part, int S, int nh, int q_log2, VarSeq vl) {
    constexpr int H = 256 * V4, LD = H + kFoldPad, NG = 4 * V4, NB = 2 * V4;
    extern __shared__ __attribute__((aligned(16))) float fold_smem[];
    float* rows = fold_smem;                                                         // [32][LD] normalised rows
    float (*scp)[kFoldSub][16] = (float (*)[kFoldSub][16])(rows + kFoldSub * LD);    // [4][32][16] score parts of the quarters of H
    float (*pr)[16] = (float (*)[16])(rows + kFoldSub * LD + 4 * kFoldSub * 16);     // [32][16] scores
    float (*pp)[16] = (float (*)[16])(rows + kFoldSub * LD + 5 * kFoldSub * 16);     // [32][16] p
    float* run = rows + kFoldSub * LD + 6 * kFoldSub * 16;                           // [2][16] running maximum (even / odd pass) | [16] rescale
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = blockIdx.x, seq = blockIdx.y, c0 = chunk * kFoldChunk;
    // variable length: this sequence's own length and first row; the grid spans the chunks of the longest sequence, and a workgroup
    // behind its sequence's last chunk has nothing to do (uniform over the workgroup, ahead of the first barrier)
    if (vl.len) {
        S = vl.len[seq];
        if (c0 >= S) return;
    }
    const float* xs = x + (vl.row0 ? (int64_t)vl.row0[seq] * H : (int64_t)seq * seq_stride);
    const int rb = wave & 1, kbase = (wave >> 1) * (H / 4);
    // step 2's B operand: lane (head fr, k slot fq) holds u[head][kbase + 16 j + 4 fq + e] as element e of fragment j (heads >= nh: a copy
    // of the last head, whose scores are dropped)
    float4 uf[NG];
    {
        const float* ur = u + ((int64_t)seq * nh + (fr < nh ? fr : nh - 1)) * H + kbase + 4 * fq;
#pragma unroll
        for (int j = 0; j < NG; ++j) uf[j] = *(const float4*)(ur + 16 * j);
    }
    float4 v[4][V4];
    auto load_rows = [&](int sub) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int srow = c0 + sub * kFoldSub + wave * 4 + i;
            if (srow < S) {                                       // wave-uniform
                const float4* xr = (const float4*)(xs + (int64_t)srow * H);
#pragma unroll
                for (int k = 0; k < V4; ++k) v[i][k] = xr[k * 64 + lane];
            } else {
#pragma unroll
                for (int k = 0; k < V4; ++k) v[i][k] = float4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    f32x4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 accl = {0.f, 0.f, 0.f, 0.f};                            // wave 0: l, as the product of p^T with a column of ones
    if (tid < 16) run[tid] = -INFINITY;
    const int left = S - c0;
    const int nsub = left >= kFoldChunk ? kFoldChunk / kFoldSub : (left + kFoldSub - 1) / kFoldSub;
    load_rows(0);
    for (int sub = 0; sub < nsub; ++sub) {
        const int s0 = c0 + sub * kFoldSub;
        // 1. LayerNorm of this wave's four rows into LDS (weight and bias re-read per pass: L1 hits, and 8 V4 registers less across the products)
        float4 w4[V4], b4[V4];
#pragma unroll
        for (int k = 0; k < V4; ++k) { w4[k] = ((const float4*)lw)[k * 64 + lane]; b4[k] = ((const float4*)lb)[k * 64 + lane]; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wave * 4 + i;
            const bool live = s0 + row < S;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < V4; ++k) s += (v[i][k].x + v[i][k].y) + (v[i][k].z + v[i][k].w);
            const float mean = wave_sum(s) * (1.0f / H);
            float qq = 0.f;
#pragma unroll
            for (int k = 0; k < V4; ++k) {
                v[i][k].x -= mean; v[i][k].y -= mean; v[i][k].z -= mean; v[i][k].w -= mean;
                qq += (v[i][k].x * v[i][k].x + v[i][k].y * v[i][k].y) + (v[i][k].z * v[i][k].z + v[i][k].w * v[i][k].w);
            }
            const float rstd = 1.0f / sqrtf(wave_sum(qq) * (1.0f / H) + 1e-6f);
#pragma unroll
            for (int k = 0; k < V4; ++k) {
                float4 y = {v[i][k].x * rstd * w4[k].x + b4[k].x, v[i][k].y * rstd * w4[k].y + b4[k].y, v[i][k].z * rstd * w4[k].z + b4[k].z,
                            v[i][k].w * rstd * w4[k].w + b4[k].w};
                if (!live) y = float4{0.f, 0.f, 0.f, 0.f};
                *(float4*)(rows + row * LD + (k * 64 + lane) * 4) = y;
            }
        }
        __syncthreads();
        if (sub + 1 < nsub) load_rows(sub + 1);
        // 2. score parts of this wave's row block and quarter of H
        {
            f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
            const float* ar = rows + (rb * 16 + fr) * LD + kbase + 4 * fq;
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                const float4 a = *(const float4*)(ar + 16 * j);
                sa = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, uf[j].x, sa, 0, 0, 0);
                sb = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, uf[j].y, sb, 0, 0, 0);
                sa = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, uf[j].z, sa, 0, 0, 0);
                sb = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, uf[j].w, sb, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) scp[wave >> 1][rb * 16 + 4 * fq + e][fr] = sa[e] + sb[e];      // D: row 4 fq + e, column (head) fr
        }
        __syncthreads();
        // 3. thread (row, head): the score; the head's new maximum; p
        const int row = tid >> 4, h = tid & 15;
        {
            float sc = (scp[0][row][h] + scp[1][row][h]) + (scp[2][row][h] + scp[3][row][h]);
            if (!q_log2) sc *= 0.125f;
            if (s0 + row >= S || h >= nh) sc = -INFINITY;
            pr[row][h] = sc;
        }
        __syncthreads();
        const float m_old = run[(sub & 1) * 16 + h];
        float mx = m_old;
#pragma unroll 8
        for (int r = 0; r < kFoldSub; ++r) mx = fmaxf(mx, pr[r][h]);
        {
            const float d = pr[row][h] - mx;
            pp[row][h] = h < nh ? (q_log2 ? exp2f(d) : expf(d)) : 0.f;
            if (tid < 16) {
                const float dm = m_old - mx;
                run[((sub + 1) & 1) * 16 + h] = mx;
                run[32 + h] = h < nh ? (q_log2 ? exp2f(dm) : expf(dm)) : 1.f;
            }
        }
        __syncthreads();
        // 4. z += p^T ln: A = p^T (lane: head fr, row 4 s + fq), B = ln (lane: row 4 s + fq, column n0 + fr)
        {
            if (sub > 0) {
                const float4 al = *(const float4*)(run + 32 + 4 * fq);
#pragma unroll
                for (int b = 0; b < NB; ++b) { acc[b][0] *= al.x; acc[b][1] *= al.y; acc[b][2] *= al.z; acc[b][3] *= al.w; }
                accl[0] *= al.x; accl[1] *= al.y; accl[2] *= al.z; accl[3] *= al.w;
            }
            float pa[kFoldSub / 4];
#pragma unroll
            for (int s = 0; s < kFoldSub / 4; ++s) pa[s] = pp[4 * s + fq][fr];
#pragma unroll
            for (int s = 0; s < kFoldSub / 4; ++s) {
                const float* br = rows + (4 * s + fq) * LD + 16 * wave + fr;
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s], br[128 * b], acc[b], 0, 0, 0);
                if (wave == 0) accl = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s], 1.0f, accl, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    float* pz = part + ((int64_t)seq * gridDim.x + chunk) * nh * (H + 2);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * fq + e < nh) pz[(4 * fq + e) * H + 16 * wave + 128 * b + fr] = acc[b][e];       // D: row (head) 4 fq + e, column fr
    if (tid < nh) pz[nh * H + 2 * tid] = run[(nsub & 1) * 16 + tid];
    if (wave == 0 && fr == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * fq + e < nh) pz[nh * H + 2 * (4 * fq + e) + 1] = accl[e];
    }
}

// zbar[seq][h][:] = sum_c e(m_c - m) z_c / sum_c e(m_c - m) l_c over the sequence's chunks in ascending order, written as the operand
// planes of the value projection (row seq, columns h H ..).  One workgroup per (head, sequence), thread t owns columns 4t .. 4t + 3.
__global__ __launch_bounds__(256) void cls_fold_combine_kernel(const float* __restrict__ part, int nchunks, int H, PlaneOut po, int q_log2,
                                                               const int* __restrict__ vl_len) {
    const int head = blockIdx.x, nh = gridDim.x, seq = blockIdx.y, c4 = 4 * threadIdx.x;
    if (c4 >= H) return;
    const int64_t ps = (int64_t)nh * (H + 2);
    const float* pb = part + (int64_t)seq * nchunks * ps;           // nchunks: the chunk pitch of `part` ...
    if (vl_len) nchunks = (vl_len[seq] + kFoldChunk - 1) / kFoldChunk;   // ... and, variable length, this sequence's own chunk count
    const float* ml = pb + (int64_t)nh * H + 2 * head;
    // loads in batches (a chunk index past the end re-reads the last chunk and is not used): a loop of single dependent loads cost one
    // memory latency per chunk
    float mx = -INFINITY;
    for (int c0 = 0; c0 < nchunks; c0 += 8) {
        float mv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) mv[i] = ml[(c0 + i < nchunks ? c0 + i : nchunks - 1) * ps];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (c0 + i < nchunks) mx = fmaxf(mx, mv[i]);
    }
    float l = 0.f, z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < nchunks; c0 += 4) {
        float mv[4], lv[4];
        float4 zc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t o = (c0 + i < nchunks ? c0 + i : nchunks - 1) * ps;
            mv[i] = ml[o]; lv[i] = ml[o + 1];
            zc[i] = *(const float4*)(pb + o + (int64_t)head * H + c4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (c0 + i >= nchunks) break;
            const float d = mv[i] - mx;
            const float w = q_log2 ? exp2f(d) : expf(d);
            l = fmaf(w, lv[i], l);
            z[0] = fmaf(w, zc[i].x, z[0]); z[1] = fmaf(w, zc[i].y, z[1]); z[2] = fmaf(w, zc[i].z, z[2]); z[3] = fmaf(w, zc[i].w, z[3]);
        }
    }
    const float inv = 1.0f / l;
    plane_store4(po, seq, head * H + c4, z[0] * inv, z[1] * inv, z[2] * inv, z[3] * inv);
}

}  // namespace

hipError_t launch_rows_ln(const float* src, int64_t stride, const float* w, const float* b, float* ln, float* copy, int rows, int H,
                          PlaneOut po, hipStream_t s, const int* vl_row0) {
    const dim3 g((rows + 3) / 4), blk(256);
    if (H == 768) hipLaunchKernelGGL(rows_ln_kernel<3>, g, blk, 0, s, src, stride, w, b, ln, copy, rows, po, vl_row0);
    else if (H == 1024) hipLaunchKernelGGL(rows_ln_kernel<4>, g, blk, 0, s, src, stride, w, b, ln, copy, rows, po, vl_row0);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

int cls_fold_chunk_rows() { return kFoldChunk; }

namespace {
template <int V4>
hipError_t launch_fold_attention(const float* x, int64_t seq_stride, const float* lw, const float* lb, const float* u, float* part, int nseq,
                                 int S, int nh, int q_log2, hipStream_t s, VarSeq vl) {
    constexpr int lds = (kFoldSub * (256 * V4 + kFoldPad) + 6 * kFoldSub * 16 + 48) * 4;
    const hipError_t e = ensure_dynamic_lds<cls_fold_attention_kernel<V4>>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((cls_fold_attention_kernel<V4>), dim3((S + kFoldChunk - 1) / kFoldChunk, nseq), dim3(512), lds, s, x, seq_stride, lw, lb, u,
                       part, S, nh, q_log2, vl);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_cls_fold(const float* q, const void* wk, int64_t w_plane, int ldw, int f16_, int wplanes, const float* x, int64_t seq_stride,
                           const float* lw, const float* lb, float* u, float* part, int nseq, int S, int H, PlaneOut zo, hipStream_t s,
                           bool q_log2, VarSeq vl) {
    if ((vl.row0 != nullptr) != (vl.len != nullptr)) return hipErrorInvalidValue;
    if (nseq < 1 || S < 1 || (H != 768 && H != 1024) || ldw < H || ldw % 4 || (wplanes != 1 && wplanes != 2) || seq_stride % 4 || !zo.p || zo.ld < (H / 64) * H)
        return hipErrorInvalidValue;
    const int nh = H / 64, nchunks = (S + kFoldChunk - 1) / kFoldChunk;
    const dim3 gk(nh, (nseq + 3) / 4), blk(256);
    hipError_t e = with_format<BF16_1 | BF16_2 | F16_1 | F16_2>(f16_ ? 1 : 0, wplanes, [&](auto t, auto planes) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cls_key_fold_kernel<T, planes.value>), gk, dim3(H), 0, s, q, (const T*)wk, w_plane, ldw, u, nseq, H);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    e = H == 768 ? launch_fold_attention<3>(x, seq_stride, lw, lb, u, part, nseq, S, nh, q_log2 ? 1 : 0, s, vl)
                 : launch_fold_attention<4>(x, seq_stride, lw, lb, u, part, nseq, S, nh, q_log2 ? 1 : 0, s, vl);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cls_fold_combine_kernel, dim3(nh, nseq), blk, 0, s, (const float*)part, nchunks, H, zo, q_log2 ? 1 : 0, vl.len);
    return hipGetLastError();
}

}  // namespace vtq
