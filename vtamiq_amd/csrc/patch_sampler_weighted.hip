// Patches placed where a pair of images differs (include/vtamiq_hip_weighted_sampler.h, which holds the definition this file implements
// word for word): a difference pass over the bytes of the pairs that leaves integer sums in a table, and a sampler that turns the
// table into cell counts (the only fp64 of the file, every operation rounded on its own) and the counts into samples.
//
// The difference pass is two kernels.  pair_minmax_kernel streams every image once with 16-byte loads (head and tail bytes singly) and
// leaves the four extrema with one 64-bit atomic max per workgroup.  diff_cells_kernel walks tiles of 8 rows x 256 pixels: the 16 row
// segments of a tile (8 rows, two images) are staged in LDS with aligned dword loads -- only a dword that straddles the image's first or
// last byte is assembled from byte loads, so nothing outside [off, off + 3 H W) is read -- one thread owns one pixel column, the
// 2^l x 2^l blocks of the pooled levels are summed down the thread's rows and across lanes by shuffles (tiles are 8-aligned, so a block
// never leaves its wave), and the window sums are taken separably: per row-cell a line of column sums goes to LDS, then one thread per
// touched cell adds its span of the line and flushes it with ONE global 64-bit integer atomic.  No LDS atomics, no floating point.
//
// The sampler is one workgroup per segment like sample_grid_kernel, whose counting rank it reuses three times: for the dissolve order,
// for the first row of every cell (a count weighted by k) and for the sub-cells of a cell (by shuffles in one wave up to 64 samples a cell,
// by the whole workgroup against draws staged in LDS above that).
#pragma clang fp contract(off)
#include "dev_common.h"
#include "kernels.h"
#include "../../include/vtamiq_hip_sampler.h"
#include "../../include/vtamiq_hip_weighted_sampler.h"

namespace vtq {
namespace {

typedef unsigned long long u64;

constexpr int TILE_H = 8, TILE_W = 256, SPAN_DW = (3 * TILE_W + 3) / 4 + 1, ROWCELL_CHUNK = 8;

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__device__ __forceinline__ uint32_t mm3_word(uint32_t h, uint32_t k) {
    k *= 0xcc9e2d51u;
    k = rotl32(k, 15);
    k *= 0x1b873593u;
    h ^= k;
    h = rotl32(h, 13);
    return h * 5u + 0xe6546b64u;
}

__device__ __forceinline__ uint32_t mm3_prefix(uint64_t seed, uint64_t key, uint32_t level) {
    uint32_t h = mm3_word(0u, (uint32_t)seed);
    h = mm3_word(h, (uint32_t)(seed >> 32));
    h = mm3_word(h, (uint32_t)key);
    h = mm3_word(h, (uint32_t)(key >> 32));
    return mm3_word(h, level);
}

__device__ __forceinline__ uint32_t mm3_draw(uint32_t prefix, uint32_t purpose, uint32_t index) {
    uint32_t h = mm3_word(mm3_word(prefix, purpose), index);
    h ^= 28u;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    return h ^ (h >> 16);
}

// vtamiq_hip_sampler.h's `coordinate`
__device__ __forceinline__ int axis_sample(int cell, uint32_t bits24, int amount_q, int G, int extent) {
    const int64_t d = 2 * (int64_t)bits24 + 1 - (1 << 24);
    const int64_t jitter = (d * amount_q) >> 15;
    int64_t t = ((int64_t)cell << 24) + (1 << 23) + jitter;
    const int64_t full = (int64_t)G << 24;
    t = t < 0 ? 0 : (t > full ? full : t);
    const int64_t v = t * extent / full;
    return (int)(v < 0 ? 0 : (v > extent ? extent : v));
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the 4 bytes at byte offset q of `images` (an offset whose ADDRESS is 4-aligned), of which only those inside [lo, hi) are read (the others are 0)
__device__ __forceinline__ uint32_t load_dword_inside(const uint8_t* __restrict__ images, int64_t q, int64_t lo, int64_t hi) {
    if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const uint32_t*>(images + q);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (q + k >= lo && q + k < hi) v |= (uint32_t)images[q + k] << (8 * k);
    return v;
}

__device__ __forceinline__ void minmax4(uint32_t v, uint32_t& mn, uint32_t& mx) {
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = (v >> (8 * k)) & 255u;
        mn = min(mn, b);
        mx = max(mx, b);
    }
}

// pairs int64 [NP][8] = (a_off, b_off, H, W, head, first lev row, lev rows, 0); grid (x, NP); tab[head + 0 .. 3] = 255 - amin, amax, 255 - bmin, bmax
__global__ __launch_bounds__(256) void pair_minmax_kernel(const uint8_t* __restrict__ images, const long long* __restrict__ pairs,
                                                           u64* __restrict__ tab) {
    __shared__ uint32_t red[4][4];
    const long long* pr = pairs + (int64_t)blockIdx.y * 8;
    const int64_t nbytes = 3 * pr[2] * pr[3];
    uint32_t ext[4];
    for (int im = 0; im < 2; ++im) {
        const int64_t lo = pr[im], hi = lo + nbytes;                 // byte offsets into `images`
        const int64_t body = min(lo + (int64_t)((16 - (((uintptr_t)images + (uintptr_t)lo) & 15)) & 15), hi);
        const int64_t nvec = (hi - body) >> 4, tail = body + (nvec << 4);
        uint32_t mn = 255u, mx = 0u;
        for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x) {
            const uint4 q = *reinterpret_cast<const uint4*>(images + body + (v << 4));
            minmax4(q.x, mn, mx);
            minmax4(q.y, mn, mx);
            minmax4(q.z, mn, mx);
            minmax4(q.w, mn, mx);
        }
        if (blockIdx.x == 0 && threadIdx.x < 32) {                   // at most 15 bytes in front of the body and 15 behind it
            const int64_t p = threadIdx.x < 16 ? lo + threadIdx.x : tail + (threadIdx.x - 16);
            const bool in = threadIdx.x < 16 ? p < body : p < hi;
            if (in) {
                const uint32_t b = images[p];
                mn = min(mn, b);
                mx = max(mx, b);
            }
        }
        ext[2 * im] = 255u - mn;
        ext[2 * im + 1] = mx;
    }
    for (int k = 0; k < 4; ++k)
        for (int d = 32; d; d >>= 1) ext[k] = max(ext[k], (uint32_t)__shfl_xor((int)ext[k], d));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; ++k) red[wave][k] = ext[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        const uint32_t v = max(max(red[0][threadIdx.x], red[1][threadIdx.x]), max(red[2][threadIdx.x], red[3][threadIdx.x]));
        if (v) atomicMax(tab + pr[4] + threadIdx.x, (u64)v);
    }
}

__device__ __forceinline__ uint32_t isqrt_u64(u64 D) {
    // D < 2^34: the fp32 root of the rounded D is within 2^-8 of the true one, so its truncation is the floor or one beside it
    uint32_t r = (uint32_t)__fsqrt_rn((float)D);
    if ((u64)r * r > D) --r;
    if ((u64)(r + 1) * (r + 1) <= D) ++r;
    return r;
}

__device__ __forceinline__ int ceil_div_pos(int num, int den) { return num <= 0 ? 0 : (num + den - 1) / den; }

struct LevelGeom {
    int H, W, y0, x0, cs, sh, sw, P;
};

// one level of one tile: the level's values of this thread's column group (down the rows, then across 2^L lanes), the two sums of the
// level, and the window sums of the cells the tile touches
template <int L>
__device__ __forceinline__ void level_pass(const uint32_t (&m0)[TILE_H], const LevelGeom& g, u64* __restrict__ cells,
                                           uint32_t (&colbuf)[ROWCELL_CHUNK][TILE_W], u64& acc1, u64& acc2) {
    constexpr int NR = TILE_H >> L, MASK = (1 << L) - 1;
    const int t = threadIdx.x, cs = g.cs;
    const int hl = g.H >> L, wl = g.W >> L, ya = g.y0 >> L, xa = g.x0 >> L;
    const bool owner = (t & MASK) == 0 && ((g.x0 + t) >> L) < wl;
    uint32_t val[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        uint32_t v = 0;
#pragma unroll
        for (int rr = 0; rr < (1 << L); ++rr) v += m0[(r << L) + rr];
#pragma unroll
        for (int d = 1; d < (1 << L); d <<= 1) v += (uint32_t)__shfl_xor((int)v, d);
        val[r] = (owner && ya + r < hl) ? v : 0;
        acc1 += val[r];
        acc2 += (u64)val[r] * val[r];
    }
    if (ya >= hl || xa >= wl) return;                                // uniform: the tile holds only dropped rows or columns of the level
    const int yb = min(ya + NR, hl) - 1, xb = min(xa + (TILE_W >> L), wl) - 1;
    const int reach = cs + g.P - 2;                                  // pixel y is in row-cell j  <=>  j cs <= y <= j cs + reach
    const int j_lo = ceil_div_pos(ya - reach, cs), j_hi = min(g.sh - 1, yb / cs);
    const int i_lo = ceil_div_pos(xa - reach, cs), i_hi = min(g.sw - 1, xb / cs);
    const int ni = i_hi - i_lo + 1;
    for (int jc = j_lo; jc <= j_hi; jc += ROWCELL_CHUNK) {
        const int nj = min(ROWCELL_CHUNK, j_hi - jc + 1);
        if ((t & MASK) == 0)
            for (int jj = 0; jj < nj; ++jj) {
                const int top = (jc + jj) * cs;
                uint32_t s = 0;
#pragma unroll
                for (int r = 0; r < NR; ++r) s += (ya + r >= top && ya + r <= top + reach) ? val[r] : 0;
                colbuf[jj][t >> L] = s;
            }
        __syncthreads();
        for (int wk = t; wk < nj * ni; wk += blockDim.x) {
            const int jj = wk / ni, i = i_lo + wk % ni;
            const int xs = max(xa, i * cs), xe = min(xb, i * cs + reach);
            u64 s = 0;
            for (int x = xs; x <= xe; ++x) s += colbuf[jj][x - xa];
            if (s) atomicAdd(cells + (int64_t)(jc + jj) * g.sw + i, s);
        }
        __syncthreads();
    }
}

// lev int32 [NL][8] = (pair, level, cs, sh, sw, head, tab_off, 0); grid (x, NP), 256 threads
__global__ __launch_bounds__(256) void diff_cells_kernel(const uint8_t* __restrict__ images, const long long* __restrict__ pairs,
                                                          const int* __restrict__ lev, int P, u64* __restrict__ tab) {
    __shared__ uint32_t stage[2 * TILE_H][SPAN_DW];
    __shared__ uint32_t colbuf[ROWCELL_CHUNK][TILE_W];
    const long long* pr = pairs + (int64_t)blockIdx.y * 8;
    const int H = (int)pr[2], W = (int)pr[3];
    const int lev0 = (int)pr[5], nlev = min((int)pr[6], 4);
    const int64_t nbytes = (int64_t)3 * H * W;
    const int64_t lo_a = pr[0], lo_b = pr[1];                        // byte offsets into `images`
    const uintptr_t base = (uintptr_t)images;
    const u64* head = tab + pr[4];
    const int amin = 255 - (int)head[0], Ra = (int)head[1] - amin, bmin = 255 - (int)head[2], Rb = (int)head[3] - bmin;
    const int t = threadIdx.x;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles = ((H + TILE_H - 1) / TILE_H) * tiles_x;
    u64 acc1[4] = {0, 0, 0, 0}, acc2[4] = {0, 0, 0, 0};

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int y0 = (tile / tiles_x) * TILE_H, x0 = (tile % tiles_x) * TILE_W;
        const int th = min(TILE_H, H - y0), tw = min(TILE_W, W - x0);
        // stage the 2 th row segments: aligned dwords, the segment's first byte at byte (address & 3) of its line
        for (int k = 0; k < 2 * th; ++k) {
            const int64_t lo = (k & 1) ? lo_b : lo_a;
            const int64_t s = lo + (int64_t)3 * ((int64_t)(y0 + (k >> 1)) * W + x0);
            const int shift = (int)((base + (uintptr_t)s) & 3), ndw = (shift + 3 * tw + 3) >> 2;
            if (t < ndw) stage[k][t] = load_dword_inside(images, s - shift + 4 * t, lo, lo + nbytes);
        }
        __syncthreads();
        uint32_t m0[TILE_H];
        for (int r = 0; r < TILE_H; ++r) {
            m0[r] = 0;
            if (r < th && t < tw) {
                const uintptr_t row = base + (uintptr_t)((int64_t)3 * ((int64_t)(y0 + r) * W + x0));
                const uint8_t* pa = reinterpret_cast<const uint8_t*>(stage[2 * r]) + ((row + (uintptr_t)lo_a) & 3) + 3 * t;
                const uint8_t* pb = reinterpret_cast<const uint8_t*>(stage[2 * r + 1]) + ((row + (uintptr_t)lo_b) & 3) + 3 * t;
                u64 D = 0;
                for (int c = 0; c < 3; ++c) {
                    const int e = ((int)pa[c] - amin) * Rb - ((int)pb[c] - bmin) * Ra;      // |e| <= 65025
                    D += (u64)((uint32_t)(e < 0 ? -e : e) * (uint32_t)(e < 0 ? -e : e));     // e^2 < 2^32
                }
                m0[r] = isqrt_u64(D);
            }
        }
        for (int li = 0; li < 4; ++li) {
            if (li >= nlev) break;
            const int4 la = *reinterpret_cast<const int4*>(lev + (int64_t)(lev0 + li) * 8);
            const int4 lb = *reinterpret_cast<const int4*>(lev + (int64_t)(lev0 + li) * 8 + 4);
            const LevelGeom g = {H, W, y0, x0, max(la.z, 1), la.w, lb.x, P};
            u64* cells = tab + lb.z + 2;
            switch (la.y) {                                              // uniform over the workgroup
                case 0: level_pass<0>(m0, g, cells, colbuf, acc1[li], acc2[li]); break;
                case 1: level_pass<1>(m0, g, cells, colbuf, acc1[li], acc2[li]); break;
                case 2: level_pass<2>(m0, g, cells, colbuf, acc1[li], acc2[li]); break;
                default: level_pass<3>(m0, g, cells, colbuf, acc1[li], acc2[li]); break;
            }
        }
        __syncthreads();                                                 // the next tile's staging writes what this one's threads read
    }
    for (int li = 0; li < 4; ++li) {
        if (li >= nlev) break;
        const u64 s1 = wave_sum(acc1[li]), s2 = wave_sum(acc2[li]);
        if ((t & 63) == 0 && (s1 | s2)) {
            u64* st = tab + lev[(int64_t)(lev0 + li) * 8 + 6];
            atomicAdd(st, s1);
            atomicAdd(st + 1, s2);
        }
    }
}

// ---- the sampler ---------------------------------------------------------------------------------------------------------------------
constexpr int MAXC = VTQ_WSAMPLER_MAX_CELLS, SUBCHUNK = 2048;

struct Scratch {
    u64 sum[16];
    int mx[16];
};

__device__ __forceinline__ u64 block_sum(u64 v, Scratch& sc) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc.sum[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += sc.sum[k];
    return s;
}

__device__ __forceinline__ int block_max(int v, Scratch& sc) {
    for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc.mx[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = sc.mx[0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) s = max(s, sc.mx[k]);
    return s;
}

__device__ __forceinline__ int ceil_sqrt(int k) {
    int wd = (int)sqrtf((float)k);
    while (wd * wd < k) ++wd;
    while (wd > 1 && (wd - 1) * (wd - 1) >= k) --wd;
    return wd;
}

// seg int32 [NS][12] = (first output row, n, cs, sh, sw, h - P, w - P, level, head, tab_off, 0, 0); one workgroup per segment, blockDim.x
// 256 (at most 256 cells in every segment) or 1024: at most 8 cells per thread
__global__ __launch_bounds__(1024) void sample_weighted_kernel(const int* __restrict__ seg, const u64* __restrict__ keys, int P,
                                                                const u64* __restrict__ tab, double dw, double uw, u64 seed, int amount_q,
                                                                int* __restrict__ samples, int* __restrict__ scale_ids) {
    __shared__ __attribute__((aligned(16))) uint32_t dk[MAXC];       // draw per cell (dissolve, then order), then the cell's first row
    __shared__ __attribute__((aligned(16))) uint16_t kc[MAXC];       // k_c in bits 0 .. 13, `not preferred` in bit 15
    __shared__ Scratch sc;
    __shared__ uint16_t big[128];                                    // the cells of more than 64 samples
    __shared__ int nbig;
    __shared__ __attribute__((aligned(16))) uint32_t sub[SUBCHUNK];  // the draws of a large cell's sub-cells, a chunk at a time
    const int s = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    if (tid == 0) nbig = 0;                                          // read behind the barriers of the allocation
    const int4 a = *reinterpret_cast<const int4*>(seg + (int64_t)s * 12);
    const int4 b = *reinterpret_cast<const int4*>(seg + (int64_t)s * 12 + 4);
    const int4 c4 = *reinterpret_cast<const int4*>(seg + (int64_t)s * 12 + 8);
    const int row0 = a.x, cs = max(a.z, 1), sh = max(a.w, 1), sw = max(b.x, 1), hm = b.y, wm = b.z, level = b.w & 3;
    const int M = min(sh * sw, MAXC);                                // addressing only: the entry has checked the host copy of the table
    const int n = min(max(a.y, 1), VTQ_WSAMPLER_MAX_SAMPLES);
    const int h = hm + P, w = wm + P, reach = cs + P - 1;
    const uint32_t prefix = mm3_prefix(seed, keys[s], (uint32_t)level);
    const int M4 = (M + 3) & ~3;

    // ---- allocation: fp64, each operation rounded on its own, in the header's order
    bool use = dw > 0.0 && tab != nullptr && c4.x >= 0 && c4.y >= 0;
    const u64* cellsum = nullptr;
    double sd = 0.0;
    if (use) {
        const u64* head = tab + c4.x;
        const u64* st = tab + c4.y;
        cellsum = st + 2;
        const long long Ra = (long long)head[1] - (255 - (long long)head[0]), Rb = (long long)head[3] - (255 - (long long)head[2]);
        const double N = (double)((long long)h * w);
        const double e1 = __ddiv_rn((double)st[0], N), e2 = __ddiv_rn((double)st[1], N);
        double var = __dsub_rn(e2, __dmul_rn(e1, e1));
        if (var < 0.0) var = 0.0;
        sd = __dsqrt_rn(var);
        use = Ra > 0 && Rb > 0 && sd > __dmul_rn(1e-6, (double)(Ra * Rb * (1ll << (2 * level))));
    }
    u64 mySS = 0, mySA = 0;
    for (int c = tid; c < M; c += T) {
        const int j = c / sw, i = c % sw;
        mySA += (u64)(min(h, j * cs + reach) - j * cs) * (u64)(min(w, i * cs + reach) - i * cs);
        if (use) mySS += cellsum[c];
    }
    const u64 SA = block_sum(mySA, sc), SS = block_sum(mySS, sc);
    double d = use ? dw : 0.0, u = use ? __dmul_rn(uw, sd) : 1.0;
    double den = __dadd_rn(__dmul_rn(d, (double)SS), __dmul_rn(u, (double)SA));
    if (!(den > 0.0)) {                                              // no weight reaches any window: uniform
        use = false;
        d = 0.0;
        u = 1.0;
        den = (double)SA;
    }
    int myk = 0, mymax = 0, mynz = 0;
    for (int c = tid; c < M4; c += T) {
        int k = 0;
        if (c < M) {
            const int j = c / sw, i = c % sw;
            const u64 A = (u64)(min(h, j * cs + reach) - j * cs) * (u64)(min(w, i * cs + reach) - i * cs);
            const u64 S = use ? cellsum[c] : 0;
            const double x = __ddiv_rn(__dmul_rn((double)n, __dadd_rn(__dmul_rn(d, (double)S), __dmul_rn(u, (double)A))), den);
            const double cx = ceil(x);
            k = cx >= (double)n ? n : (cx > 0.0 ? (int)cx : 0);
        }
        kc[c] = (uint16_t)k;                                          // the pad cells are empty
        myk += k;
        mymax = max(mymax, k);
        mynz += k > 0;
    }
    const int sumk = (int)block_sum((u64)myk, sc), nonempty = (int)block_sum((u64)mynz, sc), cmax = block_max(mymax, sc);
    const int E = sumk - n, nE = min(E < 0 ? -E : E, nonempty);

    // ---- dissolve: the first nE non-empty cells by (not preferred, draw, c) lose (gain, if E < 0) one sample
    if (nE > 0) {                                                    // uniform over the workgroup
        for (int c = tid; c < M; c += T) {
            const int k = kc[c];
            dk[c] = mm3_draw(prefix, VTQ_WSAMPLER_DISSOLVE, (uint32_t)c);
            const bool pref = (u64)mm3_draw(prefix, VTQ_WSAMPLER_ACCEPT, (uint32_t)c) * (u64)cmax < ((u64)(cmax - k) << 32);
            if (k > 0 && !pref) kc[c] = (uint16_t)(k | 0x8000);
        }
        __syncthreads();
        uint32_t hit = 0;
        int slot = 0;
        for (int c = tid; c < M; c += T, ++slot) {
            const int kme = kc[c];
            if (!(kme & 0x3fff)) continue;
            const u64 mine = ((u64)(kme >> 15) << 45) | ((u64)dk[c] << 13) | (u64)c;
            int rank = 0;
            for (int j = 0; j < M4; j += 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(dk + j);
                const uint2 kk = *reinterpret_cast<const uint2*>(kc + j);
                const uint32_t k0 = kk.x & 0xffffu, k1 = kk.x >> 16, k2 = kk.y & 0xffffu, k3 = kk.y >> 16;
                rank += ((k0 & 0x3fff) != 0 && ((((u64)(k0 >> 15) << 45) | ((u64)q.x << 13) | (u64)j) < mine)) +
                        ((k1 & 0x3fff) != 0 && ((((u64)(k1 >> 15) << 45) | ((u64)q.y << 13) | (u64)(j + 1)) < mine)) +
                        ((k2 & 0x3fff) != 0 && ((((u64)(k2 >> 15) << 45) | ((u64)q.z << 13) | (u64)(j + 2)) < mine)) +
                        ((k3 & 0x3fff) != 0 && ((((u64)(k3 >> 15) << 45) | ((u64)q.w << 13) | (u64)(j + 3)) < mine));
            }
            if (rank < nE) hit |= 1u << slot;
        }
        __syncthreads();
        slot = 0;
        for (int c = tid; c < M; c += T, ++slot) {
            const int k = kc[c] & 0x3fff;
            kc[c] = (uint16_t)(((hit >> slot) & 1u) ? (E > 0 ? k - 1 : k + 1) : k);
        }
    }
    __syncthreads();

    // ---- cell order: the first row of a cell is the k of the non-empty cells in front of it under (draw, c)
    for (int c = tid; c < M4; c += T) dk[c] = c < M ? mm3_draw(prefix, VTQ_WSAMPLER_ORDER, (uint32_t)c) : 0xffffffffu;
    __syncthreads();
    uint32_t first[8];
    {
        int slot = 0;
        for (int c = tid; c < M && slot < 8; c += T, ++slot) {
            first[slot] = 0;
            if (!kc[c]) continue;
            const u64 mine = ((u64)dk[c] << 32) | (uint32_t)c;
            uint32_t f = 0;
            for (int j = 0; j < M4; j += 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(dk + j);
                const uint2 kk = *reinterpret_cast<const uint2*>(kc + j);
                f += ((((u64)q.x << 32) | (uint32_t)j) < mine ? (kk.x & 0xffffu) : 0u) + ((((u64)q.y << 32) | (uint32_t)(j + 1)) < mine ? (kk.x >> 16) : 0u) +
                     ((((u64)q.z << 32) | (uint32_t)(j + 2)) < mine ? (kk.y & 0xffffu) : 0u) + ((((u64)q.w << 32) | (uint32_t)(j + 3)) < mine ? (kk.y >> 16) : 0u);
            }
            first[slot] = f;
        }
        __syncthreads();
        slot = 0;
        for (int c = tid; c < M && slot < 8; c += T, ++slot) dk[c] = first[slot];
    }
    __syncthreads();

    // ---- placement.  Every sub-cell's draw is made once; the rank of a sub-cell is counted against the cell's draws
    auto emit = [&](int c, int uu, int rank, int k, int f, int wd) {
        const int r = f + rank;
        if (rank >= k || r >= n) return;
        const int j = c / sw, i = c % sw;
        const int ext_r = j == sh - 1 ? max(hm - (sh - 1) * cs, 0) : cs, ext_c = i == sw - 1 ? max(wm - (sw - 1) * cs, 0) : cs;
        const uint32_t br = mm3_draw(prefix, VTQ_SAMPLER_JITTER_ROW, (uint32_t)r) >> 8;
        const uint32_t bc = mm3_draw(prefix, VTQ_SAMPLER_JITTER_COL, (uint32_t)r) >> 8;
        const int y = min(max(j * cs + axis_sample(uu % wd, br, amount_q, wd, ext_r), 0), hm);
        const int x = min(max(i * cs + axis_sample(uu / wd, bc, amount_q, wd, ext_c), 0), wm);
        const int64_t o = (int64_t)row0 + r;
        *reinterpret_cast<int2*>(samples + o * 2) = make_int2(y, x);
        if (scale_ids) scale_ids[o] = level;
    };
    // cells of at most 64 samples (wd^2 <= 64): one wave per cell, one lane per sub-cell, the draws exchanged by shuffles
    const int lane = tid & 63, nw = T >> 6;
    for (int c = tid >> 6; c < M; c += nw) {
        const int k = kc[c];
        if (!k || k > 64) continue;                                  // wave-uniform
        const int wd = ceil_sqrt(k), W2 = wd * wd;
        const u64 mine = lane < W2 ? (((u64)mm3_draw(prefix, VTQ_WSAMPLER_SUBCELL, (uint32_t)c * (uint32_t)MAXC + (uint32_t)lane) << 32) | (uint32_t)lane) : ~0ull;
        int rank = 0;
        for (int v = 0; v < W2; ++v) rank += __shfl(mine, v) < mine;
        if (lane < W2) emit(c, lane, rank, k, (int)dk[c], wd);
    }
    // larger cells (up to 8100 samples in one): the whole workgroup per cell, the draws staged in LDS SUBCHUNK at a time, up to eight
    // sub-cells per thread and pass; wd^4 compares, wd^2 draws per pass
    for (int c = tid; c < M; c += T)
        if (kc[c] > 64) big[atomicAdd(&nbig, 1) & 127] = (uint16_t)c; // at most n / 65 <= 124 such cells; their order does not matter
    __syncthreads();
    for (int b = 0; b < min(nbig, 128); ++b) {                       // uniform over the workgroup
        const int c = big[b], k = kc[c];
        const int f = (int)dk[c], wd = ceil_sqrt(k), W2 = wd * wd;
        const uint32_t base = (uint32_t)c * (uint32_t)MAXC;
        for (int u0 = 0; u0 < W2; u0 += 8 * T) {
            u64 mine[8];
            int rank[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int uu = u0 + tid + i * T;
                mine[i] = uu < W2 ? (((u64)mm3_draw(prefix, VTQ_WSAMPLER_SUBCELL, base + (uint32_t)uu) << 32) | (uint32_t)uu) : 0ull;
                rank[i] = 0;
            }
            for (int v0 = 0; v0 < W2; v0 += SUBCHUNK) {
                const int nv = min(SUBCHUNK, (W2 - v0 + 3) & ~3);    // the pad draws are the largest value at indices behind every sub-cell
                __syncthreads();
                for (int v = tid; v < nv; v += T) sub[v] = v0 + v < W2 ? mm3_draw(prefix, VTQ_WSAMPLER_SUBCELL, base + (uint32_t)(v0 + v)) : 0xffffffffu;
                __syncthreads();
                for (int v = 0; v < nv; v += 4) {
                    const uint4 q = *reinterpret_cast<const uint4*>(sub + v);
                    const u64 k0 = ((u64)q.x << 32) | (uint32_t)(v0 + v), k1 = ((u64)q.y << 32) | (uint32_t)(v0 + v + 1),
                              k2 = ((u64)q.z << 32) | (uint32_t)(v0 + v + 2), k3 = ((u64)q.w << 32) | (uint32_t)(v0 + v + 3);
#pragma unroll
                    for (int i = 0; i < 8; ++i) rank[i] += (k0 < mine[i]) + (k1 < mine[i]) + (k2 < mine[i]) + (k3 < mine[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int uu = u0 + tid + i * T;
                if (uu < W2) emit(c, uu, rank[i], k, f, wd);
            }
        }
    }
}

}  // namespace

hipError_t launch_diff_cells(const uint8_t* images, const int64_t* pairs, const int* lev, int NP, int64_t max_pixels, int P, uint64_t* tab,
                             int64_t tab_words, hipStream_t s) {
    if (NP < 1 || NP > 65535 || max_pixels < 1 || max_pixels > VTQ_WSAMPLER_MAX_PIXELS || tab_words < 1) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(tab, 0, (size_t)tab_words * 8, s);
    if (e != hipSuccess) return e;
    // neither result depends on the grid: sized so that one image of the largest size gives every workgroup a few thousand pixels
    const int gx = (int)std::min<int64_t>(64, (3 * max_pixels / 16 + 256 * 8 - 1) / (256 * 8));
    hipLaunchKernelGGL(pair_minmax_kernel, dim3((unsigned)std::max(gx, 1), (unsigned)NP), dim3(256), 0, s, images, (const long long*)pairs,
                       (u64*)tab);
    const int gt = (int)std::min<int64_t>(128, (max_pixels + TILE_H * TILE_W - 1) / (TILE_H * TILE_W) + 1);
    hipLaunchKernelGGL(diff_cells_kernel, dim3((unsigned)gt, (unsigned)NP), dim3(256), 0, s, images, (const long long*)pairs, lev, P, (u64*)tab);
    return hipGetLastError();
}

hipError_t launch_sample_weighted(const int* seg, const uint64_t* keys, int NS, int max_cells, int P, const uint64_t* tab, double dw, double uw,
                                  uint64_t seed, int amount_q, int* samples, int* scale_ids, hipStream_t s) {
    if (NS < 1 || max_cells < 1 || max_cells > VTQ_WSAMPLER_MAX_CELLS || amount_q < 0 || amount_q > 65535) return hipErrorInvalidValue;
    // the result does not depend on the workgroup size; sixteen waves as soon as a segment has more cells than four waves have lanes
    const int threads = max_cells <= 256 ? 256 : 1024;
    hipLaunchKernelGGL(sample_weighted_kernel, dim3((unsigned)NS), dim3(threads), 0, s, seg, (const u64*)keys, P, (const u64*)tab, dw, uw,
                       (u64)seed, amount_q, samples, scale_ids);
    return hipGetLastError();
}

}  // namespace vtq
