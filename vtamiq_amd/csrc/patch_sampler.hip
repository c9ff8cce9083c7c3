// Patch coordinates sampled on the device (include/vtamiq_hip_sampler.h, which holds the definition this file implements word for word):
// the reference's default sampler -- a perturbed grid of Hg x Wg cells, n of them chosen without replacement in random order, one jittered
// sample per chosen cell -- as a pure integer function of (seed, key, level, n, Hg, Wg, h - P, w - P, amount_q).
//
// One workgroup per segment (image, pyramid level).  The M = Hg Wg <= 8192 cell keys rng(.., CELL, c) go to LDS (32 KB at most); the rank
// of cell c under the order (key, c) is the number of cells in front of it, counted against the whole key array with wave-uniform 16-byte
// LDS reads (one address per wave: a broadcast, no bank conflict).  That is M^2 / 2 compares per segment -- 135 k for the N = 500 grid of
// 26 x 20 cells, 34 M at the 8192-cell limit (N = 5000: about 13 M) -- where a sort would need M log^2 M; the count is chosen because it is
// branch-free, needs no padding to a power of two and honours the tie-break by construction, and a segment's time stays far below the
// forward of the patches it produces.  The cell of rank r < n then writes sample r: nothing is exchanged after the count.
#include "dev_common.h"
#include "kernels.h"
#include "../../include/vtamiq_hip_sampler.h"

namespace vtq {
namespace {

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// one 32-bit word into the MurmurHash3_x86_32 state
__device__ __forceinline__ uint32_t mm3_word(uint32_t h, uint32_t k) {
    k *= 0xcc9e2d51u;
    k = rotl32(k, 15);
    k *= 0x1b873593u;
    h ^= k;
    h = rotl32(h, 13);
    return h * 5u + 0xe6546b64u;
}

// the state behind (seed low, seed high, key low, key high, level): the same for every draw of a segment
__device__ __forceinline__ uint32_t mm3_prefix(uint64_t seed, uint64_t key, uint32_t level) {
    uint32_t h = mm3_word(0u, (uint32_t)seed);
    h = mm3_word(h, (uint32_t)(seed >> 32));
    h = mm3_word(h, (uint32_t)key);
    h = mm3_word(h, (uint32_t)(key >> 32));
    return mm3_word(h, level);
}

__device__ __forceinline__ uint32_t mm3_draw(uint32_t prefix, uint32_t purpose, uint32_t index) {
    uint32_t h = mm3_word(mm3_word(prefix, purpose), index);
    h ^= 28u;                                                        // the message length in bytes
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    return h ^ (h >> 16);
}

// cell index + 24 random bits -> the integer sample on an axis of G cells and `extent` = dim - P
__device__ __forceinline__ int axis_sample(int cell, uint32_t bits24, int amount_q, int G, int extent) {
    const int64_t d = 2 * (int64_t)bits24 + 1 - (1 << 24);
    const int64_t jitter = (d * amount_q) >> 15;                     // arithmetic shift: floor
    int64_t t = ((int64_t)cell << 24) + (1 << 23) + jitter;
    const int64_t full = (int64_t)G << 24;
    t = t < 0 ? 0 : (t > full ? full : t);
    const int64_t v = t * extent / full;
    return (int)(v < 0 ? 0 : (v > extent ? extent : v));
}

// seg: int32 [NS][8] = (first output row, n, Hg, Wg, h - P, w - P, level, 0); one workgroup per segment, any blockDim.x
__global__ __launch_bounds__(1024) void sample_grid_kernel(const int* __restrict__ seg, const unsigned long long* __restrict__ keys,
                                                            unsigned long long seed, int amount_q, int* __restrict__ samples,
                                                            int* __restrict__ scale_ids) {
    __shared__ __attribute__((aligned(16))) uint32_t ck[VTQ_SAMPLER_MAX_CELLS];
    const int s = blockIdx.x;
    const int4 a = *reinterpret_cast<const int4*>(seg + (int64_t)s * 8);
    const int4 b = *reinterpret_cast<const int4*>(seg + (int64_t)s * 8 + 4);
    const int row0 = a.x, Hg = a.z, Wg = a.w, hm = b.x, wm = b.y, level = b.z;
    const int M = min(Hg * Wg, VTQ_SAMPLER_MAX_CELLS);               // addressing only: the entry has checked the host copy of the table
    const int n = min(a.y, M);
    const uint32_t prefix = mm3_prefix(seed, keys[s], (uint32_t)level);
    const int M4 = (M + 3) & ~3;                                     // pad keys: the largest value at an index behind every cell, never in front of one
    for (int c = threadIdx.x; c < M4; c += blockDim.x) ck[c] = c < M ? mm3_draw(prefix, VTQ_SAMPLER_CELL, (uint32_t)c) : 0xffffffffu;
    __syncthreads();
    for (int c = threadIdx.x; c < M; c += blockDim.x) {
        const uint64_t mine = ((uint64_t)ck[c] << 32) | (uint32_t)c;
        int rank = 0;
        for (int j = 0; j < M4; j += 4) {
            const uint4 k = *reinterpret_cast<const uint4*>(ck + j);
            rank += ((((uint64_t)k.x << 32) | (uint32_t)j) < mine) + ((((uint64_t)k.y << 32) | (uint32_t)(j + 1)) < mine) +
                    ((((uint64_t)k.z << 32) | (uint32_t)(j + 2)) < mine) + ((((uint64_t)k.w << 32) | (uint32_t)(j + 3)) < mine);
        }
        if (rank < n) {
            const int cr = c % Hg, cc = c / Hg;
            const uint32_t br = mm3_draw(prefix, VTQ_SAMPLER_JITTER_ROW, (uint32_t)rank) >> 8;
            const uint32_t bc = mm3_draw(prefix, VTQ_SAMPLER_JITTER_COL, (uint32_t)rank) >> 8;
            const int64_t o = (int64_t)row0 + rank;
            *reinterpret_cast<int2*>(samples + o * 2) = make_int2(axis_sample(cr, br, amount_q, Hg, hm), axis_sample(cc, bc, amount_q, Wg, wm));
            if (scale_ids) scale_ids[o] = level;
        }
    }
}

}  // namespace

hipError_t launch_sample_grid(const int* seg, const uint64_t* keys, int NS, int max_cells, uint64_t seed, int amount_q, int* samples,
                              int* scale_ids, hipStream_t s) {
    if (NS < 1 || max_cells < 1 || max_cells > VTQ_SAMPLER_MAX_CELLS || amount_q < 0 || amount_q > 65535) return hipErrorInvalidValue;
    // the result does not depend on the workgroup size.  Sixteen waves as soon as a grid has more cells than four waves have lanes: the
    // count is a dependent chain of LDS reads and compares, and one wave per SIMD issues it several times slower than four do
    // (profiles/r16_sampler.txt: the sampler alone)
    const int threads = max_cells <= 256 ? 256 : 1024;
    hipLaunchKernelGGL(sample_grid_kernel, dim3((unsigned)NS), dim3(threads), 0, s, seg, (const unsigned long long*)keys,
                       (unsigned long long)seed, amount_q, samples, scale_ids);
    return hipGetLastError();
}

}  // namespace vtq
