/*
 * vtamiq_hip_weighted_sampler.h -- patches placed where a pair of images differs (csrc/patch_sampler_weighted.hip), exported by
 * libvtamiq_hip.so beside the entries of vtamiq_hip.h, whose conventions apply (device pointers unless marked HOST, asynchronous on
 * `stream`, 0 = ok, vtq_last_error).  Two unit entries: vtq_k_diff_cells reads the bytes of image pairs and fills a table of integer
 * sums; vtq_k_sample_weighted reads such a table -- or a synthetic one -- and fills the `samples` / `scale_ids` lists that the gather of
 * vtamiq_hip_images.h reads.  It has a header of its own for the reason vtamiq_hip_sampler.h has one; its footprint is pinned by
 * tests/test_gpu_weighted_sampler.py.
 *
 * THE DEFINITION -- tests/weighted_sampler_model.py restates it in numpy and Python ints and the kernels agree with that bit for bit.  It
 * has the structure of the reference's PatchSampler(diff_weight > 0, grid_type=GRID_TYPE_PERTURBED) with DIFF_TYPE_MAGNITUDE and
 * diff_pow = 1 (data/patch_sampling.py:136-171, 224-395, 601-602); parity with numpy's random stream is not a goal.
 *
 * 1. PIXEL WEIGHT (integers).  A pair is two HWC uint8 images a (reference) and b (distorted) of one size H x W, H W <= 2^22.
 *    amin, amax, bmin, bmax: each image's minimum and maximum over all 3 H W bytes;  Ra = amax - amin,  Rb = bmax - bmin.
 *        D(y, x) = sum over the 3 channels of ((a_c - amin) Rb - (b_c - bmin) Ra)^2       (<= 3 * 65025^2)
 *        m_0(y, x) = isqrt(D), the floor, exactly
 *    -- the reference's compute_diff after pil2np's per-image rescale, times the constant Ra Rb, which cancels where the reference
 *    divides by the map's standard deviation.  Level l has h = H >> l, w = W >> l and m_l(y, x) = the SUM of the 4^l level-0 values of
 *    rows [y 2^l, (y + 1) 2^l) and columns likewise: the reference's repeated AvgPool2d(2) times 4^l; rows and columns behind h 2^l,
 *    w 2^l are dropped as the pool drops them.
 *
 * 2. CELLS.  Per (pair, level) with n samples the HOST computes in fp64 exactly as numpy does
 *        cs = int(max(0.75 P, min(max(h, w) / P * 3, sqrt(h w / n * 4)))),  sh = max(1, ceil((h - P) / cs)),  sw likewise,  sh sw <= 8192
 *    and passes cs, sh, sw in; the device never computes them.  Cell c = j sw + i (row-cell j, col-cell i: the reference's flat index) has
 *        window   rows [j cs, min(h, j cs + cs + P - 1)), columns likewise: the pixels a patch anchored in the cell can cover
 *        S_c      the sum of m_l over the window;   A_c  the window's pixel count
 *        extent   rows: cs, for the last row of cells (h - P) - (sh - 1) cs; columns likewise.  An extent of 0 (a level exactly P high
 *                 or wide) is an extension: the reference produces no cells there.
 *
 * THE TABLE of a batch is uint64 [T], all of it integer sums, so no value depends on the launch geometry or on an order.  Pair p owns
 *        head_p + 0 .. 3      255 - amin, amax, 255 - bmin, bmax      (minima stored inverted: the table is zeroed and only grows)
 * and each of its levels, in the order of the level table, owns 2 + sh sw words at `tab_off`
 *        tab_off + 0, 1       sum of m_l,  sum of m_l^2  over the h w pixels of the level (< 2^64 for H W <= 2^22, l <= 3)
 *        tab_off + 2 + c      S_c
 * back to back: head_0 = 0, the first level of a pair at head + 4, the next level or pair where the last level ends.
 *
 * 3. ALLOCATION of a segment (one level of one image, n samples, weights dw = diff_weight, uw = uniform_weight), fp64 with only
 *    + - * / sqrt, each one rounded on its own (no contraction), in exactly this order; (double) of an integer is round-to-nearest:
 *        N = h w;  e1 = (double)sum_m / (double)N;  e2 = (double)sum_m2 / (double)N;  var = e2 - e1 * e1;  if var < 0: var = 0;  sd = sqrt(var)
 *        use = dw > 0 and the segment has a table and Ra > 0 and Rb > 0 and sd > 1e-6 * (double)(Ra Rb 4^l)
 *        if use:  d = dw, u = uw * sd     else:  d = 0, u = 1     (uniform: the reference divides by zero for Ra = 0 and for uw = 0 here)
 *        SS = sum of S_c, SA = sum of A_c over the cells, as integers
 *        den = d * (double)SS + u * (double)SA
 *        if not den > 0 (no weight reaches any window):  d = 0, u = 1, den = (double)SA
 *        x_c = ((double)n * (d * (double)S_c + u * (double)A_c)) / den;     k_c = ceil(x_c), clamped to 0 .. n
 *    Dissolve: E = sum of k_c - n (0 <= E < the number of non-empty cells, up to rounding), cmax = max k_c.  A non-empty cell (k_c > 0)
 *    is PREFERRED when (uint64)rng(ACCEPT, c) * cmax < (uint64)(cmax - k_c) << 32.  Order the non-empty cells by
 *    (not preferred, rng(DISSOLVE, c), c); the first min(|E|, non-empty cells) lose one sample (gain one if E < 0): the reference's "random
 *    dissolve", which takes from low counts first.  n <= 8100 = 90^2 keeps every cell's wd^2 within 8192.
 *
 * 4. PLACEMENT.  rng(purpose, index) is vtamiq_hip_sampler.h's MurmurHash3 generator of (seed, key, level, purpose, index).
 *        cell order   the non-empty cells by (rng(ORDER, c), c); a cell's samples are consecutive, its first row f_c the sum of the k of
 *                     the cells in front of it
 *        sub-cells    a cell with k samples has wd = ceil(sqrt(k)) (the smallest wd with wd^2 >= k, wd^2 <= 8192) and takes the k
 *                     sub-cells u < wd^2 of smallest (rng(SUBCELL, c * 8192 + u), u), in that order: sample f_c + rank.  Sub-cell u is
 *                     row u % wd, column u / wd (the reference's meshgrid is xy-indexed)
 *        jitter       per axis exactly vtamiq_hip_sampler.h's `coordinate` with G = wd, dim - P = the cell's extent and the bits
 *                     rng(JITTER_ROW | JITTER_COL, r), r the sample's row within the segment
 *        coordinate   j cs (or i cs) added, clamped to [0, h - P] (or [0, w - P])
 *    A segment's output is a pure function of (seed, key, level, n, cs, sh, sw, h - P, w - P, P, amount_q, dw, uw) and its table words.
 *
 * Differences from the reference, besides those of vtamiq_hip_sampler.h: m_0 is floored to an integer (under one unit of Ra Rb per
 * pixel); the dissolve is one pass by the rule above instead of repeated draws with replacement; an extent of 0, Ra = 0, Rb = 0 and
 * a total weight that vanishes give uniform sampling where the reference fails.  centerbias_weight, DIFF_TYPE_DARK, diff_pow != 1 and
 * GRID_TYPE_HALTON are not built; vtamiq_amd.sampling.WeightedPatchSampler refuses them by name.
 */
#ifndef VTAMIQ_HIP_WEIGHTED_SAMPLER_H
#define VTAMIQ_HIP_WEIGHTED_SAMPLER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTQ_WSAMPLER_ACCEPT 3
#define VTQ_WSAMPLER_DISSOLVE 4
#define VTQ_WSAMPLER_ORDER 5
#define VTQ_WSAMPLER_SUBCELL 6
#define VTQ_WSAMPLER_MAX_CELLS 8192         /* sh * sw of one level, and wd^2 (so k_c) of one cell */
#define VTQ_WSAMPLER_MAX_SAMPLES 8100       /* n of one segment: 90^2, the largest square within 8192 */
#define VTQ_WSAMPLER_MAX_PIXELS (1 << 22)   /* H * W of one image: the sum of m_l^2 stays below 2^64 up to level 3 */

/* The difference pass: NP pairs, NL (pair, level) rows, two launches and one memset on `stream`.
 *
 *   images     uint8 [image_bytes]: only bytes inside the images, [off, off + 3 H W), are read; the offsets need no alignment
 *   pairs      int64 [NP][8] = (a_off, b_off, H, W, head, the pair's first row of lev, its number of rows, 0)
 *   lev        int32 [NL][8] = (pair, level, cs, sh, sw, head, tab_off, 0), 16-byte aligned; rows ordered by pair, then by level; every
 *              pair has at least one row
 *              -- the DEVICE copies of what the HOST arrays pairs_host / lev_host say; the entry checks the host arrays and the kernels
 *              read the device ones, so the call never synchronises (vtamiq_amd.sampling.plan_samples_weighted builds them)
 *   P          patch size, 8 .. 64
 *   tab        uint64 [T], T = 4 NP + the sum of (2 + sh sw): exactly these words are written -- zeroed, then integer atomics
 *
 * Refused, with nothing launched and nothing written: a NULL pointer; a lev that is not 16-byte aligned; NP < 1, NL < 1; P outside 8 .. 64;
 * an image outside [0, image_bytes); H W > VTQ_WSAMPLER_MAX_PIXELS; a pair index that does not start at 0, decreases, skips or ends
 * before NP - 1; a level outside 0 .. 3 or not increasing within a pair; H >> level < P or W >> level < P; cs < max(1, 3 P / 4) (integer
 * division); sh or sw that is not max(1, ceil((h - P) / cs)); sh sw > VTQ_WSAMPLER_MAX_CELLS; head / tab_off that are not the back-to-back
 * layout above; a pair's head, first row or row count that disagrees with lev; T != tab_words; NP > 65535. */
int  vtq_k_diff_cells(const uint8_t* images, int64_t image_bytes, const int64_t* pairs, const int32_t* lev, const int64_t* pairs_host,
                      const int32_t* lev_host, int32_t NP, int32_t NL, int32_t P, uint64_t* tab, int64_t tab_words, void* stream);

/* The weighted sampler: NS segments, one workgroup each, one launch.
 *
 *   seg        int32 [NS][12] = (first output row, n, cs, sh, sw, h - P, w - P, level, head, tab_off, 0, 0), 16-byte aligned; head and
 *              tab_off index `tab` as above, or are both -1 for a segment without a table (sampled uniformly)
 *   keys       uint64 [NS]
 *              -- DEVICE copies of the HOST arrays seg_host / keys_host, as above
 *   tab        uint64 [tab_words], an INPUT: read at head + 0 .. 3 and tab_off + 0 .. 1 + sh sw of every segment that has a table; NULL
 *              is allowed when dw == 0 or no segment has a table (the uniform GRID_TYPE_PERTURBED grid, which needs no pixels)
 *   dw, uw     diff_weight >= 0, uniform_weight >= 0, finite, dw + uw >= 1e-6
 *   samples    int32 [total][2] = (row, col) at the segment's level;  scale_ids  int32 [total] or NULL (every level must then be 0):
 *              exactly these extents are written, with plain stores
 *
 * Refused, with nothing launched and nothing written: a NULL required pointer; a seg that is not 16-byte aligned; NS < 1; P outside
 * 8 .. 64; n < 1 or n > VTQ_WSAMPLER_MAX_SAMPLES; cs < max(1, 3 P / 4); sh, sw that are not max(1, ceil((h - P) / cs)); sh sw > 8192; h - P or w - P negative or
 * >= 2^22; a level outside 0 .. 3; first rows that are not the back-to-back prefix of the segments or a total above 2^31 - 1; scale_ids
 * NULL while any level is non-zero; amount_q outside 0 .. 65535; weights that are negative, not finite or sum below 1e-6; head / tab_off
 * negative (other than both -1), or reaching beyond tab_words; a segment with a table while tab is NULL and dw > 0. */
int  vtq_k_sample_weighted(const int32_t* seg, const uint64_t* keys, const int32_t* seg_host, const uint64_t* keys_host, int32_t NS,
                           int32_t P, const uint64_t* tab, int64_t tab_words, double dw, double uw, uint64_t seed, int32_t amount_q,
                           int32_t* samples, int32_t* scale_ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTAMIQ_HIP_WEIGHTED_SAMPLER_H */
