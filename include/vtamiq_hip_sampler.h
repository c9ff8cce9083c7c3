/*
 * vtamiq_hip_sampler.h -- patch coordinates sampled on the device (csrc/patch_sampler.hip), exported by libvtamiq_hip.so beside the entries
 * of vtamiq_hip.h, whose conventions apply (device pointers unless marked HOST, asynchronous on `stream`, 0 = ok, vtq_last_error).  It fills
 * the `samples` / `scale_ids` lists that the gather of vtamiq_hip_images.h reads, so the coordinates never exist on the host.  It has
 * a header of its own for the reason vtamiq_hip_images.h has one; its footprint is pinned by tests/test_gpu_sampler.py.
 *
 * THE DEFINITION -- integers only; tests/sampler_model.py restates it in numpy and the kernel agrees with that bit for bit.
 * It has the structure of the reference's default sampler, PatchSampler(grid_type=GRID_TYPE_PERTURBED_SIMPLE)
 * (data/patch_sampling.py:308-395); parity with numpy's random stream is not a goal.
 *
 * A SEGMENT is one (image, pyramid level): n >= 1 samples on a level of h x w pixels (h = H >> level, w = W >> level, both >= P), a 64-bit
 * key, and a grid of Hg x Wg cells, M = Hg Wg >= n, which the HOST computes in fp64 exactly as numpy does in the reference,
 *     Wg = max(ceil(sqrt(n / (h / w))), 1),  Hg = ceil(Wg * (h / w)),
 * and passes in the segment table: the device never computes them.
 *
 * rng(seed, key, level, purpose, index) -> u32 is MurmurHash3_x86_32 (Appleby, public domain) with seed 0 of the 28-byte message of the
 * seven little-endian 32-bit words (seed low, seed high, key low, key high, level, purpose, index); all arithmetic mod 2^32:
 *     h = 0;  for each word k:  k *= 0xcc9e2d51;  k = rotl(k, 15);  k *= 0x1b873593;  h ^= k;  h = rotl(h, 13);  h = h * 5 + 0xe6546b64
 *     h ^= 28;  h ^= h >> 16;  h *= 0x85ebca6b;  h ^= h >> 13;  h *= 0xc2b2ae35;  h ^= h >> 16
 * purpose: VTQ_SAMPLER_CELL 0, VTQ_SAMPLER_JITTER_ROW 1, VTQ_SAMPLER_JITTER_COL 2.  A segment's output is a pure function of
 * (seed, key, level, n, Hg, Wg, h - P, w - P, amount_q): not of its place in the batch, of the other segments or of the launch geometry.
 *
 *   cell choice   the M cells ordered by (rng(.., CELL, c), c) ascending; sample r = 0 .. n - 1 takes the cell of rank r: a uniformly random
 *                 n-subset in random order (np.random.choice(M, n, replace=False)).  Cell c is row-cell c % Hg, col-cell c / Hg (the
 *                 reference's meshgrid is xy-indexed)
 *   jitter        per axis b = rng(.., JITTER_ROW | JITTER_COL, r) >> 8 (24 bits);  d = 2 b + 1 - 2^24 (odd, symmetric about 0);
 *                 jitter = (d * amount_q) >> 15, an arithmetic (flooring) shift of the int64 product, in 2^-24 cell units: within
 *                 +-2 perturbed_amount of a cell for amount_q = round(perturbed_amount * 2^16), 0 <= amount_q <= 65535 (0.2 -> 13107)
 *   coordinate    t = cell * 2^24 + 2^23 + jitter, clamped to [0, G * 2^24], G = Hg for rows, Wg for columns;
 *                 sample = floor(t * (dim - P) / (G * 2^24)) in int64, clamped to [0, dim - P]: the reference's
 *                 clip((cell + jitter) / G + 1 / (2 G), 0, 1) * (dim - P), truncated as its fancy indexing truncates
 *
 * Two deliberate differences from the reference.  (1) It computes `pos` from the real-valued sample; the gather computes it from the
 * integer sample, as this project always has: under one pixel.  (2) GRID_TYPE_PERTURBED, GRID_TYPE_HALTON, non-zero diff_weight /
 * centerbias_weight (which the SIMPLE grid ignores, with a warning, in the reference too) and randomize_patch_scale_order=True are not
 * built; vtamiq_amd.sampling refuses them by name.
 * Alignment needs no mechanism: two images sampled with one key, size and count get the same rows.
 */
#ifndef VTAMIQ_HIP_SAMPLER_H
#define VTAMIQ_HIP_SAMPLER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTQ_SAMPLER_CELL 0
#define VTQ_SAMPLER_JITTER_ROW 1
#define VTQ_SAMPLER_JITTER_COL 2
#define VTQ_SAMPLER_MAX_CELLS 8192          /* Hg * Wg of one segment: the cell keys of a segment live in one workgroup's LDS (32 KB) */
#define VTQ_SAMPLER_MAX_EXTENT (1 << 26)    /* h - P, w - P below this: t * (dim - P) stays inside int64 */

/* NS segments, one workgroup each, one launch.
 *
 *   seg        int32 [NS][8] = (first output row, n, Hg, Wg, h - P, w - P, level, 0): exactly 8 NS int32, 16-byte aligned
 *   keys       uint64 [NS]
 *              -- the DEVICE copies of what the HOST arrays seg_host / keys_host say; the entry checks the host arrays and the kernel reads
 *              the device ones, so a caller who keeps both in one pinned block uploads them in one copy and the call never synchronises
 *              (vtamiq_amd.sampling.plan_samples builds them)
 *   seed       any 64-bit value;  amount_q: round(perturbed_amount * 2^16)
 *   samples    int32 [total][2] = (row, col) at the segment's level, total = the sum of n; segment j owns rows [first_j, first_j + n_j)
 *   scale_ids  int32 [total] = the segment's level, or NULL (every level must then be 0)
 *              Exactly these extents are written, with plain stores: the layout vtq_k_gather_patches_u8 reads.
 *
 * Refused, with nothing launched: a NULL required pointer (everything but scale_ids); a seg that is not 16-byte aligned; NS < 1;
 * n < 1 or n > Hg Wg; Hg < 1, Wg < 1 or Hg Wg > VTQ_SAMPLER_MAX_CELLS (8192); h - P or w - P negative or >= VTQ_SAMPLER_MAX_EXTENT; a
 * level outside 0 .. 3; first rows that are not the back-to-back prefix of the segments (first_0 = 0, first_j+1 = first_j + n_j) or a total
 * above 2^31 - 1; scale_ids NULL while any level is non-zero; amount_q outside 0 .. 65535. */
int  vtq_k_sample_grid(const int32_t* seg, const uint64_t* keys, const int32_t* seg_host, const uint64_t* keys_host, int32_t NS,
                       uint64_t seed, int32_t amount_q, int32_t* samples, int32_t* scale_ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTAMIQ_HIP_SAMPLER_H */
