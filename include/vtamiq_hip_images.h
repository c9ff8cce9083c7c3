/*
 * vtamiq_hip_images.h -- the image front end for images of DIFFERENT sizes (csrc/patches_ragged.hip), exported by libvtamiq_hip.so beside
 * the entries of vtamiq_hip.h, whose conventions apply (device pointers unless marked HOST, asynchronous on `stream`, 0 = ok,
 * vtq_last_error).  It has a header of its own because the per-kernel table of vtamiq_hip.h is pinned entry by entry by
 * tests/test_gpu_footprint.py; the footprint of this entry is pinned by tests/test_gpu_image_varlen.py.
 */
#ifndef VTAMIQ_HIP_IMAGES_H
#define VTAMIQ_HIP_IMAGES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* uint8 images of NI different sizes -> the (patches, pos, scales) call tensors of vtq_forward_varlen / the *_varlen group entries, in one
 * launch and without any image-sized intermediate: vtq_k_image_normalize + vtq_k_avgpool2 + vtq_k_gather_patches of vtamiq_hip.h fused,
 * per patch.  Every output element has the BITS those three give for its image alone.
 *
 * Image i is H[i] x W[i] x 3 bytes (HWC) at byte img_off[i] of `images`; the images need not be in order, adjacent or aligned (a 17 x 33
 * image is 1683 bytes: its successor starts at an odd address), but each lies inside the buffer.  Image i owns the patch rows
 * [row0[i], row0[i + 1]) of samples / scale_ids / patches / pos / scales; total = row0[NI].
 *
 *   images     uint8, exactly image_bytes bytes.  Only bytes [img_off[i], img_off[i] + 3 H[i] W[i]) of an image with patches are read, one
 *              byte at a time: nothing in front of, between or behind the images, whatever their alignment
 *   tab        int32 [NI][4] = (img_off[i] low word, high word, H[i], W[i]): exactly 4 NI int32, 16-byte aligned
 *   patch_img  int32 [total]: the image of every patch row (patch_img[r] = i for row0[i] <= r < row0[i + 1])
 *              -- tab and patch_img are the DEVICE copies of what the HOST arrays below say; the entry checks the host arrays and the
 *              kernel reads the device ones, so that a caller who keeps both in one pinned block uploads them with its samples in one copy
 *              and the call never synchronises (vtamiq_amd.patches.image_tables builds them)
 *   img_off    HOST int64 [NI];  H, W: HOST int32 [NI];  row0: HOST int32 [NI + 1], row0[0] = 0, non-decreasing, row0[NI] >= 1
 *   samples    int32 [total][2] = (row, col) at the patch's own pyramid level s: 0 <= row <= (H >> s) - P, 0 <= col <= (W >> s) - P, which
 *              also says that level s of THAT image holds a patch: in a batch of different sizes a small image uses fewer levels than
 *              num_scales.  The kernel does not report a sample or level outside that range (the caller checks on the host); it clamps
 *              both for addressing, so the reads stay inside the image even then
 *   scale_ids  int32 [total] in [0, num_scales), or NULL (all level 0; num_scales must then be 1)
 *   flips      int32 [NI][2] = (hflip, vflip), or NULL.  Flips apply at level 0, before the pooling: a pooled level of an odd dimension
 *              drops the last row / column of the FLIPPED image
 *   mean, std  HOST float[3]
 *   patches    fp32 [total][3][P][P];  pos fp32 [total][2] = clamp((sample + P/2) / (dim_s - P/2), 0, 1 - 1e-6), dim_s = dim >> s;
 *              scales fp32 [total] (the ids as floats) or NULL.  Exactly these extents are written, with plain stores
 *
 * Refused, with nothing launched: a NULL required pointer (everything but scale_ids, flips, scales); a tab that is not 16-byte aligned;
 * NI < 1; row0[0] != 0, a decreasing row0 or row0[NI] < 1; patch_size other than 16 | 8; num_scales outside 1 .. 4; scale_ids NULL with
 * num_scales > 1; an image that leaves the buffer (img_off[i] < 0 or img_off[i] + 3 H[i] W[i] > image_bytes); an image smaller than one
 * patch (H[i] < P or W[i] < P). */
int  vtq_k_gather_patches_u8(const uint8_t* images, int64_t image_bytes, const int32_t* tab, const int32_t* patch_img,
                             const int64_t* img_off, const int32_t* H, const int32_t* W, const int32_t* row0, int32_t NI,
                             const int32_t* samples, const int32_t* scale_ids, const int32_t* flips, const float* mean, const float* std_,
                             float* patches, float* pos, float* scales, int32_t patch_size, int32_t num_scales, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTAMIQ_HIP_IMAGES_H */
