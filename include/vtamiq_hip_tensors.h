/*
 * vtamiq_hip_tensors.h -- the image front end for FLOAT images that are already on the device (csrc/patches_planar.hip): the output of
 * another model, scored without a quantisation to 8 bits.  Exported by libvtamiq_hip.so beside the entries of vtamiq_hip.h, whose
 * conventions apply (device pointers unless marked HOST, asynchronous on `stream`, 0 = ok, vtq_last_error).  It has a header of its own
 * because the per-kernel table of vtamiq_hip.h is pinned entry by entry by tests/test_gpu_footprint.py, and the set of
 * vtamiq_hip_images.h by tests/test_image_varlen_layout.py; the footprint of this entry is pinned by tests/test_gpu_tensor_metric.py.
 */
#ifndef VTAMIQ_HIP_TENSORS_H
#define VTAMIQ_HIP_TENSORS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTQ_PIXEL_F32 0
#define VTQ_PIXEL_F16 1
#define VTQ_PIXEL_BF16 2

/* Float images of NI different sizes -> the (patches, pos, scales) call tensors of vtq_forward_varlen / the *_varlen group entries, in one
 * launch and without any image-sized intermediate: vtq_k_gather_patches_u8 of vtamiq_hip_images.h for planar float pixels.
 *
 * Image i is three contiguous planes (CHW) of H[i] x W[i] elements of `dtype` at BYTE img_off[i] of `images`: element size E = 4 (fp32) or
 * 2 (fp16, bf16).  The images need not be in order or adjacent; img_off[i] is a multiple of E and needs no further alignment (a 17 x 33
 * fp16 image is 3366 bytes: its successor is 2-byte aligned only), and each image lies inside the buffer.  Image i owns the patch rows
 * [row0[i], row0[i + 1]) of samples / scale_ids / patches / pos / scales; total = row0[NI].
 *
 * Arithmetic, with no fused multiply-add: level 0 is ((float)x - mean[c]) / std[c], a true division, of the FLIPPED image's pixel; level s
 * the nested 2 x 2 sums of level s - 1 in (0,0), (0,1), (1,0), (1,1) order then / 4, s times.  Flips apply at level 0, before the
 * pooling: a pooled level of an odd dimension drops the last row / column of the FLIPPED image.  A NaN or infinite pixel reaches the
 * output elements it is pooled into and no others.
 *
 *   images     exactly image_bytes bytes.  Only bytes [img_off[i], img_off[i] + 3 H[i] W[i] E) of an image with patches are read, one
 *              element at a time: nothing in front of, between or behind the images, whatever their alignment
 *   dtype      VTQ_PIXEL_F32 | VTQ_PIXEL_F16 | VTQ_PIXEL_BF16, one for the whole call
 *   tab        int32 [NI][4] = (img_off[i] low word, high word, H[i], W[i]): exactly 4 NI int32, 16-byte aligned
 *   patch_img  int32 [total]: the image of every patch row (patch_img[r] = i for row0[i] <= r < row0[i + 1])
 *              -- tab and patch_img are the DEVICE copies of what the HOST arrays below say; the entry checks the host arrays and the
 *              kernel reads the device ones, so the call never synchronises
 *   img_off    HOST int64 [NI], bytes;  H, W: HOST int32 [NI];  row0: HOST int32 [NI + 1], row0[0] = 0, non-decreasing, row0[NI] >= 1
 *   samples    int32 [total][2] = (row, col) at the patch's own pyramid level s: 0 <= row <= (H >> s) - P, 0 <= col <= (W >> s) - P, which
 *              also says that level s of THAT image holds a patch.  The kernel does not report a sample or level outside that range (the
 *              caller checks on the host); it clamps both for addressing, so the reads stay inside the image even then
 *   scale_ids  int32 [total] in [0, num_scales), or NULL (all level 0; num_scales must then be 1)
 *   flips      int32 [NI][2] = (hflip, vflip), or NULL
 *   mean, std  HOST float[3]
 *   patches    fp32 [total][3][P][P];  pos fp32 [total][2] = clamp((sample + P/2) / (dim_s - P/2), 0, 1 - 1e-6), dim_s = dim >> s;
 *              scales fp32 [total] (the ids as floats) or NULL.  Exactly these extents are written, with plain stores
 *
 * Refused, with nothing launched: a NULL required pointer (everything but scale_ids, flips, scales); a tab that is not 16-byte aligned;
 * NI < 1; row0[0] != 0, a decreasing row0 or row0[NI] < 1; patch_size other than 16 | 8; num_scales outside 1 .. 4; scale_ids NULL with
 * num_scales > 1; an unknown dtype; an img_off[i] that is not a multiple of E; an image that leaves the buffer (img_off[i] < 0 or
 * img_off[i] + 3 H[i] W[i] E > image_bytes); an image smaller than one patch (H[i] < P or W[i] < P). */
int  vtq_k_gather_patches_planar(const void* images, int64_t image_bytes, int32_t dtype, const int32_t* tab, const int32_t* patch_img,
                                 const int64_t* img_off, const int32_t* H, const int32_t* W, const int32_t* row0, int32_t NI,
                                 const int32_t* samples, const int32_t* scale_ids, const int32_t* flips, const float* mean, const float* std_,
                                 float* patches, float* pos, float* scales, int32_t patch_size, int32_t num_scales, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTAMIQ_HIP_TENSORS_H */
