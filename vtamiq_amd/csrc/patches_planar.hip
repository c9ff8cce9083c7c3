// On-device image -> patch tensor for FLOAT images that are already resident (include/vtamiq_hip_tensors.h): NI images of different sizes,
// each three contiguous CHW planes of T = float | __half | __hip_bfloat16, packed in one buffer at per-image byte offsets; the patches of
// all of them in one launch, with no image-sized intermediate.  The contract is that of gather_patches_u8_kernel (patches_ragged.hip) with
// the pixel format changed: the output of another model is scored as it is, without a quantisation to 8 bits.
//
// Arithmetic, operation for operation (fp contract off, so no a * b + c fuses):
//   level 0     ((float)x - mean[c]) / std[c] of the FLIPPED image's pixel, a true division ((float) of a 16-bit T is exact)
//   level s     the nested 2 x 2 sums of level s - 1, in (0,0),(0,1),(1,0),(1,1) order then / 4, s times: level-s pixel (y, x) covers the
//               flipped level-0 pixels (y 2^s + dy, x 2^s + dx), dy, dx < 2^s -- flips apply before the pooling, so an odd dimension
//               loses the last row / column of the FLIPPED image
//   pos         clamp((sample + P/2) / (dim_s - P/2), 0, 1 - 1e-6), dim_s = dim >> s
// The u8 kernel's 3 x 256 table has no float counterpart: every level-0 value is normalised where it is read and pooled in registers.
//
// Reads of the image buffer are single-element loads of T.  An image's offset is a multiple of sizeof(T) and nothing more (a 17 x 33 fp16
// image is 3366 bytes: its successor is 2-byte aligned only), so a single element is the widest load that is aligned for every image, and
// nothing outside [img_off[i], img_off[i] + 3 H W sizeof(T)) is touched; the level is clamped to the image's last level that holds a patch
// and the sample into that level for ADDRESSING, so that holds for any sample and scale id.
//
// Thread (i, j) of the P x P workgroup forms output pixel (i, j) of the 3 channels from its 2^s x 2^s level-0 pixels; the nested order
// visits them as 2^s-element runs of a source row, so the 16 lanes of a patch row cover P 2^s contiguous elements of that row between
// them: every cache line a wave requests is used in full by that wave within 2^s consecutive loads (a wave of 64 lanes = 4 patch rows
// asks for 4 lines of 128 B per load at level 0 and 1 in fp32, 4 2^(s-1) at level s), and HBM sees each line once.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "dev_common.h"
#include "kernels.h"

namespace vtq {
namespace {

// exact: no a * b + c of the pooling sums may fuse
#pragma clang fp contract(off)

struct NormF {
    float m[3], s[3];
};

__device__ __forceinline__ float px_f32(float v) { return v; }
__device__ __forceinline__ float px_f32(__half v) { return __half2float(v); }
__device__ __forceinline__ float px_f32(__hip_bfloat16 v) { return __bfloat162float(v); }

// level-S pixel (y, x) of one channel plane of the flipped image
template <typename T, int S>
__device__ __forceinline__ float level_px(const T* __restrict__ plane, int H, int W, int hf, int vf, int y, int x, float mean, float sd) {
    if constexpr (S == 0) {
        const int ys = vf ? H - 1 - y : y, xs = hf ? W - 1 - x : x;
        return __fdiv_rn(px_f32(plane[(int64_t)ys * W + xs]) - mean, sd);
    } else {
        float sum = level_px<T, S - 1>(plane, H, W, hf, vf, 2 * y, 2 * x, mean, sd);
        sum += level_px<T, S - 1>(plane, H, W, hf, vf, 2 * y, 2 * x + 1, mean, sd);
        sum += level_px<T, S - 1>(plane, H, W, hf, vf, 2 * y + 1, 2 * x, mean, sd);
        sum += level_px<T, S - 1>(plane, H, W, hf, vf, 2 * y + 1, 2 * x + 1, mean, sd);
        return sum / 4.0f;
    }
}

template <typename T, int S>
__device__ __forceinline__ void patch_level(const T* __restrict__ img, int H, int W, int hf, int vf, int y, int x, const NormF& nf,
                                            float* __restrict__ dst, int PP) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
        dst[c * PP + threadIdx.x] = level_px<T, S>(img + (int64_t)c * H * W, H, W, hf, vf, y, x, nf.m[c], nf.s[c]);
}

// one workgroup per patch, P * P threads.  tab: int32 [NI][4] = (img_off low word, high word, H, W), img_off in BYTES; patch_img: int32 [total]
template <typename T>
__global__ __launch_bounds__(256) void gather_patches_planar_kernel(const uint8_t* __restrict__ images, const int* __restrict__ tab,
                                                                    const int* __restrict__ patch_img, const int* __restrict__ samples,
                                                                    const int* __restrict__ scale_ids, const int* __restrict__ flips,
                                                                    float* __restrict__ patches, float* __restrict__ pos,
                                                                    float* __restrict__ scales, NormF nf, int P, int num_scales) {
    const int64_t pn = blockIdx.x;
    const int ni = patch_img[pn];
    const int4 t = *reinterpret_cast<const int4*>(tab + (int64_t)ni * 4);
    const int64_t off = (int64_t)(((uint64_t)(uint32_t)t.y << 32) | (uint32_t)t.x);
    const int H = t.z, W = t.w;
    const int sc = scale_ids ? scale_ids[pn] : 0;
    int lvl = min(max(sc, 0), num_scales - 1);                       // addressing only: a valid id on a level that holds a patch is unchanged
    while (lvl > 0 && ((H >> lvl) < P || (W >> lvl) < P)) --lvl;     // (level 0 holds one: checked by the entry)
    const int h = H >> lvl, w = W >> lvl;
    const int row = samples[pn * 2], col = samples[pn * 2 + 1];
    const int hf = flips ? flips[ni * 2] : 0, vf = flips ? flips[ni * 2 + 1] : 0;
    const int PP = P * P, i = threadIdx.x / P, j = threadIdx.x - i * P;
    const T* img = reinterpret_cast<const T*>(images + off);         // off is a multiple of sizeof(T): checked by the entry
    float* dst = patches + pn * 3 * PP;
    const int y = min(max(row, 0), h - P) + i, x = min(max(col, 0), w - P) + j;       // clamped for addressing only
    switch (lvl) {
        case 0: patch_level<T, 0>(img, H, W, hf, vf, y, x, nf, dst, PP); break;
        case 1: patch_level<T, 1>(img, H, W, hf, vf, y, x, nf, dst, PP); break;
        case 2: patch_level<T, 2>(img, H, W, hf, vf, y, x, nf, dst, PP); break;
        default: patch_level<T, 3>(img, H, W, hf, vf, y, x, nf, dst, PP); break;
    }
    if (threadIdx.x < 2) {
        const float half = (float)(P / 2);                           // data/patch_sampling.py:565-568
        const float smp = (float)(threadIdx.x == 0 ? row : col) + half;
        const float den = (float)(threadIdx.x == 0 ? h : w) - half;
        pos[pn * 2 + threadIdx.x] = fminf(fmaxf(smp / den, 0.0f), (float)(1.0 - 1e-6));
    }
    if (scales && threadIdx.x == 2) scales[pn] = (float)sc;
}

}  // namespace

hipError_t launch_gather_patches_planar(const void* images, int dtype, const int* tab, const int* patch_img, const int* samples,
                                        const int* scale_ids, const int* flips, float* patches, float* pos, float* scales, int64_t total,
                                        const float* mean, const float* sd, int P, int num_scales, hipStream_t s) {
    if (total < 1 || total > 0x7fffffff || (P != 16 && P != 8) || num_scales < 1 || num_scales > 4 || dtype < 0 || dtype > 2)
        return hipErrorInvalidValue;
    NormF nf;
    for (int c = 0; c < 3; ++c) { nf.m[c] = mean[c]; nf.s[c] = sd[c]; }
    const uint8_t* img = static_cast<const uint8_t*>(images);
    const dim3 grid((unsigned)total), block(P * P);
    if (dtype == 0)
        hipLaunchKernelGGL(gather_patches_planar_kernel<float>, grid, block, 0, s, img, tab, patch_img, samples, scale_ids, flips, patches, pos,
                           scales, nf, P, num_scales);
    else if (dtype == 1)
        hipLaunchKernelGGL(gather_patches_planar_kernel<__half>, grid, block, 0, s, img, tab, patch_img, samples, scale_ids, flips, patches, pos,
                           scales, nf, P, num_scales);
    else
        hipLaunchKernelGGL(gather_patches_planar_kernel<__hip_bfloat16>, grid, block, 0, s, img, tab, patch_img, samples, scale_ids, flips,
                           patches, pos, scales, nf, P, num_scales);
    return hipGetLastError();
}

}  // namespace vtq
