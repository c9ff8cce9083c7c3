// On-device image -> patch tensor for images of DIFFERENT sizes (include/vtamiq_hip_images.h): NI uint8 HWC images packed back to back
// in one byte buffer, the patches of all of them in one launch, and no image-sized intermediate -- a patch reads the uint8 pixels it
// is made of and normalises and pools them in registers, where patches.hip writes a normalised fp32 copy of every image and its whole
// AvgPool pyramid first and gathers from those.
//
// Bit contract: every output element has the bits patches.hip gives for that image alone, so the arithmetic is its arithmetic,
// operation for operation:
//   level 0     (__fdiv_rn((float)u8, 255) - mean[c]) / std[c] of the FLIPPED image's pixel (image_normalize_kernel)
//   level s     the nested 2 x 2 sums of level s - 1, in (0,0),(0,1),(1,0),(1,1) order then / 4 (avgpool2_kernel), s times: level-s
//               pixel (y, x) covers the flipped level-0 pixels (y 2^s + dy, x 2^s + dx), dy, dx < 2^s -- flips apply before the
//               pooling, so an odd dimension loses the last row / column of the FLIPPED image
//   pos         clamp((sample + P/2) / (dim_s - P/2), 0, 1 - 1e-6), dim_s = dim >> s (gather_patches_kernel)
// The normalisation of a level >= 1 patch goes through a 3 x 256 table in LDS, filled once per workgroup with the same three
// operations on the 256 possible bytes: the same bits without 4^s divisions per output element.
//
// Reads of the image buffer are byte loads (an image starts at any byte: a 17 x 33 image is 1683 bytes long), so nothing outside
// [img_off[i], img_off[i] + 3 H W) is touched; the level is clamped to the image's last level that holds a patch and the sample into that
// level for ADDRESSING, so that holds for any sample and scale id (the outputs of an out-of-range sample are then not the reference's
// IndexError: the Python layer raises that on the host).
// Thread (i, j) of the P x P workgroup forms output pixel (i, j) of the 3 channels: the 16 threads of a patch row read 48 * 2^s
// contiguous bytes of each of the 2^s source rows.
#include "dev_common.h"
#include "kernels.h"

namespace vtq {
namespace {

// exact: no a * b + c of the pooling sums may fuse (the sums of patches.hip are separate kernels' stores)
#pragma clang fp contract(off)

struct NormU8 {
    float m[3], s[3];
};

__device__ __forceinline__ float norm_u8(uint8_t v, float mean, float sd) { return (__fdiv_rn((float)v, 255.0f) - mean) / sd; }

// level-S pixel (y, x) of channel c of the flipped image; S == 0 normalises directly, S >= 1 reads lut[c * 256 + byte]
template <int S, bool LUT>
__device__ __forceinline__ float level_px(const uint8_t* __restrict__ img, int H, int W, int hf, int vf, int y, int x, int c,
                                          const float* lut, float mean, float sd) {
    if constexpr (S == 0) {
        const int ys = vf ? H - 1 - y : y, xs = hf ? W - 1 - x : x;
        const uint8_t v = img[((int64_t)ys * W + xs) * 3 + c];
        if constexpr (LUT) return lut[c * 256 + v];
        else return norm_u8(v, mean, sd);
    } else {
        float sum = level_px<S - 1, LUT>(img, H, W, hf, vf, 2 * y, 2 * x, c, lut, mean, sd);
        sum += level_px<S - 1, LUT>(img, H, W, hf, vf, 2 * y, 2 * x + 1, c, lut, mean, sd);
        sum += level_px<S - 1, LUT>(img, H, W, hf, vf, 2 * y + 1, 2 * x, c, lut, mean, sd);
        sum += level_px<S - 1, LUT>(img, H, W, hf, vf, 2 * y + 1, 2 * x + 1, c, lut, mean, sd);
        return sum / 4.0f;
    }
}

template <int S>
__device__ __forceinline__ void patch_level(const uint8_t* __restrict__ img, int H, int W, int hf, int vf, int row, int col, int i, int j,
                                            const float* lut, const NormU8& nu, float* __restrict__ dst, int PP) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * PP + threadIdx.x] = level_px<S, (S > 0)>(img, H, W, hf, vf, row + i, col + j, c, lut, nu.m[c], nu.s[c]);
}

// one workgroup per patch, P * P threads.  tab: int32 [NI][4] = (img_off low word, high word, H, W); patch_img: int32 [total]
__global__ __launch_bounds__(256) void gather_patches_u8_kernel(const uint8_t* __restrict__ images, const int* __restrict__ tab,
                                                                const int* __restrict__ patch_img, const int* __restrict__ samples,
                                                                const int* __restrict__ scale_ids, const int* __restrict__ flips,
                                                                float* __restrict__ patches, float* __restrict__ pos,
                                                                float* __restrict__ scales, NormU8 nu, int P, int num_scales) {
    __shared__ float lut[3 * 256];
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
    if (lvl > 0) {                                                    // uniform per workgroup
        for (int e = threadIdx.x; e < 3 * 256; e += PP) {
            const int c = e >> 8;
            const float mean = c == 0 ? nu.m[0] : (c == 1 ? nu.m[1] : nu.m[2]), sd = c == 0 ? nu.s[0] : (c == 1 ? nu.s[1] : nu.s[2]);
            lut[e] = norm_u8((uint8_t)(e & 255), mean, sd);
        }
        __syncthreads();
    }
    const uint8_t* img = images + off;
    float* dst = patches + pn * 3 * PP;
    const int ra = min(max(row, 0), h - P), ca = min(max(col, 0), w - P);       // addressing only
    switch (lvl) {
        case 0: patch_level<0>(img, H, W, hf, vf, ra, ca, i, j, nullptr, nu, dst, PP); break;
        case 1: patch_level<1>(img, H, W, hf, vf, ra, ca, i, j, lut, nu, dst, PP); break;
        case 2: patch_level<2>(img, H, W, hf, vf, ra, ca, i, j, lut, nu, dst, PP); break;
        default: patch_level<3>(img, H, W, hf, vf, ra, ca, i, j, lut, nu, dst, PP); break;
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

hipError_t launch_gather_patches_u8(const uint8_t* images, const int* tab, const int* patch_img, const int* samples, const int* scale_ids,
                                    const int* flips, float* patches, float* pos, float* scales, int64_t total, const float* mean,
                                    const float* sd, int P, int num_scales, hipStream_t s) {
    if (total < 1 || total > 0x7fffffff || (P != 16 && P != 8) || num_scales < 1 || num_scales > 4) return hipErrorInvalidValue;
    NormU8 nu;
    for (int c = 0; c < 3; ++c) { nu.m[c] = mean[c]; nu.s[c] = sd[c]; }
    hipLaunchKernelGGL(gather_patches_u8_kernel, dim3((unsigned)total), dim3(P * P), 0, s, images, tab, patch_img, samples, scale_ids, flips,
                       patches, pos, scales, nu, P, num_scales);
    return hipGetLastError();
}

}  // namespace vtq
