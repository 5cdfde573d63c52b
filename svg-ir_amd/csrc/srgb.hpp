// svg-ir_amd/csrc/srgb.hpp -- `rgb_to_srgb` (utils/graphics_utils.py:198-215) and the NaN-propagating clamps of the image-space kernels:
// the epilogue right after the rasterizer (csrc/epilogue.hip) and the eval view's environment backdrop (csrc/backdrop.hip).
#pragma once
#include "common.hpp"

namespace svgir {

#if defined(__HIPCC__)
// torch.clamp / clamp_min propagate NaN (fminf / fmaxf return the other operand): a NaN plane or opacity stays NaN in every result
// it reaches, as in the reference, instead of turning into a valid-looking pixel.  Plain compares: false on NaN, so x passes through.
__device__ __forceinline__ float clamp_min_nan(float x, float lo) { return x < lo ? lo : x; }
__device__ __forceinline__ float clamp01_nan(float y) { return y < 0.f ? 0.f : (y > 1.f ? 1.f : y); }

__device__ __forceinline__ float srgb(float x) {
    const float y = x > 0.0031308f ? powf(x, 1.0f / 2.4f) * 1.055f - 0.055f : 12.92f * x;   // (NaN takes the linear branch: NaN)
    return clamp01_nan(y);
}
// d srgb / dx: 0 where the final clip to [0,1] is active -- and for a NaN argument, as torch.clamp's backward (its mask
// min <= y <= max is false): the gradients of a NaN pixel stay confined to that pixel either way, the kernel being per-pixel
__device__ __forceinline__ float dsrgb(float x) {
    const float y = x > 0.0031308f ? powf(x, 1.0f / 2.4f) * 1.055f - 0.055f : 12.92f * x;
    if (!(y >= 0.f && y <= 1.f)) return 0.f;
    return x > 0.0031308f ? (1.055f / 2.4f) * powf(x, 1.0f / 2.4f - 1.0f) : 12.92f;
}

// `srgb_to_rgb` (utils/graphics_utils.py:218-229): x <= 0.04045 ? x / 12.92 : pow((max(x, 0.04045) + 0.055) / 1.055, 2.4), every
// operation rounded on its own in fp32.  On the pow side of the compare max(x, 0.04045) is x itself.  NaN: `<=` is false, torch.where
// takes the pow branch, whose max and pow propagate it: NaN.  No clip: the reference has none here.
__device__ __forceinline__ float srgb_to_rgb(float x) {
#pragma clang fp contract(off)
    if (x <= 0.04045f) return __fdiv_rn(x, 12.92f);
    return powf(__fdiv_rn(x + 0.055f, 1.055f), 2.4f);
}
#endif

}  // namespace svgir
