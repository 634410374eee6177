// Device expressions of the HDR viewing chain, shared by reni_tu_image.hip (reni_unnormalise_srgb writes the mapped images) and
// reni_tu_metrics.hip (reni_pair_stats / reni_ssim map in registers): one spelling, so both units see the same numbers.
//
// Reference:
//   UnMinMaxNormlise   src/utils/custom_transforms.py:14-21   y = exp(0.5 (x + 1)(m1 - m0) + m0)
//   sRGB               src/utils/utils.py:30-42               x / q_b -> clamp [0,1] -> sRGB transfer curve
//
// Pinned semantics: NaN propagates as in torch (torch.clamp keeps a NaN; fminf / fmaxf would return the other operand and
// turn it into black), so a NaN pixel, a NaN exposure and 0 / 0 under an exposure q == 0 all come out NaN; a lit pixel
// under q == 0 is +inf before the clamp and 1 after it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace reni {

// 0.5 * (img + 1) * (m1 - m0) + m0, rounded after every operation as the reference's tensor ops are; range = (float)(m1 - m0)
__device__ __forceinline__ float img_unnormalise(float x, float range, float m0) {
  return expf(__fadd_rn(__fmul_rn(__fmul_rn(0.5f, __fadd_rn(x, 1.f)), range), m0));
}

// linear radiance under exposure q (the image's nested 0.98-quantile): divide, clamp, sRGB transfer curve (utils.py:35-41)
__device__ __forceinline__ float img_srgb(float lin, float q) {
  float x = lin / q;
  x = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);  // torch.clamp(x, 0, 1): both comparisons are false for a NaN, which stays
  return (x <= 0.0031308f) ? 12.92f * x : 1.055f * powf(fabsf(x), 1.f / 2.4f) - 0.055f;
}

}  // namespace reni
