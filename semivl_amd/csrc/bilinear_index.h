// Bilinear source index of every kernel that resizes: ATen's upsample_bilinear2d index math (area_pixel_compute_scale,
// area_pixel_compute_source_index + guard_index_and_lambda), which is what F.interpolate / mmseg.ops.resize call in the
// reference.  ONE definition: the resize kernels (resample.hip), the evaluator's views (tta.hip), the MaskCLIP label tail
// (pixel_loss.hip) and the resize-fused losses (pixel_loss_up.hip, host and device) form the same taps and weights, which is
// what makes the fused and the unfused loss paths of a step agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

__host__ __device__ inline float area_scale(int in, int out, bool align) {
  if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  return (float)in / (float)out;
}
// taps i0 <= i1 (clamped to the last source index) and their weights l0 + l1 = 1 of destination index `dst`
__host__ __device__ inline void src_index(int dst, float scale, int in_size, bool align, int& i0, int& i1, float& l0,
                                          float& l1) {
  float s = align ? scale * dst : scale * (dst + 0.5f) - 0.5f;
  if (!align && s < 0.f) s = 0.f;
  i0 = (int)s < in_size - 1 ? (int)s : in_size - 1;
  i1 = i0 + 1 < in_size - 1 ? i0 + 1 : in_size - 1;
  l1 = fminf(fmaxf(s - i0, 0.f), 1.f);
  l0 = 1.f - l1;
}
