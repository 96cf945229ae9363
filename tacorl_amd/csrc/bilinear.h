// The bilinear sampling rule of torchvision.transforms.Resize on a float tensor, stated once for the kernels that resize uint8
// frames: the first stage of the augmenting pack (data_ops.hip pack_u8_aug_kernel) and the store-time resize
// (frame_ops.hip).  torch.nn.functional.interpolate(mode="bilinear", align_corners=False), no antialias = ATen's
// upsample_bilinear2d:
//   src = max(scale * (dst + 0.5) - 0.5, 0), scale = in / out (fp32); i0 = floor(src), i1 = i0 + (i0 < in - 1);
//   l1 = src - i0, l0 = 1 - l1;  out = h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11)
// Every operation is a separate fp32 rounding (the library is built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void bilinear_axis(int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
  const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

// the four-term sum on the 0..255 values of one channel
__device__ __forceinline__ float bilinear_mix(float h0, float h1, float w0, float w1, unsigned char p00, unsigned char p01,
                                              unsigned char p10, unsigned char p11) {
  return h0 * (w0 * (float)p00 + w1 * (float)p01) + h1 * (w0 * (float)p10 + w1 * (float)p11);
}
