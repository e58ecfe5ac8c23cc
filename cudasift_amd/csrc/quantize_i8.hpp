// quantize_i8.hpp — the 8-bit descriptor rule of misift_quantize_batch, for host and device.
//
//   q = (int8) clamp(rint(256 * d), 0, 127),   NaN -> 0, +inf -> 127, negatives -> 0
//
// 256 * d is exact (a power-of-two scale; it can only overflow to inf, which saturates), and rint rounds half to even, as
// the default fp32 rounding mode does on host and device.  SIFT descriptor elements stay below the 0.2 clip of the
// normalisation step by a margin (0.431 on the project's golden stereo pair), so 127 / 256 = 0.496 does not saturate.
// The same function backs the device kernel (kernels_match_i8.hip) and the host test hook misift_test_quantize, so the
// code a CPU test pins is the code the kernel runs.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QUANT_I8_HD __host__ __device__ __forceinline__
#else
#define QUANT_I8_HD inline
#endif

QUANT_I8_HD int8_t quantize_i8(float d)
{
  const float v = rintf(256.0f * d);
  if (!(v > 0.0f)) return 0;                      // NaN, -0, 0 and negatives
  return v >= 127.0f ? (int8_t)127 : (int8_t)(int)v;
}
