// Block arithmetic shared by the MX kernels (mx_fp8.hip, mx_fp4.hip): the amax of a 16-B piece on
// the bf16 magnitude patterns, the e4m3fn block scale byte and divisor of the quantizer (the row
// quantizer and both one-token prologues, so that they produce the same bytes), and the block
// scale applied to a partial sum. Internal device header; the formulas are mx_fp8.hip's header
// comment.
#pragma once

#include "tao_common.h"

namespace tao {

// max(m, |.|) over the 8 bf16 of one 16-B piece, on the 15-bit magnitude patterns
__device__ __forceinline__ uint32_t mx_amax8(const uint4 v, uint32_t m) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t a = d[j] & 0x7FFF7FFFu;
    const uint32_t lo = a & 0xFFFFu, hi = a >> 16;
    m = m > lo ? m : lo;
    m = m > hi ? m : hi;
  }
  return m;
}
// the block's E8M0 byte from its amax pattern: exponent field - 8, floored at 0; NaN -> 255
__device__ __forceinline__ uint32_t mx_scale_byte(uint32_t amax15) {
  const uint32_t e = amax15 >> 7;
  return amax15 > 0x7F80u ? 255u : (e > 8u ? e - 8u : 0u);
}
// the fp32 number with that exponent field, at least 2^-126 (byte 255: +inf)
__device__ __forceinline__ float mx_divisor(uint32_t byte) {
  return __builtin_bit_cast(float, (byte > 1u ? byte : 1u) << 23);
}

// d * 2^(xb - 127) * 2^(wb - 127); a byte 255 is NaN
__device__ __forceinline__ float mx_scaled(float d, uint32_t xb, uint32_t wb) {
  const float v = ldexpf(d, (int)(xb + wb) - 254);
  return (xb == 255u || wb == 255u) ? __builtin_nanf("") : v;
}

}  // namespace tao
