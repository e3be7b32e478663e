// Block arithmetic of the blockwise float8 quantizers (block_fp8.hip): the scale of a block from
// its amax and the e4m3fn codes of a 16-B piece under that scale. Shared by the activation
// quantizer, the weight quantizer and the one-token prologue of the GEMV so that all three produce
// the same bytes. Internal device header; the formulas are block_fp8.hip's header comment.
#pragma once

#include "fp8_quant_row.h"

namespace tao {

// s = amax / 448: a correctly rounded fp32 division, subnormal results kept. The amax itself is
// fp8_amax8's (fp8_quant_row.h): fmaxf over |x|, so a NaN element is ignored.
__device__ __forceinline__ float blockfp8_scale(float amax) { return amax / 448.0f; }

// code = e4m3fn_rne(x / s) for the 8 bf16 of one 16-B piece; where s == 0 (an all-zero block, or
// one with NaN only) the element itself is encoded: a signed zero stays, a NaN stays NaN. No clamp:
// |x| <= amax, so |x / s| passes 448 by division rounding only, and the rounding takes that to 448.
__device__ __forceinline__ uint2 blockfp8_quant8(const uint4 v, float s) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t o[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = (j & 1) ? bf16hi_to_f32(d[j >> 1]) : bf16lo_to_f32(d[j >> 1]);
    const float q = s == 0.0f ? x : x / s;
    o[j >> 2] |= (uint32_t)f32_to_e4m3fn_rne(q) << (8 * (j & 3));
  }
  return make_uint2(o[0], o[1]);
}

// max over the 16 lanes that share a block (lanes 16 i .. 16 i + 15 of a wave)
__device__ __forceinline__ float blockfp8_amax16(float m) {
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));
  return m;
}

}  // namespace tao
