// Per-row symmetric quantisation arithmetic of the W4A8 linear (w4a8.hip), shared by the per-token
// quantizer, the per-row weight quantizer and the one-token prologue of the W4A8 GEMV, so that all
// of them produce the same bytes. Internal device header.
//   s = max(fp32(bf16(amax / H)), 2^-23),  r = 1 / s (fp32, IEEE),
//   q = clamp(rint(fp32(x) * r), lo, hi)
// with H = 127.5, [lo, hi] = [-128, 127] for the int8 activation (_int8_symm_cutlass_quant,
// torchao/quantization/quant_api.py:1299-1308) and H = 7.5, [-8, 7] for the int4 weight
// (_int4_symm_cutlass_quant, :1311-1323): choose_qparams_affine divides the bf16 amax by
// (quant_max - quant_min) / 2 in the input's dtype, clamps at eps = finfo(float32).eps = 2^-23 (a
// bf16 number) and widens to scale_dtype = float32; quantize_affine multiplies the bf16 input by
// the fp32 reciprocal, so the product is fp32 (quant_primitives.py:1548-1565, 449-453).
#pragma once

#include "tao_common.h"

namespace tao {

constexpr float kW4A8ActHalf = 127.5f, kW4A8WgtHalf = 7.5f;

__device__ __forceinline__ float cutlass_row_scale(float amax, float half_range) {
  const float s = round_bf16(amax / half_range);
  return s < 1.1920928955078125e-07f ? 1.1920928955078125e-07f : s;
}

// q = clamp(rint(x * r), LO, HI) of one value, as an integer
template <int LO, int HI>
__device__ __forceinline__ int cutlass_code(float xv, float r) {
  float t = rintf(xv * r);
  t = fminf(fmaxf(t, (float)LO), (float)HI);
  return (int)t;
}

// the 8 bf16 of one 16-B piece -> 8 int8 codes in element order
__device__ __forceinline__ uint2 w4a8_quant8(const uint4 v, float r) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t packed[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xv = (j & 1) ? bf16hi_to_f32(d[j >> 1]) : bf16lo_to_f32(d[j >> 1]);
    packed[j >> 2] |= ((uint32_t)cutlass_code<-128, 127>(xv, r) & 0xFFu) << (8 * (j & 3));
  }
  return make_uint2(packed[0], packed[1]);
}

// the same codes de-interleaved: .x = elements 0, 2, 4, 6, .y = elements 1, 3, 5, 7: the order
// in which the nibble expansion of w4a8.hip meets them (even elements in the low nibbles)
__device__ __forceinline__ uint2 w4a8_quant8_eo(const uint4 v, float r) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t packed[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xv = (j & 1) ? bf16hi_to_f32(d[j >> 1]) : bf16lo_to_f32(d[j >> 1]);
    packed[j & 1] |= ((uint32_t)cutlass_code<-128, 127>(xv, r) & 0xFFu) << (8 * (j >> 1));
  }
  return make_uint2(packed[0], packed[1]);
}

// the 8 bf16 of one 16-B piece -> 8 int4 codes in 4 bytes: element 2 j in the low nibble of byte
// j, element 2 j + 1 in the high nibble, two's complement (CutlassInt4PackedLayout's from_plain,
// torchao/dtypes/uintx/cutlass_int4_packed_layout.py:131-144)
__device__ __forceinline__ uint32_t w4a8_quant8_nib(const uint4 v, float r) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t packed = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xv = (j & 1) ? bf16hi_to_f32(d[j >> 1]) : bf16lo_to_f32(d[j >> 1]);
    packed |= ((uint32_t)cutlass_code<-8, 7>(xv, r) & 0xFu) << (4 * j);
  }
  return packed;
}

}  // namespace tao
