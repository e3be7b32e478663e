// Per-row e4m3fn quantisation arithmetic, shared by the row quantizer (fp8_quantize.hip) and the
// one-token prologues of the float8 dynamic-activation GEMVs (scaled_gemv.h with row scales,
// fp8dq_decode_kernel in fp8_dyn.hip) so that all produce the
// same bytes. Internal device header. The formulas are fp8_quantize.hip's header comment.
#pragma once

#include "fp8_convert.h"
#include "tao_common.h"

namespace tao {

// max(m, |v|) over the 8 bf16 of one 16-B piece
__device__ __forceinline__ float fp8_amax8(const uint4 v, float m) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    m = fmaxf(m, fmaxf(fabsf(bf16lo_to_f32(d[j])), fabsf(bf16hi_to_f32(d[j]))));
  return m;
}

// s = float(bf16(amax / 448)): a true fp32 division, rounded to bf16, kept in fp32
__device__ __forceinline__ float fp8_row_scale(float amax) { return round_bf16(amax / 448.0f); }

// q = e4m3fn_rne(clamp(float(x) / s, -448, 448)) for the 8 bf16 of one 16-B piece -> 8 codes
__device__ __forceinline__ uint2 fp8_quant8(const uint4 v, float s) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t o[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = (j & 1) ? bf16hi_to_f32(d[j >> 1]) : bf16lo_to_f32(d[j >> 1]);
    o[j >> 2] |= (uint32_t)f32_to_e4m3fn_rne(clamp_e4m3fn(x / s)) << (8 * (j & 3));
  }
  return make_uint2(o[0], o[1]);
}

}  // namespace tao
