// Per-token symmetric int8 quantisation arithmetic in bf16, shared by the per-token quantizer and
// the one-token prologue of the int8 dynamic-activation GEMV (int8_dyn.hip) and by the quantized
// KV-cache write (kv_q8.hip), so that all of them produce the same bytes. Internal device header.
//   s = max(bf16(amax / 127), bf16(1e-5)),  r = bf16(1 / s),
//   q = clamp(rint(bf16(x * r)), -127, 127)
// (choose_qparams_affine + quantize_affine with every step in the input's dtype:
// quant_primitives.py:1548-1554, 449-453; the KV cache reaches them through
// _quantize_activation_per_token_absmax, quantization/utils.py:152-182).
#pragma once

#include "tao_common.h"

namespace tao {

// per-token scale from amax; its reciprocal is round_bf16(1.f / token_scale(amax))
__device__ __forceinline__ float token_scale(float amax) {
  float s = round_bf16(amax / 127.f);
  const float eps = round_bf16(1e-5f);
  return s < eps ? eps : s;
}

// The same scale with the clamp choose_qparams_affine applies when its caller passes no eps:
// torch.finfo(bfloat16).eps = 2^-7 (quant_primitives.py:1526-1527, 1565). SmoothQuant's
// _ActQuantizer.dynamic_quantize (prototype/smoothquant/api.py:138-145) is such a caller, so an
// all-zero or tiny token gets the scale 0.0078125 there, not bf16(1e-5).
__device__ __forceinline__ float token_scale_default_eps(float amax) {
  const float s = round_bf16(amax / 127.f);
  return s < 0.0078125f ? 0.0078125f : s;
}

// q = clamp(round(bf16(x * r)), -127, 127) of one value, as the low byte of the result
__device__ __forceinline__ uint32_t quant1(float xv, float r) {
  float t = rintf(round_bf16(xv * r));
  t = fminf(fmaxf(t, -127.f), 127.f);
  return (uint32_t)(int32_t)t & 0xFFu;
}

// the same for the 8 bf16 of one 16-B piece -> 8 int8 bytes
__device__ __forceinline__ uint2 quant8(const uint4 v, float r) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t packed[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xv = (j & 1) ? bf16hi_to_f32(d[j >> 1]) : bf16lo_to_f32(d[j >> 1]);
    packed[j >> 2] |= quant1(xv, r) << (8 * (j & 3));
  }
  return make_uint2(packed[0], packed[1]);
}

__device__ __forceinline__ float bf16_abs_max2(uint32_t d, float m) {
  m = fmaxf(m, fabsf(bf16lo_to_f32(d)));
  return fmaxf(m, fabsf(bf16hi_to_f32(d)));
}

}  // namespace tao
