// Block arithmetic shared by the MX kernels (mx_fp8.hip, mx_fp4.hip): the amax of a 16-B piece on
// the bf16 magnitude patterns, the e4m3fn block scale byte and divisor of the quantizer (the row
// quantizer and both one-token prologues, so that they produce the same bytes), the block scale
// applied to a partial sum, the part of the decode GEMV's policy that the two formats share
// (MxScales), and the entries' common size check. Internal header; the formulas are mx_fp8.hip's
// header comment.
#pragma once

#include "scaled_gemv.h"

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

// What the two MX policies of scaled_gemv_kernel share: E8M0 bytes per 32-k block on both
// operands, the one-token prologue's e4m3fn block quantizer (the row quantizer's arithmetic; four
// consecutive threads hold one block), and the block scale applied to a chunk's partial sum with
// one v_ldexp_f32 (exact short of fp32 overflow / underflow, so scaling the parts of a block apart
// equals scaling their sum).
struct MxScales {
  using Args = ScaledGemvArgs<uint8_t>;  // xs [M][K/32], ws [N][K/32]
  using Scale = uint32_t;
  static constexpr bool kRowScales = false;
  static constexpr int kBlockShift = 5;
  static __device__ __forceinline__ size_t scale_row(size_t nn) { return nn; }
  static __device__ __forceinline__ uint32_t token_scale(const uint4 xv) {
    uint32_t m = mx_amax8(xv, 0u);
    uint32_t o = (uint32_t)__shfl_xor((int)m, 1);
    m = m > o ? m : o;
    o = (uint32_t)__shfl_xor((int)m, 2);
    m = m > o ? m : o;
    return mx_scale_byte(m);
  }
  static __device__ __forceinline__ uint2 token_codes(const uint4 xv, uint32_t byte) {
    return fp8_quant8(xv, mx_divisor(byte));
  }
  static __device__ __forceinline__ float add(float d, uint32_t xb, uint32_t wb, float acc) {
    return acc + mx_scaled(d, xb, wb);
  }
};

// the size checks common to every MX entry; `what` prefixes the messages
static inline int check_mx_sizes(const char* what, int64_t M, int64_t N, int64_t K) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "%s: negative size", what);
  TAO_CHECK_ARG(K % 32 == 0, "%s: K (%lld) must be a multiple of 32 (the MX block size)", what,
                (long long)K);
  return TAO_OK;
}

}  // namespace tao
