// The arithmetic of the two OCP FP6 formats (e3m2: bias 3, max 28; e2m3: bias 1, max 7.5; no inf,
// no NaN), shared by the row quantizer, the dequantizer and the decode GEMV of fp6.hip so that all
// of them form the same bits. Internal device header.
//
// Storage ("native", torchao/dtypes/floatx/floatx_tensor_core_layout.py): a row of K codes is a
// little-endian bit stream, code k at bits 6 k .. 6 k + 5 (00SEEEMM without the two zeros), so 32
// codes are 6 consecutive dwords: one operand of v_cvt_scalef32_pk32_bf16_{bf6,fp6}, which decodes
// them to 32 bf16 in one instruction. Every fp6 value is a bf16 number, so with scale 1.0 the
// decode is exact. Operand order (element i of the conversion = bits 6 i .. 6 i + 5 of the six
// dwords, result element i = half i & 1 of result dword i >> 1) is what experiments/
// probe_fp6_order.hip measures.
#pragma once

#include "tao_common.h"

namespace tao {

constexpr int kFp6Group = 32;        // codes per conversion operand
constexpr int kFp6GroupDwords = 6;   // dwords (24 B) per group

// Fmt: 0 = e3m2 (the hardware's "bf6"), 1 = e2m3 (its "fp6")
template <int FMT>
struct Fp6 {
  static constexpr int kM = FMT == 0 ? 2 : 3;          // mantissa bits
  static constexpr int kBias = FMT == 0 ? 3 : 1;       // exponent bias
  static constexpr float kMax = FMT == 0 ? 28.0f : 7.5f;
  static constexpr uint32_t kMaxCode = 0x1Fu;          // S = 0, E and M all ones
};

typedef uint32_t u32x6_t __attribute__((ext_vector_type(6)));
typedef __bf16 bf16x32_t __attribute__((ext_vector_type(32)));
typedef uint32_t u32x16_t __attribute__((ext_vector_type(16)));

// 32 codes (6 dwords) -> 16 bf16 pairs (k, k + 1), in the dword order x is loaded in
template <int FMT>
__device__ __forceinline__ void fp6_decode32(const uint32_t (&c)[6], uint32_t (&p)[16]) {
  const u32x6_t v = {c[0], c[1], c[2], c[3], c[4], c[5]};
  bf16x32_t r;
  if constexpr (FMT == 0) r = __builtin_amdgcn_cvt_scalef32_pk32_bf16_bf6(v, 1.0f);
  else r = __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(v, 1.0f);
  const u32x16_t d = __builtin_bit_cast(u32x16_t, r);
#pragma unroll
  for (int i = 0; i < 16; ++i) p[i] = d[i];
}

// s = float(bf16(max(amax, 1e-12) / max_normal)): the IEEE fp32 quotient rounded to bf16
template <int FMT>
__device__ __forceinline__ float fp6_row_scale(float amax) {
  return round_bf16(fmaxf(amax, 1e-12f) / Fp6<FMT>::kMax);
}

// One fp32 value -> its 6-bit code: round to nearest even, saturated at +-max_normal, subnormals
// kept, the sign of a zero kept. Integer arithmetic on the fp32 bits; a NaN takes the low five
// bits of what the normal branch makes of its bits (rows with inf or NaN are outside the format's
// contract, but a NaN's code never touches its neighbours').
template <int FMT>
__device__ __forceinline__ uint32_t fp6_encode(float f) {
  constexpr int M = Fp6<FMT>::kM, B = Fp6<FMT>::kBias;
  constexpr int SH = 23 - M;
  const uint32_t bits = __float_as_uint(f);
  const uint32_t sign = (bits >> 31) << 5;
  const uint32_t ab = bits & 0x7FFFFFFFu;
  const float a = __uint_as_float(ab);
  uint32_t code;
  if (a >= Fp6<FMT>::kMax) {
    code = Fp6<FMT>::kMaxCode;
  } else if (ab < ((uint32_t)(127 + 1 - B) << 23)) {
    // below the smallest normal 2^(1 - B): units of the subnormal step 2^(1 - B - M); rintf is
    // round-half-even and the product is exact; the result 2^M is the smallest normal's code
    code = (uint32_t)rintf(a * (float)(1 << (B - 1 + M)));
  } else {
    const uint32_t r = ab + ((1u << (SH - 1)) - 1u) + ((ab >> SH) & 1u);
    code = (r >> SH) - ((uint32_t)(127 - B) << M);
  }
  // a NaN's normal branch is wider than five bits: masked, so that it stays inside its own field
  return sign | (code & 0x1Fu);
}

// 32 codes -> the six dwords of their bit stream
__device__ __forceinline__ void fp6_pack32(const uint32_t (&c)[32], uint32_t (&o)[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) o[i] = 0u;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int bit = 6 * j, d = bit >> 5, sh = bit & 31;
    o[d] |= c[j] << sh;
    if (sh > 26) o[d + 1] |= c[j] >> (32 - sh);
  }
}

}  // namespace tao
