// fp32 -> OCP e4m3fn (torch.float8_e4m3fn) in plain integer C++, for the weight quantizer.
// Internal header; host- and device-compilable so the rounding can be checked on the CPU.
//
// e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; S.1111.111 is NaN; the
// largest finite value is 448 (0x7E); subnormals are m * 2^-9 (m = 1..7); smallest normal 2^-6.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TAO_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define TAO_HD inline
#endif

namespace tao {

// Round-to-nearest-even encoding of v, which the caller has clamped to [-448, 448] (NaN passes
// through the clamp and encodes as NaN, sign kept). Matches tensor.to(torch.float8_e4m3fn).
TAO_HD uint8_t f32_to_e4m3fn_rne(float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  const uint32_t sign = (b >> 24) & 0x80u;
  const uint32_t a = b & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return (uint8_t)(sign | 0x7Fu);  // NaN
  if (a >= 0x3C800000u) {                               // |v| >= 2^-6: a normal e4m3 number
    // keep 3 mantissa bits: add half an ulp (ties to even), drop 20 bits, rebias 127 -> 7
    const uint32_t r = (a + 0x7FFFFu + ((a >> 20) & 1u)) >> 20;
    return (uint8_t)(sign | (r - (120u << 3)));
  }
  // below the smallest normal: a multiple of 2^-9, 0..8 after rounding (8 is the code of 2^-6)
  float av;
  __builtin_memcpy(&av, &a, 4);
  return (uint8_t)(sign | (uint32_t)rintf(av * 512.0f));
}

// clamp(v, -448, 448) that keeps NaN (torch.clamp's behaviour; fminf / fmaxf would drop it)
TAO_HD float clamp_e4m3fn(float v) {
  return v != v ? v : (v < -448.0f ? -448.0f : (v > 448.0f ? 448.0f : v));
}

}  // namespace tao
