// The per-block arithmetic of the NF4 (QLoRA) format, shared by the quantizer, the dequantizer and
// the decode GEMV of nf4.hip so that all of them form the same bits. Internal device header.
//
// A block is 64 consecutive weights of the flattened tensor; block b has
//   s[b] = bf16( bf16( float(q[b]) / float(qf[b / 256]) ) + mean )
// (q the int8 double-quantized scaler, qf the bf16 factor of its group of 256, mean bf16: the
// reference's dequantize_scalers, every torch op rounded to bf16 once), and a weight is
//   w^ = bf16( level[code] * s[b] )
// with the 16 bf16 levels read from the tensor's own table, never from a compiled-in one.
// Packed codes: byte j holds element 2j in its HIGH nibble and element 2j + 1 in its low one.
#pragma once

#include "tao_common.h"

namespace tao {

constexpr int kNf4Block = 64;         // weights per block (one int8 scaler)
constexpr int kNf4ScalerBlock = 256;  // blocks per quantization factor

// s[b], as float. The division is the IEEE fp32 quotient, as torch's.
__device__ __forceinline__ float nf4_block_scaler(const int8_t* __restrict__ qs,
                                                  const uint16_t* __restrict__ qf, float mean,
                                                  int64_t b) {
  const float d = round_bf16((float)qs[b] / bf16_to_f32(qf[b >> 8]));
  return round_bf16(d + mean);
}

// The level table of one block, pre-multiplied: t[j] = bf16(level[j] * s), split into the low
// and the high bytes of the 16 results so that a 4-bit code indexes bytes:
//   lo[0..1] / hi[0..1] levels 0 - 7, lo[2..3] / hi[2..3] levels 8 - 15 (one byte per level).
struct Nf4Table {
  uint32_t lo[4], hi[4];
};

// lv: the 16 levels as 8 bf16 pairs (pair i = levels 2i, 2i + 1); s == 1.0f gives the bare levels
__device__ __forceinline__ Nf4Table nf4_scaled_table(const uint32_t (&lv)[8], float s) {
  uint32_t p[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    p[i] = (uint32_t)f32_to_bf16(bf16lo_to_f32(lv[i]) * s) |
           ((uint32_t)f32_to_bf16(bf16hi_to_f32(lv[i]) * s) << 16);
  Nf4Table t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // pairs 2i, 2i + 1 = levels 4i .. 4i + 3: bytes 0, 2 are the low bytes, 1, 3 the high ones
    t.lo[i] = __builtin_amdgcn_perm(p[2 * i + 1], p[2 * i], 0x06040200u);
    t.hi[i] = __builtin_amdgcn_perm(p[2 * i + 1], p[2 * i], 0x07050301u);
  }
  return t;
}

// Four codes (one per byte of c, each 0 .. 15) -> their table entries as two bf16 pairs:
// p01 = (t[c0], t[c1]), p23 = (t[c2], t[c3]). Byte permutes over the table held in registers:
// levels 0 - 7 and 8 - 15 are looked up with the codes' low three bits, bit 3 picks per byte.
__device__ __forceinline__ void nf4_lookup4(const Nf4Table& t, uint32_t c, uint32_t& p01,
                                            uint32_t& p23) {
  const uint32_t sel = c & 0x07070707u;
  const uint32_t b3 = c & 0x08080808u;
  const uint32_t m = (b3 << 5) - (b3 >> 3);  // 0xFF in every byte whose code is >= 8
  const uint32_t la = __builtin_amdgcn_perm(t.lo[1], t.lo[0], sel);
  const uint32_t lb = __builtin_amdgcn_perm(t.lo[3], t.lo[2], sel);
  const uint32_t ha = __builtin_amdgcn_perm(t.hi[1], t.hi[0], sel);
  const uint32_t hb = __builtin_amdgcn_perm(t.hi[3], t.hi[2], sel);
  const uint32_t l = (lb & m) | (la & ~m);
  const uint32_t h = (hb & m) | (ha & ~m);
  p01 = __builtin_amdgcn_perm(h, l, 0x05010400u);
  p23 = __builtin_amdgcn_perm(h, l, 0x07030602u);
}

// TAO_NF4_FETCH (timing-only variant builds, experiments/ab_nf4_fetch.sh; every variant forms
// the same w^): 0 = the byte permutes above (built-in); 1 = a select tree per code (the dword of
// the byte tables by bits 3 and 2, the byte by a shift); 2 = the permutes without the final
// interleave in the one-token GEMV, x re-paired once per chunk instead (nf4_decode8_split).
#ifndef TAO_NF4_FETCH
#define TAO_NF4_FETCH 0
#endif

// One code (0 .. 15) -> its table entry (bf16 bits) by selects on register values
__device__ __forceinline__ uint32_t nf4_select1(const Nf4Table& t, uint32_t c) {
  const uint32_t m3 = (c & 8u) ? ~0u : 0u, m2 = (c & 4u) ? ~0u : 0u;
  const uint32_t la = (t.lo[1] & m2) | (t.lo[0] & ~m2), lb = (t.lo[3] & m2) | (t.lo[2] & ~m2);
  const uint32_t ha = (t.hi[1] & m2) | (t.hi[0] & ~m2), hb = (t.hi[3] & m2) | (t.hi[2] & ~m2);
  const uint32_t l = (lb & m3) | (la & ~m3), h = (hb & m3) | (ha & ~m3);
  const uint32_t sh = (c & 3u) * 8u;
  return ((l >> sh) & 0xFFu) | (((h >> sh) & 0xFFu) << 8);
}

// One dword of packed codes -> the pairs (e0, e2), (e1, e3), (e4, e6), (e5, e7): nf4_decode8
// without its interleave, for a caller that pairs x the same way
__device__ __forceinline__ void nf4_decode8_split(const Nf4Table& t, uint32_t w,
                                                  uint32_t (&o)[4]) {
  nf4_lookup4(t, (w >> 4) & 0x0F0F0F0Fu, o[0], o[2]);
  nf4_lookup4(t, w & 0x0F0F0F0Fu, o[1], o[3]);
}

// One dword of packed codes (8 consecutive weights e0 .. e7) -> four bf16 pairs in element
// order: o[0] = (e0, e1), o[1] = (e2, e3), o[2] = (e4, e5), o[3] = (e6, e7).
__device__ __forceinline__ void nf4_decode8(const Nf4Table& t, uint32_t w, uint32_t (&o)[4]) {
#if TAO_NF4_FETCH == 1
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t b = w >> (8 * i);
    o[i] = nf4_select1(t, (b >> 4) & 15u) | (nf4_select1(t, b & 15u) << 16);
  }
  return;
#endif
  const uint32_t ev = (w >> 4) & 0x0F0F0F0Fu;  // e0, e2, e4, e6
  const uint32_t od = w & 0x0F0F0F0Fu;         // e1, e3, e5, e7
  uint32_t e01, e23, o01, o23;                 // (e0, e2), (e4, e6), (e1, e3), (e5, e7)
  nf4_lookup4(t, ev, e01, e23);
  nf4_lookup4(t, od, o01, o23);
  o[0] = __builtin_amdgcn_perm(o01, e01, 0x05040100u);
  o[1] = __builtin_amdgcn_perm(o01, e01, 0x07060302u);
  o[2] = __builtin_amdgcn_perm(o23, e23, 0x05040100u);
  o[3] = __builtin_amdgcn_perm(o23, e23, 0x07060302u);
}

// The 16 levels as 8 bf16 pairs from the tensor's table (32 bytes, 4-byte aligned)
__device__ __forceinline__ void nf4_load_levels(const uint16_t* __restrict__ levels,
                                                uint32_t (&lv)[8]) {
  const uint32_t* p = reinterpret_cast<const uint32_t*>(levels);
#pragma unroll
  for (int i = 0; i < 8; ++i) lv[i] = p[i];
}

}  // namespace tao
