// Host-side arithmetic of the uintx (1- to 7-bit) weight-only linear (uintx.hip, torch_ops.cpp)
// that is the format's own: which shards a width has, the measured boundary of its route rule,
// what the MFMA GEMM serves, the decode GEMV's lane unit and where it reads x. The rule itself and
// the GEMV's instantiation for a token count are in wo_host.h. Plain functions of their arguments,
// so that a stand-alone host program can run them on the CPU. Internal header.
#pragma once

#include <stdint.h>

#include "wo_host.h"

namespace tao {

// A code of `bits` bits is cut into shards of 4, 2 and 1 bits: the set bits of `bits` itself.
static inline bool uintx_bits_ok(int64_t bits) { return bits >= 1 && bits <= 7; }
static inline bool uintx_has_s4(int bits) { return (bits & 4) != 0; }
static inline bool uintx_has_s2(int bits) { return (bits & 2) != 0; }
static inline bool uintx_has_s1(int bits) { return (bits & 1) != 0; }

// What the HIP kernels serve: K % 128 == 0 (K / 8 a multiple of 16: every shard address of a
// 16-byte unit is 16-B aligned) and groups that a 16-element unit never straddles. The kernels
// divide by the group size with uintx_group_mul, exact for every k < K where the group size is a
// power of two or K * group < 2^32.
static inline bool uintx_shape_ok(int64_t K, int64_t group) {
  return K > 0 && K < (1LL << 31) && K % 128 == 0 && group > 0 && group % 16 == 0 &&
         K % group == 0 && ((group & (group - 1)) == 0 || K * group < (1LL << 32));
}
// ceil(2^32 / group): k / group == umulhi(k, mul). With e = mul * group - 2^32 < group the
// quotient is exact while k * e < 2^32; e == 0 for a power of two.
static inline uint32_t uintx_group_mul(int64_t group) {
  return (uint32_t)(((1LL << 32) + group - 1) / group);
}

// Two built-in routes (wo_route): the decode GEMV, and the dequantizer into a temporary + the bf16
// matmul. force: tao_tune_uintx's route (kWoRoute*); max_gemv_m > 0 moves the boundary (tao_tune_uintx too).
// The built-in boundary is measured per width (experiments/bench_uintx.py --boundary,
// profiles/uintx_bench_boundary.jsonl, both routes forced at M = 4, 8, 12, 16; us GEMV vs
// dequantize + matmul at 4096^2, 6144 x 4096, 14336 x 4096, 4096 x 14336). M = 8: uint1 13.5 /
// 18.6 / 36.3 / 37.2 vs 32.7 / 35.1 / 59.5 / 56.1, uint7 15.8 / 20.5 / 41.0 / 48.1 vs 31.1 / 35.1 /
// 59.2 / 57.5: the GEMV wins at all four shapes for every width. M = 12 (8 + 4 tokens): it wins
// at the two smaller shapes for every width, loses at 4096 x 14336 from uint2 up (uint4 59.0 vs
// 54.7) and at 14336 x 4096 from uint5 up (uint4 ties, 56.1 vs 56.7; uint5 60.8 vs 57.9).
// M = 16: it wins at 4096^2 only (uint1 25.8 / 35.1 / 70.5 / 73.5 vs 32.1 / 34.8 / 59.5 / 56.4). So M <= 8 for every width: the largest measured M
// without a losing shape; it loses at all four shapes at no measured M.
static inline int uintx_default_max_m(int bits) {
  (void)bits;
  return 8;
}
// What the UintxWO policy of gemm_mfma_kernel serves (gemm_mfma_policy.h): each of its MFMAs takes
// the 32 consecutive k of one aligned 32-k block and meets one (scale, zero point) pair, so a
// group must be a whole number of such blocks. K needs nothing beyond uintx_shape_ok: where
// K / 8 is an odd multiple of 16 the odd segments' step windows start 16 positions early, which
// keeps every MFMA on an aligned block. group_size <= 0: not known to the caller
// (tao_uintx_linear_route), taken as served.
static inline bool uintx_mfma_ok(int64_t K, int64_t group) {
  if (group <= 0) return K > 0 && K < (1LL << 31) && K % 128 == 0;
  return uintx_shape_ok(K, group) && group % 32 == 0;
}

// A third route, the UintxWO policy of gemm_mfma_kernel, is behind a hook of its own (mfma:
// tao_tune_uintx_mfma): with it on, every call this rule would send to dequantize + matmul, and
// that uintx_mfma_ok serves, goes to the MFMA GEMM instead. A forced route still wins, and
// max_gemv_m still moves the GEMV boundary. The built-in rule does not name it yet (measurements
// and the boundary they suggest: DESIGN 4.23.1).
static inline int uintx_route(int64_t M, int64_t K, int bits, int64_t group, int force,
                              int max_gemv_m, int mfma) {
  return wo_route(M, force, max_gemv_m, uintx_default_max_m(bits),
                  mfma && uintx_mfma_ok(K, group));
}

// Bytes of each shard stream per lane unit (U = 4, 8 or 16: 32, 64 or 128 codes); a row has
// K / (8 U) units. The built-in choice follows profiles/uintx_bench.jsonl, where every unit was
// forced at every width at K = 4096 (N 4096, 6144, 14336) and K = 14336 (N 4096); other K take the
// rule of the nearer regime and are not measured.
//   * K >= 8192 (a 16-byte unit still fills a wave): 16 B. At K = 14336 it is the fastest at every
//     width at M = 1 (8.8 .. 15.6 us vs 9.7 .. 20.2 for 8 B) and at most widths beyond. Exceptions,
//     each seen in two separate runs: more than 4 tokens at uint2, uint6, uint7 (16 B 48.7 / 51.4 /
//     51.7 vs 8 B 41.4 / 45.7 / 47.5 us at 4096 x 14336, M = 8), whose <*, 8, 1, 16> instances take
//     66 / 71 / 70 VGPRs and hold 7 waves per SIMD, three 8-wave workgroups per CU, where the other
//     widths' (62 to 64 VGPRs) hold 8 and four; and 3 to 4 tokens (the 4 x 2 tile) at uint2, uint3
//     (20.6 / 23.1 vs 18.3 / 20.0 us at M = 4; <*, 4, 2, 16> holds 7 waves at every width up to
//     uint3, so occupancy alone does not explain these two). They take 8 B. At 2 tokens (the 2 x 4
//     tile) 16 B wins or ties at every width (uint2 10.9 vs 21.9 us for 8 B).
//   * 4096 <= K < 8192, more than 4 tokens (the 8 x 1 tile): 8 B, 1.3 to 1.7 times faster than
//     either other unit at every width and N.
//   * 4096 <= K < 8192, one token: 8 B for uint1 .. uint3 and uint7, 4 B for uint4 .. uint6 (4 B
//     6.1 / 6.5 / 7.0 vs 8 B 7.3 / 8.6 / 8.2 us at 4096^2; uint7: 8 B wins or ties at two of the
//     three N).
//   * 4096 <= K < 8192, 2 tokens (the 2 x 4 tile): 4 B for uint2 .. uint5, 8 B for uint1, uint6,
//     uint7 (the faster in the sum over the three N; 8 B is twice as slow as 4 B at uint2 .. uint4:
//     12.7 / 14.2 / 10.8 vs 6.3 / 6.7 / 6.9 us at 4096^2).
//   * 4096 <= K < 8192, 3 to 4 tokens: 8 B for uint1 .. uint4, 4 B for uint5 .. uint7 (M = 4 at
//     4096^2: uint3 7.2 vs 8.6, uint4 9.0 vs 8.9, uint5 10.3 vs 9.0, uint7 12.8 vs 9.8 us, 8 B vs
//     4 B).
//   * K < 4096: 4 B (more units per row than lanes only there).
// tuned: tao_tune_uintx's unit; rpw: its rows per wave at one token. 8 rows per wave take at most
// an 8-byte unit: 8 rows x 7 pieces x 4 dwords of a 16-byte one do not fit the register file (the
// 5- to 7-bit instances spilled).
static inline int uintx_unit(int64_t K, int bits, int64_t m, int tuned, int rpw) {
  int u = tuned;
  if (u != 4 && u != 8 && u != 16) {
    if (K >= 8192)
      u = (m > 4 ? (bits == 2 || bits >= 6) : (m > 2 && (bits == 2 || bits == 3))) ? 8 : 16;
    else if (K < 4096) u = 4;
    else if (m > 4) u = 8;
    else if (m <= 1) u = (bits >= 4 && bits <= 6) ? 4 : 8;
    else if (m == 2) u = (bits >= 2 && bits <= 5) ? 4 : 8;
    else u = bits >= 5 ? 4 : 8;
  }
  return (rpw == 8 && m <= 1 && u > 8) ? 8 : u;
}

// x of the GEMV launch that serves m tokens: staged once per workgroup in LDS (true) or read
// through L1 (false). Only the 4 x 2 and 8 x 1 tiles (m > 2) have a staged instance, and only while
// the m-token tile's [MT][K] bf16 fits 128 KiB of the CU's 160 KiB next to the partials (8 tokens:
// K <= 8192; 4 tokens: K <= 16384); beyond that x goes through L1, which at K = 14336 still beats
// the dequantize + matmul route. tuned: tao_tune_uintx's x_lds (1 = L1, 2 = LDS where it fits).
// Built-in, measured with both forms forced at every lane unit (profiles/uintx_bench.jsonl,
// gemv_xl1_u* / gemv_xlds_u*, us at N = 4096 / 6144 / 14336, the rule's unit):
//   * K = 4096, M = 4, uint4 .. uint7: LDS wins, 6 to 8 % in the sum over N and up to 14 % at
//     N = 14336 (uint4 8.2 / 11.9 / 18.8 vs 9.0 / 12.1 / 20.8; uint6 9.5 / 12.2 / 22.5 vs 9.4 /
//     13.0 / 25.4). uint1 .. uint3 tie within 2 % (uint1 7.2 / 10.3 / 16.5 vs 6.5 / 10.1 / 16.9).
//   * K = 4096, M = 8: LDS wins 5 to 7 % at N = 4096 (uint4 13.2 vs 14.1), ties at 6144 and loses
//     7 % at 14336 (39.0 vs 36.6): through L1 is faster in the sum at every width.
//   * K = 14336, M = 4: the 112 KiB of x leave one workgroup per CU; LDS loses 25 to 35 %
//     (uint1 22.1 vs 16.5). M = 8 does not fit.
// So: staged in LDS at 3 to 4 tokens for uint4 .. uint7 at 4096 <= K < 8192, through L1 elsewhere
// (K < 4096 is not measured and takes L1).
static inline int64_t uintx_x_lds_bytes(int64_t K, int mt) { return (int64_t)mt * K * 2; }
static inline bool uintx_x_lds(int64_t K, int bits, int64_t m, int tuned) {
  if (m <= 2 || uintx_x_lds_bytes(K, m <= 4 ? 4 : 8) > 128 * 1024) return false;
  if (tuned == 1 || tuned == 2) return tuned == 2;
  return m <= 4 && bits >= 4 && K >= 4096 && K < 8192;
}

}  // namespace tao
