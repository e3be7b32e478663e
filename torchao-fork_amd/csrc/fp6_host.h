// Host-side arithmetic of the FP6 weight-only linear (fp6.hip, torch_ops.cpp): which formats are
// served, which route serves a call, and the decode GEMV's instantiation for a token count. Plain
// functions of their arguments, so that a stand-alone host program can run them on the CPU.
// Internal header.
#pragma once

#include <stdint.h>

namespace tao {

// (ebits, mbits) -> 0 for e3m2, 1 for e2m3, -1 for a pair that is not served
static inline int fp6_format_of(int64_t ebits, int64_t mbits) {
  if (ebits == 3 && mbits == 2) return 0;
  if (ebits == 2 && mbits == 3) return 1;
  return -1;
}

// dwords of native storage per row of K codes (K % 32 == 0): K * 6 / 32
static inline int64_t fp6_row_dwords(int64_t K) { return K / 32 * 6; }

enum { kFp6RouteAuto = 0, kFp6RouteGemv = 1, kFp6RouteDequantMm = 2 };

// The most tokens one GEMV launch serves (fp6wo_gemv_kernel<*, 8, 1, *>); a forced GEMV beyond it
// is a sequence of launches over 8-token pieces.
constexpr int kFp6GemvMaxM = 8;

// Two routes: the decode GEMV, and the dequantizer into a temporary + the bf16 matmul. force:
// tao_tune_fp6's route (kFp6Route*); max_gemv_m > 0 moves the boundary (tao_tune_fp6 too).
// The built-in boundary is measured (experiments/bench_fp6.py --boundary,
// profiles/fp6_bench_boundary.jsonl, both routes forced, e3m2; e2m3 is within 1 %; us GEMV vs
// dequantize + matmul at 4096^2, 6144 x 4096, 14336 x 4096, 4096 x 14336): at M = 8 the GEMV's
// 8-token instance wins at all four shapes (22.9 vs 42.9, 33.3 vs 53.5, 74.0 vs 120.4, 87.8 vs
// 113.6); at M = 16, two 8-token launches, it loses at all four (45.8 vs 42.9, 66.6 vs 52.6,
// 148.2 vs 119.7, 175.7 vs 114.5). N and K do not enter: the rule is M <= 8, one launch.
constexpr int kFp6GemvDefaultM = 8;
static inline int fp6_route(int64_t M, int64_t N, int64_t K, int force, int max_gemv_m) {
  (void)N;
  (void)K;
  if (force == kFp6RouteGemv || force == kFp6RouteDequantMm) return force;
  const int64_t lim = max_gemv_m > 0 ? max_gemv_m : kFp6GemvDefaultM;
  return M <= lim ? kFp6RouteGemv : kFp6RouteDequantMm;
}

// Tokens per lane set (MT) and rows per wave (RPW) of the GEMV launch that serves m <= 8 tokens:
// V = MT * RPW partials per lane, 4 at one token and 8 beyond, as nf4_host.h and the byte-weight
// GEMVs keep it.
struct Fp6GemvTile {
  int mt, rpw;
};
static inline Fp6GemvTile fp6_gemv_tile(int m) {
  if (m <= 1) return {1, 4};
  if (m <= 2) return {2, 4};
  if (m <= 4) return {4, 2};
  return {8, 1};
}

// 32-code groups per lane chunk: 1 (24 B, three 8-B loads, a 2048-code wave slice) unless the
// tuning hook asks for 2 (48 B, three 16-B loads, a 4096-code slice). Measured
// (profiles/fp6_bench.jsonl, us, 24 B vs 48 B at the four shapes): M = 1 5.0 / 6.3 / 10.9 / 12.7
// vs 7.0 / 8.6 / 17.6 / 19.7; M = 4 8.1 / 10.6 / 22.3 / 24.0 vs 11.9 / 21.0 / 39.3 / 37.3;
// M = 8 22.9 / 33.3 / 73.8 / 87.7 vs 36.0 / 53.7 / 126.3 / 195.9. The shorter chunk wins at every
// shape and M (twice the waves along K for the same row).
constexpr int kFp6DefaultGroups = 1;
static inline int fp6_chunk_groups(int tuned) { return tuned == 1 || tuned == 2 ? tuned : kFp6DefaultGroups; }

}  // namespace tao
