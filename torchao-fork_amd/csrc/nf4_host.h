// Host-side arithmetic of the NF4 linear (nf4.hip, torch_ops.cpp): which route serves a call, and
// the decode GEMV's instantiation for a token count. Plain functions of their arguments, so that
// a stand-alone host program can run them on the CPU. Internal header.
#pragma once

#include <stdint.h>

namespace tao {

enum { kNf4RouteAuto = 0, kNf4RouteGemv = 1, kNf4RouteDequantMm = 2 };

// The most tokens one GEMV launch serves (nf4_gemv_kernel<8, 1>); a forced GEMV beyond it is a
// sequence of launches over 8-token pieces.
constexpr int kNf4GemvMaxM = 8;

// Two routes: the decode GEMV, and the dequantizer into a temporary + the bf16 matmul (the
// reference's own form with a fast dequantizer). force: tao_tune_nf4's route (kNf4Route*);
// max_gemv_m > 0 moves the boundary (tao_tune_nf4 too). The built-in boundary is measured
// (experiments/bench_nf4.py --boundary, profiles/nf4_bench_boundary.jsonl, both routes forced; us
// GEMV vs dequantize + matmul): at M = 4 the GEMV wins at all four shapes (4096^2 8.2 vs 37.4,
// 14336 x 4096 22.3 vs 65.2, 4096 x 14336 26.4 vs 61.8); its 8-token instance (one row per wave)
// still wins on the two smaller weights (20.8 vs 37.4, 30.1 vs 39.7) but loses at 14336 x 4096
// (66.9 vs 63.8) and at 4096 x 14336 (72.2 vs 59.5); at M = 16 it loses everywhere. N and K do
// not enter: the rule is M <= 4.
constexpr int kNf4GemvDefaultM = 4;
static inline int nf4_route(int64_t M, int64_t N, int64_t K, int force, int max_gemv_m) {
  (void)N;
  (void)K;
  if (force == kNf4RouteGemv || force == kNf4RouteDequantMm) return force;
  const int64_t lim = max_gemv_m > 0 ? max_gemv_m : kNf4GemvDefaultM;
  return M <= lim ? kNf4RouteGemv : kNf4RouteDequantMm;
}

// Tokens per lane set (MT) and rows per wave (RPW) of the GEMV launch that serves m <= 8 tokens:
// V = MT * RPW partials per lane, 4 at one token and 8 beyond, as the byte-weight GEMVs keep it.
struct Nf4GemvTile {
  int mt, rpw;
};
static inline Nf4GemvTile nf4_gemv_tile(int m) {
  if (m <= 1) return {1, 4};
  if (m <= 2) return {2, 4};
  if (m <= 4) return {4, 2};
  return {8, 1};
}

// Factors (one per 256 blocks of 64 weights) a weight of N x K holds: ceil(N K / 16384)
static inline int64_t nf4_num_factors(int64_t N, int64_t K) {
  return (N * K + 16383) / 16384;
}

}  // namespace tao
