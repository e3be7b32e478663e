// Host-side arithmetic of the NF4 linear (nf4.hip, torch_ops.cpp) that is the format's own: the
// measured boundary of its route rule and the factor count. The rule itself and the decode GEMV's
// instantiation for a token count are in wo_host.h. Plain functions of their arguments, so that
// a stand-alone host program can run them on the CPU. Internal header.
#pragma once

#include <stdint.h>

#include "wo_host.h"

namespace tao {

// Two routes (wo_route without an MFMA GEMM): the decode GEMV, and the dequantizer into a
// temporary + the bf16 matmul (the reference's own form with a fast dequantizer). force:
// tao_tune_nf4's route (kWoRoute*); max_gemv_m > 0 moves the boundary (tao_tune_nf4 too). The
// built-in boundary is measured
// (experiments/bench_nf4.py --boundary, profiles/nf4_bench_boundary.jsonl, both routes forced; us
// GEMV vs dequantize + matmul): at M = 4 the GEMV wins at all four shapes (4096^2 8.2 vs 37.4,
// 14336 x 4096 22.3 vs 65.2, 4096 x 14336 26.4 vs 61.8); its 8-token instance (one row per wave)
// still wins on the two smaller weights (20.8 vs 37.4, 30.1 vs 39.7) but loses at 14336 x 4096
// (66.9 vs 63.8) and at 4096 x 14336 (72.2 vs 59.5); at M = 16 it loses everywhere. N and K do
// not enter: the rule is M <= 4.
constexpr int kNf4GemvDefaultM = 4;
static inline int nf4_route(int64_t M, int force, int max_gemv_m) {
  return wo_route(M, force, max_gemv_m, kNf4GemvDefaultM, false);
}

// Factors (one per 256 blocks of 64 weights) a weight of N x K holds: ceil(N K / 16384)
static inline int64_t nf4_num_factors(int64_t N, int64_t K) {
  return (N * K + 16383) / 16384;
}

}  // namespace tao
