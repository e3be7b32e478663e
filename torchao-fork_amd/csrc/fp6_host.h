// Host-side arithmetic of the FP6 weight-only linear (fp6.hip, torch_ops.cpp) that is the format's
// own: which formats are served, the measured boundary of its route rule and the lane chunk. The
// rule itself and the decode GEMV's instantiation for a token count are in wo_host.h. Plain
// functions of their arguments, so that a stand-alone host program can run them on the CPU.
// Internal header.
#pragma once

#include <stdint.h>

#include "wo_host.h"

namespace tao {

// (ebits, mbits) -> 0 for e3m2, 1 for e2m3, -1 for a pair that is not served
static inline int fp6_format_of(int64_t ebits, int64_t mbits) {
  if (ebits == 3 && mbits == 2) return 0;
  if (ebits == 2 && mbits == 3) return 1;
  return -1;
}

// dwords of native storage per row of K codes (K % 32 == 0): K * 6 / 32
static inline int64_t fp6_row_dwords(int64_t K) { return K / 32 * 6; }

// Two built-in routes (wo_route): the decode GEMV, and the dequantizer into a temporary + the bf16
// matmul. force: tao_tune_fp6's route (kWoRoute*); max_gemv_m > 0 moves the boundary (tao_tune_fp6 too).
// The built-in boundary is measured (experiments/bench_fp6.py --boundary,
// profiles/fp6_bench_boundary.jsonl, both routes forced, e3m2; e2m3 is within 1 %; us GEMV vs
// dequantize + matmul at 4096^2, 6144 x 4096, 14336 x 4096, 4096 x 14336): at M = 8 the GEMV's
// 8-token instance wins at all four shapes (22.9 vs 42.9, 33.3 vs 53.5, 74.0 vs 120.4, 87.8 vs
// 113.6); at M = 16, two 8-token launches, it loses at all four (45.8 vs 42.9, 66.6 vs 52.6,
// 148.2 vs 119.7, 175.7 vs 114.5). N and K do not enter: the rule is M <= 8, one launch.
// A third route, the Fp6WO policy of gemm_mfma_kernel (gemm_mfma.hip), is behind a hook of its
// own (mfma: tao_tune_fp6_mfma): with it on, every call this rule would send to dequantize +
// matmul goes to the MFMA GEMM instead. A forced route still wins, and max_gemv_m still moves the
// GEMV boundary. The built-in rule does not name it yet (measurements: DESIGN §4.20).
constexpr int kFp6GemvDefaultM = 8;
static inline int fp6_route(int64_t M, int force, int max_gemv_m, int mfma) {
  return wo_route(M, force, max_gemv_m, kFp6GemvDefaultM, mfma != 0);
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
