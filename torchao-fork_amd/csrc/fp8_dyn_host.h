// Host-side arithmetic of the float8-activation linears (scaled_gemv.h, fp8_dyn.hip,
// gemm_mfma.hip): the GEMV launch shape with the fused prologue's token-piece count, for every
// format of scaled_gemv.h, and the per-row format's GEMV / MFMA route choice.
// Plain functions of their arguments, so that a stand-alone host program can run them under the
// sanitizers (experiments/sanitize_fp8dyn_host.hip). Internal header.
#pragma once

#include "tao_gemv.h"

namespace tao {

struct Fp8DynLaunch {
  int S, Wk, G, grid, threads, per;  // per: 16-B pieces of the bf16 token per thread (fused)
  size_t lds;
};

// rpw rows per wave, mt tokens per lane set, (wk, g) the wanted waves along K and row groups;
// fq: the fused one-token launch (the token's codes live in LDS behind the partials); max_per:
// the most token pieces a thread of the kernel to be launched holds (scaled_gemv_kernel 16; the
// decode kernel 8, and 4 with the RMSNorm, whose weight pieces sit beside the token's); chunk_k:
// the k in one 16-B weight chunk (16 e4m3fn codes, 32 e2m1 codes); scale_bytes: the token's block
// scales, which a fused launch keeps behind the codes (rounded up to whole 16 B)
static inline Fp8DynLaunch fp8dyn_launch_shape(int N, int K, int rpw, int mt, int wk, int g,
                                               bool fq, int max_per = 16, int chunk_k = 16,
                                               int scale_bytes = 0) {
  const GemvLaunchShape sh = gemv_launch_shape(K / chunk_k, wk, g);
  Fp8DynLaunch L{sh.S, sh.Wk, sh.G, 0, 0, 0, 0};
  // fq: the token must fit the workgroup's registers (K <= 8 x max_per pieces x threads); row
  // groups are added while they fit 8 waves
  while (fq && (int64_t)64 * L.Wk * L.G * 8 * max_per < K && L.Wk * L.G * 2 <= 8) L.G *= 2;
  const int rows_per_wg = L.G * rpw;
  L.grid = (int)(((int64_t)N + rows_per_wg - 1) / rows_per_wg);  // (N up to 2^31 - 1)
  const int nw = L.G * L.Wk;
  L.threads = 64 * nw;
  L.lds = (size_t)nw * rpw * mt * sizeof(float);
  if (fq) {
    L.lds = (((size_t)nw * rpw * mt + 8 + 3) & ~(size_t)3) * sizeof(float) + (size_t)K +
            (size_t)((scale_bytes + 15) & ~15);
    L.per = (K / 8 + L.threads - 1) / L.threads;
  }
  return L;
}

// The GEMV / MFMA crossover, from experiments/bench_fp8dyn.py (profiles/fp8dyn_bench.jsonl, both
// kernels forced at M = 1..8): the GEMV wins at M = 1 everywhere (4096^2 5.2 vs 6.8 us) and up to
// M = 4 on weights of <= 32 Mi codes (4096^2 M = 4: 6.6 vs 7.1 us); on the larger ones the MFMA
// kernel already wins at M = 2 (14336 x 4096: 12.9 vs 13.9 us, M = 4: 13.0 vs 17.7 us), and at
// M = 8 everywhere (7.0 vs 12.8 us). force_mfma: tao_tune_fp8dyn_mfma; max_gemv_m > 0:
// tao_tune_linear_crossover.
static inline bool fp8dyn_route_gemv(int64_t M, int64_t N, int64_t K, int force_mfma,
                                     int max_gemv_m) {
  if (force_mfma != 0) return false;
  if (max_gemv_m > 0) return M <= max_gemv_m;
  return M <= 1 || (M <= 4 && N * K <= (32LL << 20));
}

}  // namespace tao
