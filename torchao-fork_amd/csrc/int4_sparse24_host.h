// Host-side rules of the 2:4 sparse int4 weight-only linear (int4_sparse24.hip): which route serves
// a call and the launch shape of the sparse MFMA GEMM. Plain functions of their arguments, so that a
// stand-alone host program can run them on the CPU. Internal header.
#pragma once

#include <stdint.h>

#include "wo_host.h"

namespace tao {

// tao_tune_int4_sp24's route and what tao_int4_sp24_route answers
enum { kI4Sp24RouteAuto = 0, kI4Sp24RouteGemv = 1, kI4Sp24RouteGemm = 2 };

// The GEMV serves up to this many tokens by default: the largest measured M at which it beats the
// GEMM at every shape where its tokens fit LDS (experiments/bench_int4_sp24.py --boundary,
// profiles/int4_sp24_bench_boundary.jsonl; GEMV / GEMM at M = 1: 0.70, 0.60, 0.53, 0.41; at M = 2:
// 0.81, 0.69, 0.67, 0.50; at M = 4: 0.74, 0.89, 0.89, the fourth shape does not fit). Five to eight
// tokens use the 8-token tile, which does not fit from K = 4096 on.
constexpr int kI4Sp24GemvDefaultMaxM = 4;
// The GEMV stages its bf16 tokens in LDS, MT x 2 K bytes for the MT tokens of its tile
// (wo_gemv_tile). Together with the reduction's partials (under 1 KiB) they stay inside the 64 KiB
// of dynamic LDS a kernel has without asking for more; what does not fit goes to the GEMM.
constexpr int64_t kI4Sp24GemvMaxXBytes = 65536 - 1024;

static inline bool i4sp24_gemv_fits(int64_t M, int64_t K) {
  return wo_gemv_tile((int)(M < kWoGemvMaxM ? M : kWoGemvMaxM)).mt * 2 * K <= kI4Sp24GemvMaxXBytes;
}

// A forced route wins (a forced GEMV whose tokens do not fit LDS is refused by the entry).
// Otherwise M <= boundary is the GEMV where its tokens fit, everything else the sparse MFMA GEMM.
static inline int i4sp24_route(int64_t M, int64_t K, int force, int max_gemv_m) {
  if (force == kI4Sp24RouteGemv || force == kI4Sp24RouteGemm) return force;
  const int bound = max_gemv_m > 0 ? max_gemv_m : kI4Sp24GemvDefaultMaxM;
  return (M <= bound && i4sp24_gemv_fits(M, K)) ? kI4Sp24RouteGemv : kI4Sp24RouteGemm;
}

// Launch shape of int4_sp24_gemm_kernel: BM tokens per tile (16, 32, 64), NWV waves of 16 output
// features per k-group (1, 2, 4), KG k-groups. Narrower tiles until the grid covers the 256 CUs;
// k-groups fill the workgroup up to 8 waves and 64 KiB of x tiles (KG * 2 * BM * 256 B).
struct I4Sp24GemmShape {
  int bm, nwv, kg;
};
static inline I4Sp24GemmShape i4sp24_gemm_shape(int64_t M, int64_t N, int64_t K, int tbm, int tnwv,
                                                int tkg) {
  I4Sp24GemmShape s;
  s.bm = tbm > 0 ? tbm : (M <= 16 ? 16 : M <= 32 ? 32 : 64);
  const int64_t mt = (M + s.bm - 1) / s.bm;
  s.nwv = 4;
  while (s.nwv > 1 && ((N + 16 * s.nwv - 1) / (16 * s.nwv)) * mt < 256) s.nwv >>= 1;
  if (tnwv > 0) s.nwv = tnwv;
  const int nsteps = (int)(K / 128);
  int kg = 8 / s.nwv;
  if (kg > 128 / s.bm) kg = 128 / s.bm;
  if (tkg > 0 && tkg < kg) kg = tkg;
  if (kg > nsteps) kg = nsteps;
  s.kg = kg < 1 ? 1 : kg;
  return s;
}

}  // namespace tao
