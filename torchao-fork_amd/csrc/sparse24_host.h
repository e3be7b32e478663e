// Host-side rules of the 2:4 sparse int8 linear (sparse24.hip): which route serves a call and the
// launch shape of the sparse MFMA GEMM. Plain functions of their arguments, so that a stand-alone
// host program can run them on the CPU. Internal header.
#pragma once

#include <stdint.h>

#include "wo_host.h"

namespace tao {

// tao_tune_sp24's route and what tao_int8_sp24_route answers
enum { kSp24RouteAuto = 0, kSp24RouteGemv = 1, kSp24RouteGemm = 2 };

// The GEMV serves up to this many tokens by default: the largest measured M at which it beats the
// GEMM at all four shapes (experiments/bench_sp24.py --boundary, profiles/sp24_bench_boundary.jsonl;
// GEMV / GEMM at M = 2: 0.68, 0.77, 0.69, 0.52; at M = 4: 0.84, 0.89, 1.00, 1.02; at M = 8: 1.6-2.6).
constexpr int kSp24GemvDefaultMaxM = 2;
// The GEMV stages its int8 tokens in LDS, MT x K bytes for the MT tokens of its tile
// (wo_gemv_tile; a launch serves up to kWoGemvMaxM tokens, a forced GEMV beyond it is a sequence of
// launches). Together with the reduction's partials and wave maxima (under 1 KiB: 8 waves x 8
// values + 8 words) they stay inside the 64 KiB of dynamic LDS a kernel has without asking for
// more; what does not fit goes to the GEMM.
constexpr int64_t kSp24GemvMaxXBytes = 65536 - 1024;

static inline bool sp24_gemv_fits(int64_t M, int64_t K) {
  return wo_gemv_tile((int)(M < kWoGemvMaxM ? M : kWoGemvMaxM)).mt * K <= kSp24GemvMaxXBytes;
}

// A forced route wins (a forced GEMV whose tokens do not fit LDS is refused by the entry).
// Otherwise M <= boundary is the GEMV where its tokens fit, everything else the sparse MFMA GEMM.
static inline int sp24_route(int64_t M, int64_t K, int force, int max_gemv_m) {
  if (force == kSp24RouteGemv || force == kSp24RouteGemm) return force;
  const int bound = max_gemv_m > 0 ? max_gemv_m : kSp24GemvDefaultMaxM;
  return (M <= bound && sp24_gemv_fits(M, K)) ? kSp24RouteGemv : kSp24RouteGemm;
}

// Launch shape of sp24_gemm_kernel: BM tokens per tile (16, 32, 64), NWV waves of 16 output
// features per k-group (1, 2, 4), KG k-groups. Narrower tiles until the grid covers the 256 CUs;
// k-groups fill the workgroup up to 8 waves and 64 KiB of x tiles (KG * 2 * BM * 128 B).
struct Sp24GemmShape {
  int bm, nwv, kg;
};
static inline Sp24GemmShape sp24_gemm_shape(int64_t M, int64_t N, int64_t K, int tbm, int tnwv,
                                            int tkg) {
  Sp24GemmShape s;
  s.bm = tbm > 0 ? tbm : (M <= 16 ? 16 : M <= 32 ? 32 : 64);
  const int64_t mt = (M + s.bm - 1) / s.bm;
  s.nwv = 4;
  while (s.nwv > 1 && ((N + 16 * s.nwv - 1) / (16 * s.nwv)) * mt < 256) s.nwv >>= 1;
  if (tnwv > 0) s.nwv = tnwv;
  const int nsteps = (int)(K / 128);
  int kg = 8 / s.nwv;
  if (kg > 256 / s.bm) kg = 256 / s.bm;
  if (tkg > 0 && tkg < kg) kg = tkg;
  if (kg > nsteps) kg = nsteps;
  s.kg = kg < 1 ? 1 : kg;
  return s;
}

}  // namespace tao
