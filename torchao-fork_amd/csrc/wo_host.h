// Host-side rules shared by the weight-only linears with a decode GEMV (nf4.hip, fp6.hip,
// uintx.hip, and the tile ladder of the byte-weight GEMVs in tao_gemv.h): which route serves a call
// and which instantiation of the GEMV serves a token count. A format keeps what is its own in its
// *_host.h: the measured default boundary and whether the MFMA GEMM serves a shape. Plain functions
// of their arguments, so that a stand-alone host program can run them on the CPU. Internal header.
#pragma once

#include <stdint.h>

namespace tao {

// tao_tune_{nf4,fp6,uintx}'s route and what tao_*_linear_route answers. The hooks take 0 to 2;
// the MFMA GEMM is only reached through a format's own hook (tao_tune_fp6_mfma, tao_tune_uintx_mfma).
enum { kWoRouteAuto = 0, kWoRouteGemv = 1, kWoRouteDequantMm = 2, kWoRouteMfma = 3 };

// The most tokens one GEMV launch serves (the <8, 1> tile); a forced GEMV beyond it is a sequence
// of launches over 8-token pieces (for_gemv_pieces, tao_gemv.h).
constexpr int kWoGemvMaxM = 8;

// A forced route (1 or 2) wins. Otherwise M <= boundary is the decode GEMV, where max_gemv_m > 0
// (the hooks again) moves the boundary and default_max_m is the format's measured one. Beyond it:
// the dequantizer into a temporary + the bf16 matmul, or, with the format's MFMA hook on and a
// shape its policy of gemm_mfma_kernel serves (mfma_served), the MFMA GEMM instead. N and K do not
// enter any format's measured boundary.
static inline int wo_route(int64_t M, int force, int max_gemv_m, int default_max_m,
                           bool mfma_served) {
  if (force == kWoRouteGemv || force == kWoRouteDequantMm) return force;
  if (M <= (max_gemv_m > 0 ? max_gemv_m : default_max_m)) return kWoRouteGemv;
  return mfma_served ? kWoRouteMfma : kWoRouteDequantMm;
}

// Tokens per lane set (MT) and rows per wave (RPW) of the GEMV launch that serves m <= 8 tokens:
// V = MT * RPW partials per lane, 4 at one token and 8 beyond. At one token the hooks' rows_per_wave
// (2 or 8) replaces RPW (dispatch_gemv_tile, tao_gemv.h).
struct WoGemvTile {
  int mt, rpw;
};
static inline WoGemvTile wo_gemv_tile(int m) {
  if (m <= 1) return {1, 4};
  if (m <= 2) return {2, 4};
  if (m <= 4) return {4, 2};
  return {8, 1};
}

}  // namespace tao
