// Host-side arithmetic of the grouped (MoE) int4 expert GEMM (moe_gemm.hip, torch_ops.cpp): the
// bounds the entries check, the row tile of a launch, whether gate and up share a launch, and the
// grid's upper bound. Plain functions of their arguments, so that a stand-alone host program can
// run them on the CPU. Internal header.
#pragma once

#include <stdint.h>

namespace tao {

constexpr int kMoeMaxExperts = 256;  // E: a wave finds its tile in four offsets per lane
constexpr int kMoeMaxTopK = 8;       // A: the combine keeps a token's positions in registers

// Rows per tile (BM) of tao_int4wo_grouped_linear_bf16 for R = T * A sorted rows over E experts;
// tuned: tao_tune_moe's bm (0 = this rule). An expert's c_e rows take ceil(c_e / BM) tiles, each of
// which streams the expert's whole [64][K] weight slice, so BM wants to cover the mean count R / E
// without padding a short expert to a long tile. Measured (experiments/bench_moe.py,
// profiles/moe_bench.jsonl; Mixtral-8x7B shapes, E = 8, top-2, g 32; us per expert FFN, gate and up
// in one launch, BM 16 / 32 / 64, uniform routing; skewed routing orders them the same way):
//   R =    4 (T = 2)     115 /  124 /  222        R =  128 (T = 64)     379 /  268 /  360
//   R =    8 (T = 4)     187 /  188 /  281        R =  512 (T = 256)   1127 /  710 /  621
//   R =   16 (T = 8)     241 /  249 /  350        R = 2048 (T = 1024)  3951 / 2234 / 1665
//   R =   32 (T = 16)    245 /  252 /  352
// 16 wins up to a mean of 4 rows per expert (by 1-8 %), 32 at a mean of 16 (by 29 %), 64 from a
// mean of 64 (by 13-25 %). Between the measured points (means of 4 to 16, and of 16 to 64) the
// thresholds are a supposition: the larger tile from the first measured point where it won, except
// that 32 starts right after the last point where 16 won, since 16 loses far more at a mean of 16
// (41 %) than 32 loses at a mean of 4 (3 %).
static inline int moe_row_tile(int64_t R, int64_t E, int tuned) {
  if (tuned == 16 || tuned == 32 || tuned == 64) return tuned;
  if (E <= 0 || R <= 4 * E) return 16;
  return R >= 64 * E ? 64 : 32;
}

// Gate and up in one launch (two accumulator sets over one x tile, SwiGLU in the epilogue):
// tuned: tao_tune_moe's dual (0 = this rule, 1 = never, 2 = always). Every BM's dual instance is
// free of scratch (csrc/resource_usage.py). Measured in the same runs, us per expert
// FFN, two launches + torch's silu and mul vs one launch: BM 16 117 / 185 / 240 / 246 / 389 vs
// 115 / 187 / 241 / 245 / 379 (T = 2 .. 64; a tie within the 1-2 % either way); BM 32 129 / 194 /
// 259 / 264 / 287 / 763 / 2423 vs 124 / 188 / 249 / 252 / 268 / 710 / 2234 (T = 2 .. 1024); BM 64
// 445 / 752 / 2020 vs 360 / 621 / 1665 (T = 64 .. 1024). The one launch never loses by more than
// 1 %, so every BM keeps the dual form.
static inline bool moe_dual(int bm, int tuned) {
  (void)bm;
  return tuned != 1;
}

// grid.y of the grouped launch: an upper bound on sum_e ceil(c_e / BM) known on the host. Every
// expert with rows adds at most one partial tile: at most min(E, R) of them.
static inline int64_t moe_tile_bound(int64_t R, int64_t E, int bm) {
  return R / bm + (E < R ? E : R);
}

}  // namespace tao
