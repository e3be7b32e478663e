// Host-side rules of the NVFP4 linear (nvfp4.hip, torch_ops.cpp) that are the format's own: the
// block, the two scale layouts, the shapes the kernels serve, the lane chunk of the decode GEMV and
// the default boundary of its route rule. The rule itself and the GEMV's instantiation for a token
// count are in wo_host.h. Plain functions of their arguments, so that a stand-alone host program
// can run them on the CPU. Internal header.
#pragma once

#include <stdint.h>

#include "wo_host.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TAO_NVFP4_HD __attribute__((host)) __attribute__((device)) inline
#else
#define TAO_NVFP4_HD inline
#endif

namespace tao {

// e2m1 codes per e4m3fn scale byte
constexpr int kNvfp4Block = 16;
// A lane's chunk of the GEMV: 32 k = 16 B of codes (one load) and the 2 scale bytes of its two
// blocks (one aligned 2-B load in either layout); a wave slice is 2048 k, as for int4 nibbles.
constexpr int kNvfp4ChunkK = 32;

// ceil(cols / 4): the column tiles of the swizzled layout of a [rows][cols] scale matrix
TAO_NVFP4_HD int64_t nvfp4_col_tiles(int64_t cols) { return (cols + 3) / 4; }

// Byte offset of scale (r, c) in the swizzled ("blocked") layout: tiles of 128 rows x 4 columns,
// row tiles outermost, each stored as 32 x 16 bytes. The four c % 4 bytes of a row are adjacent.
TAO_NVFP4_HD int64_t nvfp4_scale_offset(int64_t r, int64_t c, int64_t ncb) {
  return (((r / 128) * ncb + c / 4) * 32 + r % 32) * 16 + ((r % 128) / 32) * 4 + c % 4;
}

// Scale bytes of [rows][K / 16] scales: row-major, or swizzled with its zero padding
static inline int64_t nvfp4_scale_bytes(int64_t rows, int64_t K, bool swizzled) {
  const int64_t cols = K / kNvfp4Block;
  if (!swizzled) return rows * cols;
  return (rows + 127) / 128 * 128 * nvfp4_col_tiles(cols) * 4;
}

// What the linear's kernels serve: N % 16 == 0 (the reference's own rule) and K % 64 == 0 (whole
// lane chunks, and no column padding in the swizzled layout).
static inline bool nvfp4_shape_ok(int64_t N, int64_t K) {
  return N > 0 && K > 0 && N % 16 == 0 && K % 64 == 0;
}

// Two routes (wo_route): the decode GEMV, and the dequantizer into a temporary + the bf16 matmul
// (after the activation snap in DYNAMIC mode). force and max_gemv_m are tao_tune_nvfp4's.
// The built-in boundary is measured (experiments/bench_nvfp4.py --boundary,
// profiles/nvfp4_bench_boundary.jsonl, both routes forced, WEIGHT_ONLY; DYNAMIC adds about 3 us to
// either; us GEMV vs dequantize + matmul at 4096^2, 6144 x 4096, 14336 x 4096, 4096 x 14336): at
// M = 4 the GEMV wins at all four shapes (8.7 vs 36.2, 14.2 vs 36.3, 28.1 vs 65.3, 36.2 vs 62.8);
// at M = 8, the 8-token instance, it wins at two and loses at two (22.3 vs 35.9, 33.0 vs 36.4,
// 74.4 vs 67.6, 95.2 vs 62.8); at M = 16, two launches, it loses at all four. N and K do not
// enter: the rule is M <= 4, the last count at which the GEMV wins everywhere.
// A third route, the Nvfp4WO policy of gemm_mfma_kernel (gemm_mfma.hip), is behind a hook of its
// own (mfma: tao_tune_nvfp4_mfma): with it on, every call this rule would send to dequantize +
// matmul goes to the MFMA GEMM instead, in both modes and both scale layouts. A forced route still
// wins, and max_gemv_m still moves the GEMV boundary. The built-in rule does not name it yet
// (measurements: DESIGN §4.25.1).
constexpr int kNvfp4GemvDefaultM = 4;
// The MFMA GEMM serves every shape the linear serves: its step is 256 k with 64-k tails masked.
static inline bool nvfp4_mfma_ok(int64_t N, int64_t K) { return nvfp4_shape_ok(N, K); }
static inline int nvfp4_route(int64_t M, int64_t N, int64_t K, int force, int max_gemv_m,
                              int mfma) {
  return wo_route(M, force, max_gemv_m, kNvfp4GemvDefaultM, mfma != 0 && nvfp4_mfma_ok(N, K));
}

}  // namespace tao
