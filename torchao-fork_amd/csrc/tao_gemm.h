// The linear kernels' functions that are called across source files. Internal header: each
// definer and each caller includes it, so a signature is written once.
#pragma once

#include "tao_common.h"

namespace tao {

// int4_gemv.hip, int8_gemv.hip, fp8_gemv.hip: the decode GEMVs behind the weight-only linears
int int4wo_gemv(const uint16_t* x, const uint32_t* packed, const uint16_t* sz,
                const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                int64_t group_size, hipStream_t stream);
int int4_check_linear_args(const uint16_t* x, const uint32_t* packed, const uint16_t* sz,
                           uint16_t* y, int64_t M, int64_t N, int64_t K, int64_t group_size);
int int8wo_gemv(const uint16_t* x, const int8_t* w, const uint16_t* scale, const uint16_t* bias,
                uint16_t* y, int64_t M, int64_t N, int64_t K, hipStream_t stream);
int fp8wo_gemv(const uint16_t* x, const uint8_t* w, const float* scale, const uint16_t* bias,
               uint16_t* y, int64_t M, int64_t N, int64_t K, hipStream_t stream);

// gemm_tile.hip: the weight-shared tile GEMM (4 waves split the rows, weights dequantised once per
// workgroup) and its routing rule
int tile_int4(const uint16_t* x, const uint32_t* packed, const uint16_t* sz, int gshift,
              const uint16_t* bias, uint16_t* y, int M, int N, int K, hipStream_t stream,
              int splits);
int tile_int8wo(const uint16_t* x, const int8_t* w, const uint16_t* scale, const uint16_t* bias,
                uint16_t* y, int M, int N, int K, hipStream_t stream, int splits);
int tile_int8dyn(const int8_t* xq, const uint16_t* xs, const int8_t* wq, const uint16_t* ws,
                 const uint16_t* bias, uint16_t* y, int M, int N, int K, hipStream_t stream,
                 int splits);
bool use_tile(int path, int64_t M, int64_t N, int64_t K);

// gemm_sf.hip: the single-fetch prefill GEMM (128-row tiles, LDS-DMA, fixed-reducer split-K)
bool use_sf(int path, int64_t M, int64_t N, int64_t K, int64_t group_size);
int sf_int8dyn(const int8_t* xq, const uint16_t* xs, const int8_t* wq, const uint16_t* ws,
               const uint16_t* bias, uint16_t* y, int M, int N, int K, hipStream_t stream);
int sf_int4(const uint16_t* x, const uint32_t* packed, const uint16_t* sz, int lg,
            const uint16_t* bias, uint16_t* y, int M, int N, int K, hipStream_t stream,
            int epi = 0);

// gemm_i8_lds.hip: the int8 x int8 GEMM with both operands staged through LDS, for K a multiple
// of its k step; auto_mode: the routed shape rule, else the forced one (tao_tune_gemm_algo 2)
constexpr int kI8Step = 128;  // k bytes per step of gemm_i8_lds_kernel
int launch_i8_lds(const int8_t* xq, const uint16_t* xs, const int8_t* wq, const uint16_t* ws,
                  const uint16_t* bias, uint16_t* y, int M, int N, int K, bool auto_mode,
                  hipStream_t stream);

// gemm32_int4.hip: the int4 weight-only GEMM on 32x32x16 MFMAs; tbm / tsplits: a measured table
// entry's M tile and K slices (0: the kernel's own rule and tao_tune_gemm)
int launch_gemm32_int4(const uint16_t* x, const uint32_t* packed, const uint16_t* sz, int gshift,
                       const uint16_t* bias, uint16_t* y, int M, int N, int K,
                       hipStream_t stream, int tbm = 0, int tsplits = 0);

// gemm_mfma.hip: the skinny-M crossovers and the MFMA launches of the scaled-mm entries
// (fp8_dyn.hip, mx_fp8.hip, mx_fp4.hip, block_fp8.hip, int8_dyn.hip, w4a8.hip)
bool int4_linear_takes_gemv(int64_t M, int64_t N, int64_t K);
bool fp8dyn_takes_gemv(int64_t M, int64_t N, int64_t K);
bool mx_takes_gemv(int64_t M, int64_t N, int64_t K);
int fp8_scaled_mm_launch(const uint8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                         const uint16_t* bias, uint16_t* y, int M, int N, int K,
                         hipStream_t stream);
int mx_scaled_mm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq, const uint8_t* ws,
                        const uint16_t* bias, uint16_t* y, int M, int N, int K,
                        hipStream_t stream);
int mxfp4w_scaled_mm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq,
                            const uint8_t* ws, const uint16_t* bias, uint16_t* y, int M, int N,
                            int K, hipStream_t stream);
bool blockfp8_takes_gemv(int64_t M, int64_t N, int64_t K);
int blockfp8_scaled_mm_launch(const uint8_t* xq, const float* xs, const uint8_t* wq,
                              const float* ws, const uint16_t* bias, uint16_t* y, int M, int N,
                              int K, hipStream_t stream);
int int8_scaled_mm_launch(const int8_t* xq, const uint16_t* xs, const int8_t* wq,
                          const uint16_t* ws, const uint16_t* bias, uint16_t* y, int M, int N,
                          int K, hipStream_t stream);
int w4a8_scaled_mm_launch(const int8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                          const uint16_t* bias, uint16_t* y, int M, int N, int K,
                          hipStream_t stream);

}  // namespace tao
