// Blockwise float8 inference linear (torchao.prototype.blockwise_fp8_inference, the DeepSeek-V3
// recipe): e4m3fn codes, one fp32 scale per 1 x 128 block of the activation ([M][K/128]) and one
// per 128 x 128 block of the weight ([ceil(N/128)][K/128]). K % 128 == 0, any N.
//
// Quantizer (replaces fp8_blockwise_act_quant / fp8_blockwise_weight_quant,
// blockwise_quantization.py), per block, from float32(x):
//   amax = max |x|, a NaN element ignored (fmaxf); 0 if the block holds no number
//   s    = amax / 448            correctly rounded fp32 division, a subnormal quotient kept
//   code = e4m3fn_rne(x / s)     correctly rounded fp32 division, no clamp; NaN stays NaN
//          e4m3fn_rne(x)         where amax == 0 (x is a signed zero or NaN)
// An infinite element makes s = inf: the block's finite elements become zero codes, the infinite
// one NaN. An all-zero block stores zero codes and scale 0 (the reference stores NaN codes there).
// A weight block of a ragged last tile row takes its amax over the rows that exist.
//
// Product, P[m][n][b] the fp32 dot product of the 128 code pairs of block b:
//   y[m][n] = bf16( sum_b P[m][n][b] * (xs[m][b] * ws[n/128][b]) + fp32(bias[n]) )
// in fp32 with one rounding to bf16. The factor f = xs * ws is rounded to fp32 first and each
// term enters the sum by one fused multiply-add, acc = fma(P, f, acc); the bias is a separate add.
// Order of the sum, fixed per route:
//   * GEMV (M up to the crossover): lane l of a wave holds the 16 codes l of each 1024-k slice
//     (1/8 of a block), its fp32 dot product of them is the P of the fma above, slices in
//     ascending order per wave; then the lanes, waves along K and row groups are summed by
//     tao_gemv.h's shared tail in its fixed order.
//   * MFMA (gemm_mfma_kernel, policy BlockFp8): P is one v_mfma_scale_f32_16x16x128_f8f6f4 into a
//     zero accumulator (unit E8M0 bytes), blocks in ascending order per k-group, then the
//     k-groups and split-K slices in their fixed orders.
// An all-zero token has zero codes and zero scales: its row is exactly bf16(bias), 0 without bias.
// No scale past either array is read: the weight's scale row is clamped to ceil(N/128) - 1, block
// indices to K/128 - 1, and the second MFMA of a K % 256 == 128 tail gets zero codes and factor 0.
//
//   1. tao_blockfp8_quantize_act_bf16: blockfp8_quantize_act_kernel, 16 lanes x 8 bf16 per block.
//   2. tao_blockfp8_quantize_weight_bf16: blockfp8_quantize_weight_kernel, one workgroup per
//      128 x 128 tile.
//   3. tao_blockfp8_dequant_weight: blockfp8_dequant_weight_kernel, float(code) * s in fp32, stored
//      as fp32 or rounded once to bf16.
//   4. tao_blockfp8_scaled_mm_bf16: up to the crossover scaled_gemv_kernel (scaled_gemv.h) under
//      the policy BlockFp8Fmt below, recorded as "blockfp8_gemv_kernel"; the BlockFp8 instance of
//      gemm_mfma_kernel above it.
//   5. tao_blockfp8_dyn_linear_bf16 (one token): 1 and 4 in one launch; the token is quantised per
//      block into LDS (a block's scale depends on that block alone: no row-wide reduction), then the
//      GEMV runs on the codes. Bit-identical to 1 -> 4.
#include "blockfp8_block.h"
#include "scaled_gemv.h"
#include "tao_gemm.h"

namespace tao {
namespace {

// ---- quantizers --------------------------------------------------------------------------------
// One thread per 16-B piece (8 bf16); lanes 16 i .. 16 i + 15 share block i of the flat run of
// blocks ([M][K], K % 128 == 0). npiece % 16 == 0: a group of 16 is whole or past the end.
__global__ __launch_bounds__(256) void blockfp8_quantize_act_kernel(const uint4* __restrict__ x,
                                                                    uint2* __restrict__ q,
                                                                    float* __restrict__ scale,
                                                                    int64_t npiece) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t cc = c < npiece ? c : npiece - 1;
  const uint4 v = x[cc];
  const float s = blockfp8_scale(blockfp8_amax16(fp8_amax8(v, 0.f)));
  const uint2 o = blockfp8_quant8(v, s);
  if (c < npiece) {
    q[c] = o;
    if ((c & 15) == 0) scale[c >> 4] = s;
  }
}

// One 256-thread workgroup per 128 x 128 tile (blockIdx.x: k block, blockIdx.y: row block): thread
// t holds the 16-B piece t % 16 of rows t / 16 + 16 i, i < 8. Rows at or past N are loaded clamped
// and neither counted in the amax nor stored.
__global__ __launch_bounds__(256) void blockfp8_quantize_weight_kernel(
    const uint4* __restrict__ w, uint2* __restrict__ q, float* __restrict__ scale, int N, int K) {
  __shared__ float red[4];
  const int t = threadIdx.x;
  const int kb = blockIdx.x, nb = blockIdx.y;
  const int npr = K >> 3;  // 16-B pieces per row
  const int pc = kb * 16 + (t & 15);
  uint4 v[8];
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = nb * 128 + (t >> 4) + 16 * i;
    v[i] = w[(size_t)(n < N ? n : N - 1) * npr + pc];
    const float mi = fp8_amax8(v[i], 0.f);
    m = fmaxf(m, n < N ? mi : 0.f);
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));
  if ((t & 63) == 0) red[t >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float s = blockfp8_scale(m);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = nb * 128 + (t >> 4) + 16 * i;
    const uint2 o = blockfp8_quant8(v[i], s);
    if (n < N) q[(size_t)n * npr + pc] = o;
  }
  if (t == 0) scale[(size_t)nb * gridDim.x + kb] = s;
}

// One thread per 16 codes of the flat [N][K] run: out = float(code) * s[n / 128][k / 128].
template <bool BF16>
__global__ __launch_bounds__(256) void blockfp8_dequant_weight_kernel(
    const uint4* __restrict__ q, const float* __restrict__ scale, void* __restrict__ out,
    int64_t nchunk, int cpr) {  // cpr: 16-B chunks per row (K / 16)
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= nchunk) return;
  const int64_t n = c / cpr;
  const int kc = (int)(c - n * cpr);
  const float s = scale[(n >> 7) * (cpr >> 3) + (kc >> 3)];
  uint32_t p[8];
  e4m3_chunk_bf16(q[c], p);
  float f[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    f[2 * i] = bf16lo_to_f32(p[i]) * s;
    f[2 * i + 1] = bf16hi_to_f32(p[i]) * s;
  }
  if constexpr (BF16) {
    uint32_t o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      o[i] = (uint32_t)f32_to_bf16(f[2 * i]) | ((uint32_t)f32_to_bf16(f[2 * i + 1]) << 16);
    uint4* dst = reinterpret_cast<uint4*>(out) + 2 * c;
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
  } else {
    float4* dst = reinterpret_cast<float4*>(out) + 4 * c;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dst[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
  }
}

// ---- GEMV ------------------------------------------------------------------------------------------
// scaled_gemv_kernel's policy: fp32 scales per 128-k block, the weight's shared by 128 rows. A
// lane's 16-B chunk is an eighth of a block; its fp32 partial sum enters the accumulator as
// fma(partial, xs * ws, acc). The fused launch quantises the token per block (sixteen consecutive
// threads hold one; the arithmetic of blockfp8_quantize_act_kernel).
struct BlockFp8Fmt {
  using Args = ScaledGemvArgs<float>;  // xs [M][K/128], ws [ceil(N/128)][K/128]
  using Scale = float;
  static constexpr const char* name = "blockfp8_gemv_kernel";
  static constexpr const char* what = "blockfp8";
  static constexpr int kChunkShift = 4, kBlockShift = 7;
  static constexpr bool kRowScales = false, kFp4Weights = false;
  // row N - 1 lies in scale row ceil(N/128) - 1: a clamped row reads inside the array
  static __device__ __forceinline__ size_t scale_row(size_t nn) { return nn >> 7; }
  static __device__ __forceinline__ float token_scale(const uint4 xv) {
    return blockfp8_scale(blockfp8_amax16(fp8_amax8(xv, 0.f)));
  }
  static __device__ __forceinline__ uint2 token_codes(const uint4 xv, float s) {
    return blockfp8_quant8(xv, s);
  }
  static __device__ __forceinline__ float add(float d, float xf, float wf, float acc) {
    return __builtin_fmaf(d, xf * wf, acc);
  }
};

int check_sizes(const char* what, int64_t M, int64_t N, int64_t K) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "%s: negative size", what);
  TAO_CHECK_ARG(K % 128 == 0, "%s: K (%lld) must be a multiple of 128 (the block size)", what,
                (long long)K);
  return TAO_OK;
}

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_blockfp8_quantize_act_bf16(const uint16_t* x, uint8_t* q, float* scale, int64_t M,
                                   int64_t K, void* stream) {
  const int rc = check_sizes("blockfp8 quantize act", M, 0, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(M < (1LL << 31) && K < (1LL << 31) && M * K < (1LL << 32),
                "blockfp8 quantize act: size out of range (codes below 4 GiB)");
  if (M == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(q, 8, "q");
  TAO_CHECK_ALIGN(scale, 4, "scale");
  const int64_t npiece = M * K / 8;
  launch(blockfp8_quantize_act_kernel, dim3((unsigned)((npiece + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint4*>(x), reinterpret_cast<uint2*>(q), scale,
         npiece);
  return check_launch("blockfp8_quantize_act_kernel");
}

int tao_blockfp8_quantize_weight_bf16(const uint16_t* w, uint8_t* q, float* scale, int64_t N,
                                      int64_t K, void* stream) {
  const int rc = check_sizes("blockfp8 quantize weight", 0, N, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(N < (1LL << 31) - 128 && K < (1LL << 31) && N * K < (1LL << 32) &&
                    (N + 127) / 128 < 65536,
                "blockfp8 quantize weight: size out of range (codes below 4 GiB, N below 8 Mi)");
  if (N == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(q, 8, "q");
  TAO_CHECK_ALIGN(scale, 4, "scale");
  launch(blockfp8_quantize_weight_kernel, dim3((unsigned)(K / 128), (unsigned)((N + 127) / 128)),
         dim3(256), 0, as_stream(stream), reinterpret_cast<const uint4*>(w),
         reinterpret_cast<uint2*>(q), scale, (int)N, (int)K);
  return check_launch("blockfp8_quantize_weight_kernel");
}

int tao_blockfp8_dequant_weight(const uint8_t* q, const float* scale, void* out, int64_t N,
                                int64_t K, int out_bf16, void* stream) {
  const int rc = check_sizes("blockfp8 dequant weight", 0, N, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1,
                "blockfp8 dequant weight: out_bf16 must be 0 (fp32) or 1 (bf16)");
  TAO_CHECK_ARG(N < (1LL << 31) && K < (1LL << 31) && N * K < (1LL << 32),
                "blockfp8 dequant weight: size out of range (codes below 4 GiB)");
  if (N == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(q, 16, "q");
  TAO_CHECK_ALIGN(scale, 4, "scale");
  TAO_CHECK_ALIGN(out, 16, "out");
  const int64_t nchunk = N * K / 16;
  const dim3 grid((unsigned)((nchunk + 255) / 256));
  if (out_bf16)
    launch(blockfp8_dequant_weight_kernel<true>, grid, dim3(256), 0, as_stream(stream),
           reinterpret_cast<const uint4*>(q), scale, out, nchunk, (int)(K / 16));
  else
    launch(blockfp8_dequant_weight_kernel<false>, grid, dim3(256), 0, as_stream(stream),
           reinterpret_cast<const uint4*>(q), scale, out, nchunk, (int)(K / 16));
  return check_launch("blockfp8_dequant_weight_kernel");
}

int tao_blockfp8_scaled_mm_bf16(const uint8_t* xq, const float* xs, const uint8_t* wq,
                                const float* ws, const uint16_t* bias, uint16_t* y, int64_t M,
                                int64_t N, int64_t K, void* stream) {
  const int rc = check_sizes("blockfp8 scaled mm", M, N, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(M < (1LL << 31) && N < (1LL << 31) - 128 && K < (1LL << 31) &&
                    M * K < (1LL << 32) && N * K < (1LL << 32),
                "blockfp8 scaled mm: size out of range (operands below 4 GiB)");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "blockfp8 scaled mm: K must be > 0");
  TAO_CHECK_ALIGN(xq, 16, "xq");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  TAO_CHECK_ALIGN(xs, 4, "xs");
  TAO_CHECK_ALIGN(ws, 4, "ws");
  if (blockfp8_takes_gemv(M, N, K)) {
    const BlockFp8Fmt::Args a{xq, xs, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                              (int)M, (int)N, (int)K, 0, 0, 0};
    return scaled_gemv<BlockFp8Fmt>(a, as_stream(stream));
  }
  return blockfp8_scaled_mm_launch(xq, xs, wq, ws, bias, y, (int)M, (int)N, (int)K,
                                   as_stream(stream));
}

int tao_blockfp8_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const float* ws,
                                 const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                                 int64_t K, void* stream) {
  const int rc = check_sizes("blockfp8 dyn linear", M, N, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(M <= 1, "blockfp8 dyn linear: the fused path is one token (M <= 1, got %lld)",
                (long long)M);
  TAO_CHECK_ARG(K <= 65536, "blockfp8 dyn linear: K (%lld) must be <= 65536 (token in LDS)",
                (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31) - 128 && N * K < (1LL << 32),
                "blockfp8 dyn linear: size out of range (weight below 4 GiB)");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "blockfp8 dyn linear: K must be > 0");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  TAO_CHECK_ALIGN(ws, 4, "ws");
  const BlockFp8Fmt::Args a{x, nullptr, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                            1, (int)N, (int)K, 0, 0, 0};
  return scaled_gemv_fused<BlockFp8Fmt>(a, as_stream(stream));
}

}  // extern "C"
