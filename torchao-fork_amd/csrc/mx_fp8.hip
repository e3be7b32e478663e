// MXFP8 inference linear (MXFPInferenceConfig, activation and weight float8_e4m3fn, block size 32):
// 32-element blocks along K, each with one E8M0 (power-of-two) scale byte; the native matrix
// format of gfx950.
//
// Quantizer (replaces to_mx, torchao/prototype/mx_formats/mx_tensor.py:133-326, FLOOR mode), per
// block of 32 consecutive elements of the last dimension, from float32(x):
//   e       = (biased fp32 exponent field of amax|x|) - 127 - 8       8 = F8E4M3_MAX_POW2
//             clamped to [-127, 128]
//   byte    = e + 127; 255 if the amax is NaN
//   divisor = the fp32 number with `byte` as its exponent field, clamped from below to 2^-126
//             (an all-zero or all-subnormal block stores byte 0 and divides by 2^-126; byte 255 is
//             +inf as an exponent field: finite x -> 0, NaN and inf -> NaN)
//   code    = e4m3fn_rne(clamp(x / divisor, -448, 448))                NaN stays NaN
// The amax is taken on the 15-bit magnitude patterns of the bf16 inputs (integer order is float
// order there, and a NaN pattern is above every number, so a NaN anywhere in the block wins, as
// torch.amax has it); the exponent field of the bf16 pattern is that of float32(x). The division
// is a true fp32 division (fp8_quant_row.h's fp8_quant8, the conversion of fp8_convert.h): the
// bytes equal the reference's, scale bytes and codes alike.
//
// Product:
//   acc[m][n] = sum_b 2^(xs[m][b]-127) * 2^(ws[n][b]-127) * sum_{k in block b} f(xq[m][k]) * f(wq[n][k])
//   y[m][n]   = bf16( acc[m][n] + fp32(bias[n]) )                      fp32 sums, one rounding
// An all-zero token has scale bytes 0 and codes 0: its output row is exactly bf16(bias), or 0
// without bias (the per-row float8 path gives NaN there). A scale byte 255 is NaN, whatever the
// codes. No scale byte at or past K/32 is read.
//
//   1. tao_mx_quantize_rows_bf16: mx_quantize_rows_kernel. One thread per 16 elements (two 16-B
//      loads, one 16-B store), the block's amax met across the two lanes that share it; no LDS.
//      [M][K] with K % 32 == 0 is one flat run of blocks, so the kernel is one-dimensional.
//   2. tao_mx_scaled_mm_bf16: replaces the torch._scaled_mm call of _addmm_mx_dispatch
//      (torchao/prototype/mx_formats/mx_ops.py). M above the GEMV crossover: the MxFp8 instance
//      of the shared skinny-GEMM template (gemm_mfma.hip), the scale bytes applied inside
//      v_mfma_scale_f32_16x16x128_f8f6f4; M at or below it: the decode GEMV (below).
//   3. tao_mx_dyn_linear_bf16 (one token): 1 and 2 in one launch. Every workgroup issues its first
//      weight slice, quantises the token into LDS (codes and scale bytes, the arithmetic of 1: a
//      block's scale depends on that block alone, so there is no row-wide reduction and no barrier
//      before the codes are written), then runs the GEMV on the codes. Bit-identical to 1 -> 2.
//
// The decode GEMV of 2 and 3 is scaled_gemv_kernel (scaled_gemv.h: decomposition, hardware decode
// of both code streams, skipped tail lanes, the fused prologue's order of loads) under the policy
// MxFmt below, recorded as "mx_gemv_kernel". This format's own part (MxScales, mx_block.h): a
// lane's 16-B chunk is half a block; its fp32 partial sum is scaled by the block's
// 2^(xs + ws - 254) with one v_ldexp_f32 (exact short of fp32 overflow / underflow, so scaling the
// two halves of a block apart equals scaling their sum), then accumulated in fp32.
#include "mx_block.h"
#include "tao_gemm.h"

namespace tao {
namespace {

// ---- the quantizer (its arithmetic, shared with the one-token prologues: mx_block.h) -----------
// One thread per 16 elements (half a block); lanes 2i, 2i + 1 share block i of the flat run.
__global__ __launch_bounds__(256) void mx_quantize_rows_kernel(const uint4* __restrict__ x,
                                                               uint4* __restrict__ q,
                                                               uint8_t* __restrict__ scale,
                                                               int64_t nchunk) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t cc = c < nchunk ? c : nchunk - 1;  // nchunk is even: a pair is whole or past the end
  const uint4 a = x[2 * cc], b = x[2 * cc + 1];
  uint32_t m = mx_amax8(b, mx_amax8(a, 0u));
  const uint32_t o = (uint32_t)__shfl_xor((int)m, 1);
  m = m > o ? m : o;
  const uint32_t byte = mx_scale_byte(m);
  const float div = mx_divisor(byte);
  const uint2 lo = fp8_quant8(a, div), hi = fp8_quant8(b, div);
  if (c < nchunk) {
    q[c] = make_uint4(lo.x, lo.y, hi.x, hi.y);
    if ((c & 1) == 0) scale[c >> 1] = (uint8_t)byte;
  }
}

// ---- GEMV ------------------------------------------------------------------------------------------
// scaled_gemv_kernel's policy: MxScales (mx_block.h) on e4m3fn weight chunks. A lane's 16-B chunk
// is half a block.
struct MxFmt : MxScales {
  static constexpr const char* name = "mx_gemv_kernel";
  static constexpr const char* what = "mx";
  static constexpr int kChunkShift = 4;
  static constexpr bool kFp4Weights = false;
};

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_mx_quantize_rows_bf16(const uint16_t* x, uint8_t* q, uint8_t* scale, int64_t M, int64_t K,
                              void* stream) {
  const int rc = check_mx_sizes("mx quantize", M, 0, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(M < (1LL << 31) && K < (1LL << 31) && M * K < (1LL << 32),
                "mx quantize: size out of range (codes below 4 GiB)");
  if (M == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(q, 16, "q");
  const int64_t nchunk = M * K / 16;
  launch(mx_quantize_rows_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint4*>(x), reinterpret_cast<uint4*>(q), scale,
         nchunk);
  return check_launch("mx_quantize_rows_kernel");
}

int tao_mx_scaled_mm_bf16(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq,
                          const uint8_t* ws, const uint16_t* bias, uint16_t* y, int64_t M,
                          int64_t N, int64_t K, void* stream) {
  const int rc = check_mx_sizes("mx scaled mm", M, N, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31) &&
                    M * K < (1LL << 32) && N * K < (1LL << 32),
                "mx scaled mm: size out of range (operands below 4 GiB)");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "mx scaled mm: K must be > 0");
  TAO_CHECK_ALIGN(xq, 16, "xq");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  if (K % 256 == 0) {  // whole 8-B words of scale bytes per 256-k step (the MFMA route's loads)
    TAO_CHECK_ALIGN(xs, 8, "xs");
    TAO_CHECK_ALIGN(ws, 8, "ws");
  }
  if (mx_takes_gemv(M, N, K)) {
    const MxFmt::Args a{xq, xs, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                        (int)M, (int)N, (int)K, 0, 0, 0};
    return scaled_gemv<MxFmt>(a, as_stream(stream));
  }
  return mx_scaled_mm_launch(xq, xs, wq, ws, bias, y, (int)M, (int)N, (int)K, as_stream(stream));
}

int tao_mx_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const uint8_t* ws,
                           const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                           void* stream) {
  const int rc = check_mx_sizes("mx dyn linear", M, N, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(M <= 1, "mx dyn linear: the fused path is one token (M <= 1, got %lld)",
                (long long)M);
  TAO_CHECK_ARG(K <= 65536, "mx dyn linear: K (%lld) must be <= 65536 (token in LDS)",
                (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31) && N * K < (1LL << 32),
                "mx dyn linear: size out of range (weight below 4 GiB)");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "mx dyn linear: K must be > 0");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  const MxFmt::Args a{x, nullptr, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                      1, (int)N, (int)K, 0, 0, 0};
  return scaled_gemv_fused<MxFmt>(a, as_stream(stream));
}

}  // extern "C"
