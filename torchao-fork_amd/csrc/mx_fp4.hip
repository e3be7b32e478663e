// MXFP4 weights under MXFP8 activations (MXFPInferenceConfig, activation float8_e4m3fn, weight
// float4_e2m1fn_x2, block size 32): e2m1 codes, two per byte, with one E8M0 scale byte per 32-k
// block; the activation side is mx_fp8.hip's unchanged.
//
// Storage is the reference's (pack_uint4): element 2 j of a row sits in the HIGH nibble of byte j,
// element 2 j + 1 in the low nibble. The hardware converters put the LOW nibble first, so the
// kernels pair the codes explicitly (below); the stored bytes are never changed.
//
// Quantizer (replaces to_mx with elem_dtype float4_e2m1fn_x2,
// torchao/prototype/mx_formats/mx_tensor.py:133-326, FLOOR mode, and f32_to_f4_unpacked /
// pack_uint4 of kernel.py), per block of 32 consecutive elements of the last dimension:
//   byte    = (biased fp32 exponent field of amax|x|) - 2   (2 = F4_E2M1_MAX_POW2), floored at 0;
//             255 if the amax is NaN
//   divisor = the fp32 number with `byte` as its exponent field, at least 2^-126 (255: +inf)
//   code    = e2m1_rne(x / divisor), saturating at +-6; no clamp before the cast, so +-inf -> +-6
//             sign bit 3, magnitude codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6
// The divisor is a power of two between 2^-126 and 2^126, so x / divisor is the exact product with
// its reciprocal (2^(127 - max(byte, 1)) 2^127 as one exponent field 254 - max(byte, 1)); byte 255
// multiplies by 0: finite -> +-0, inf and NaN -> NaN, as dividing by +inf gives. The rounding is
// integer arithmetic on the fp32 pattern (mxfp4_code). A NaN pattern takes the rounding of the
// normal range, as the reference's arithmetic does (the default NaN gives magnitude code 3); an inf
// in a NaN block gives 0xB (inf / inf is the default NaN of the host the reference ran on, sign
// set). The whole block dequantizes to NaN either way.
//
// Product:
//   acc[m][n] = sum_b 2^(xs[m][b]-127) 2^(ws[n][b]-127) sum_{k in block b} e4m3(xq[m][k]) e2m1(wq[n][k])
//   y[m][n]   = bf16( acc[m][n] + fp32(bias[n]) )                      fp32 sums, one rounding
// with mx_fp8.hip's conventions: an all-zero token gives exactly bf16(bias); a scale byte 255 is
// NaN; no scale byte at or past K/32 is read.
//
//   1. tao_mxfp4_quantize_rows_bf16: mxfp4_quantize_rows_kernel, flat over blocks like
//      mx_quantize_rows_kernel (one thread per 16 elements, two 16-B loads, one 8-B store, the amax
//      met across the two lanes of a block; no LDS).
//   2. tao_mxfp4w_scaled_mm_bf16: M above the GEMV crossover (the MXFP8 rule, mx_takes_gemv): the
//      MxFp8Fp4 instance of the shared skinny-GEMM template (gemm_mfma.hip), e4m3 A and e2m1 B
//      inside v_mfma_scale_f32_16x16x128_f8f6f4; M at or below it: the decode GEMV (below).
//   3. tao_mxfp4w_dyn_linear_bf16 (one token): the e4m3fn block quantizer of mx_fp8.hip into LDS,
//      then the same GEMV, in one launch. Bit-identical to tao_mx_quantize_rows_bf16 -> 2.
//
// The decode GEMV of 2 and 3 is scaled_gemv_kernel (scaled_gemv.h) under the policy Mx4Fmt below,
// recorded as "mxw4_gemv_kernel": MXFP8's scales and token quantizer (MxScales, mx_block.h) and the
// kernel's kFp4Weights branch. A lane's 16-B weight chunk is one whole 32-k block (its x is 32 B of
// e4m3fn).
// Both code streams are decoded in hardware with scale 1.0 (exact): v_cvt_scalef32_pk_bf16_fp4
// turns byte j of a weight dword into the bf16 pair (low nibble, high nibble) = (w[2j+1], w[2j]);
// the x dword has its byte pairs swapped by one v_perm_b32 before v_cvt_scalef32_pk_bf16_fp8, so
// its pairs come out as (x[2j+1], x[2j]) too, and one v_dot2c_f32_bf16 takes each pair. (Where a
// lane holds more tokens than rows, MT = 4 and 8, the weight dwords have their nibbles exchanged
// instead, 3 instructions per dword, and x stays in k order.) The x pairs are converted once per
// token and reused by the wave's RPW rows. The block's fp32 partial
// sum is scaled by 2^(xs + ws - 254) with one v_ldexp_f32 and accumulated in fp32.
#include "mx_block.h"
#include "tao_gemm.h"

namespace tao {
namespace {

// ---- quantizer -------------------------------------------------------------------------------------
// the block's E8M0 byte from its amax pattern: exponent field - 2, floored at 0; NaN -> 255
__device__ __forceinline__ uint32_t mxfp4_scale_byte(uint32_t amax15) {
  const uint32_t e = amax15 >> 7;
  return amax15 > 0x7F80u ? 255u : (e > 2u ? e - 2u : 0u);
}
// 1 / divisor: exponent field 254 - max(byte, 1); byte 255 -> 0 (x / +inf)
__device__ __forceinline__ float mxfp4_recip(uint32_t byte) {
  const uint32_t b = byte > 1u ? byte : 1u;
  return __builtin_bit_cast(float, byte == 255u ? 0u : (254u - b) << 23);
}
// e2m1 code of the fp32 y, round to nearest even, saturating. Magnitudes at or above 6 (inf too)
// -> 7; below 1 the codes 0, 1, 2 lie 0.5 apart (ties 0.25 -> 0, 0.75 -> 2); in [1, 6) the code is
// the top of the pattern rebiased from 127 to 1 and rounded at bit 22, ties to the even code. A
// NaN pattern takes the last formula, its low byte kept.
__device__ __forceinline__ uint32_t mxfp4_code(float y) {
  const uint32_t bits = __builtin_bit_cast(uint32_t, y);
  const uint32_t a = bits & 0x7FFFFFFFu;
  const uint32_t norm = ((a - (126u << 23) + 0x1FFFFFu + ((a >> 22) & 1u)) >> 22) & 0xFFu;
  const uint32_t sub = a > 0x3E800000u ? (a >= 0x3F400000u ? 2u : 1u) : 0u;
  uint32_t c = a < 0x3F800000u ? sub : norm;
  c = (a >= 0x40C00000u && a <= 0x7F800000u) ? 7u : c;
  return ((bits >> 28) & 8u) | (c & 0xFu);
}
// the 8 bf16 of one 16-B piece -> 8 nibbles, element 2 j in the high nibble of byte j
__device__ __forceinline__ uint32_t mxfp4_quant8(const uint4 v, float recip, bool nan_block) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t o = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t h = (j & 1) ? d[j >> 1] >> 16 : d[j >> 1] & 0xFFFFu;
    const float x = __builtin_bit_cast(float, h << 16);
    uint32_t c = mxfp4_code(x * recip);
    if (nan_block && (h & 0x7FFFu) == 0x7F80u) c = 0xBu;  // inf / inf
    o |= c << (8 * (j >> 1) + ((j & 1) ? 0 : 4));
  }
  return o;
}

// One thread per 16 elements (half a block); lanes 2i, 2i + 1 share block i of the flat run.
__global__ __launch_bounds__(256) void mxfp4_quantize_rows_kernel(const uint4* __restrict__ x,
                                                                  uint2* __restrict__ q,
                                                                  uint8_t* __restrict__ scale,
                                                                  int64_t nchunk) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t cc = c < nchunk ? c : nchunk - 1;  // nchunk is even: a pair is whole or past the end
  const uint4 a = x[2 * cc], b = x[2 * cc + 1];
  uint32_t m = mx_amax8(b, mx_amax8(a, 0u));
  const uint32_t o = (uint32_t)__shfl_xor((int)m, 1);
  m = m > o ? m : o;
  const uint32_t byte = mxfp4_scale_byte(m);
  const float r = mxfp4_recip(byte);
  const uint32_t lo = mxfp4_quant8(a, r, byte == 255u), hi = mxfp4_quant8(b, r, byte == 255u);
  if (c < nchunk) {
    q[c] = make_uint2(lo, hi);
    if ((c & 1) == 0) scale[c >> 1] = (uint8_t)byte;
  }
}

// ---- GEMV ------------------------------------------------------------------------------------------
// scaled_gemv_kernel's policy: MxScales (mx_block.h) on e2m1 weight chunks, with the arithmetic of
// the kernel's kFp4Weights branch.
struct Mx4Fmt : MxScales {
  static constexpr const char* name = "mxw4_gemv_kernel";
  static constexpr const char* what = "mxfp4w";
  static constexpr int kChunkShift = 5;  // a 16-B weight chunk is one whole block
  static constexpr bool kFp4Weights = true;

  // the 16 e4m3fn codes of a 16-B piece -> 8 bf16 pairs in k order; SWAP: pair 2 j + h =
  // (x[4j+2h+1], x[4j+2h]), swapped within the pair, the order the e2m1 converter gives the
  // weight's stored bytes
  template <bool SWAP>
  static __device__ __forceinline__ void x16_bf16(const uint4 v, uint32_t* p) {
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t s = SWAP ? __builtin_amdgcn_perm(d[j], d[j], 0x02030001u) : d[j];  // 1 0 3 2
      p[2 * j] = e4m3_pair_bf16<false>(s);
      p[2 * j + 1] = e4m3_pair_bf16<true>(s);
    }
  }
  // byte B of a weight dword -> the bf16 pair (low nibble, high nibble) = (w[2B+1], w[2B]) of the
  // stored bytes
  template <int B>
  static __device__ __forceinline__ uint32_t w_pair(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, B));
  }
  // the nibbles of every byte exchanged: the converter then gives (w[2B], w[2B+1])
  static __device__ __forceinline__ uint32_t swap_nibbles(uint32_t v) {
    return ((v << 4) & 0xF0F0F0F0u) | ((v >> 4) & 0x0F0F0F0Fu);
  }
  static __device__ __forceinline__ uint4 swap_nibbles(const uint4 v) {
    return make_uint4(swap_nibbles(v.x), swap_nibbles(v.y), swap_nibbles(v.z), swap_nibbles(v.w));
  }
  // sum over the block's 32 k of x * w, from the 16 x pairs and the 16-B weight chunk (in the same
  // order within the pairs)
  static __device__ __forceinline__ float block_dot(const uint32_t (&xp)[16], const uint4 wv) {
    const uint32_t d[4] = {wv.x, wv.y, wv.z, wv.w};
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s = dot2_bf16(xp[4 * j + 0], w_pair<0>(d[j]), s);
      s = dot2_bf16(xp[4 * j + 1], w_pair<1>(d[j]), s);
      s = dot2_bf16(xp[4 * j + 2], w_pair<2>(d[j]), s);
      s = dot2_bf16(xp[4 * j + 3], w_pair<3>(d[j]), s);
    }
    return s;
  }
};

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_mxfp4_quantize_rows_bf16(const uint16_t* x, uint8_t* q, uint8_t* scale, int64_t M,
                                 int64_t K, void* stream) {
  const int rc = check_mx_sizes("mxfp4 quantize", M, 0, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(M < (1LL << 31) && K < (1LL << 31) && M * K < (1LL << 32),
                "mxfp4 quantize: size out of range (fewer than 2^32 elements)");
  if (M == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(q, 16, "q");
  const int64_t nchunk = M * K / 16;
  launch(mxfp4_quantize_rows_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint4*>(x), reinterpret_cast<uint2*>(q), scale,
         nchunk);
  return check_launch("mxfp4_quantize_rows_kernel");
}

int tao_mxfp4w_scaled_mm_bf16(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq,
                              const uint8_t* ws, const uint16_t* bias, uint16_t* y, int64_t M,
                              int64_t N, int64_t K, void* stream) {
  const int rc = check_mx_sizes("mxfp4w scaled mm", M, N, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31) &&
                    M * K < (1LL << 32) && N * K < (1LL << 32),
                "mxfp4w scaled mm: size out of range (fewer than 2^32 elements per operand)");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "mxfp4w scaled mm: K must be > 0");
  TAO_CHECK_ALIGN(xq, 16, "xq");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  if (K % 256 == 0) {  // the contract of tao_mx_scaled_mm_bf16: whole 8-B words of scale bytes
    TAO_CHECK_ALIGN(xs, 8, "xs");
    TAO_CHECK_ALIGN(ws, 8, "ws");
  }
  if (mx_takes_gemv(M, N, K)) {
    const Mx4Fmt::Args a{xq, xs, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                         (int)M, (int)N, (int)K, 0, 0, 0};
    return scaled_gemv<Mx4Fmt>(a, as_stream(stream));
  }
  return mxfp4w_scaled_mm_launch(xq, xs, wq, ws, bias, y, (int)M, (int)N, (int)K,
                                 as_stream(stream));
}

int tao_mxfp4w_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const uint8_t* ws,
                               const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                               void* stream) {
  const int rc = check_mx_sizes("mxfp4w dyn linear", M, N, K);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(M <= 1, "mxfp4w dyn linear: the fused path is one token (M <= 1, got %lld)",
                (long long)M);
  TAO_CHECK_ARG(K <= 65536, "mxfp4w dyn linear: K (%lld) must be <= 65536 (token in LDS)",
                (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31) && N * K < (1LL << 32),
                "mxfp4w dyn linear: size out of range (fewer than 2^32 weight elements)");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "mxfp4w dyn linear: K must be > 0");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  const Mx4Fmt::Args a{x, nullptr, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                       1, (int)N, (int)K, 0, 0, 0};
  return scaled_gemv_fused<Mx4Fmt>(a, as_stream(stream));
}

}  // extern "C"
