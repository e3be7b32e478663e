// float8 (OCP e4m3fn) per-row weight quantizer and dequantizer (Float8WeightOnlyConfig, version 1):
//
//   quantize (reference _choose_scale_float8 + _quantize_affine_float8,
//   quant_primitives.py:2175-2221, 2274-2293), per row:
//     s = float(bf16(amax|w| / 448))            a true (correctly rounded) fp32 division, rounded
//                                               to bf16 as the reference's division of the bf16
//                                               amax tensor is, then kept in fp32
//     q = e4m3fn_rne(clamp(float(w) / s, -448, 448))   again a true division, in fp32
//   No eps, as in the reference: an all-zero row gives s = 0 and 0 / 0 = NaN codes.
//
//   dequantize (reference _dequantize_affine_float8, quant_primitives.py:2298-2312):
//     w = bf16(float(q) * s)                    NaN codes give NaN
//
// Both are HBM-bound byte work: 16-B loads of the bf16 weight, one thread per 8 weights; the row
// reduction is a workgroup per row. hipcc keeps fp32 division correctly rounded by default
// (v_div_scale / v_div_fmas / v_div_fixup; the Makefile passes no fast-math flag), which the
// byte-for-byte match with the torch ops needs.
#include "fp8_quant_row.h"
#include "tao_reduce.h"

namespace tao {
namespace {

// One workgroup per row; K % 8 == 0. Pass 1: amax; pass 2 (the row again, from L2): quantise.
__global__ __launch_bounds__(256) void fp8_quantize_rows_kernel(const uint4* __restrict__ w,
                                                                uint2* __restrict__ q,
                                                                float* __restrict__ scale,
                                                                int K8) {
  __shared__ float red[4];
  const uint4* row = w + (size_t)blockIdx.x * K8;
  float amax = 0.f;
  for (int i = threadIdx.x; i < K8; i += 256) amax = fp8_amax8(row[i], amax);
  amax = wave_max(amax);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float s = fp8_row_scale(amax);
  if (threadIdx.x == 0) scale[blockIdx.x] = s;
  uint2* qr = q + (size_t)blockIdx.x * K8;
  for (int i = threadIdx.x; i < K8; i += 256) qr[i] = fp8_quant8(row[i], s);
}

// One thread per 8 codes: 8-B load, 16-B store.
__global__ __launch_bounds__(256) void fp8_dequant_kernel(const uint2* __restrict__ q,
                                                          const float* __restrict__ scale,
                                                          uint4* __restrict__ w, int64_t total8,
                                                          int K8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total8) return;
  const float s = scale[i / K8];
  const uint2 c = q[i];
  const uint32_t d[2] = {c.x, c.y};
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(d[j], 1.0f, false);
    const f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(d[j], 1.0f, true);
    o[2 * j] = (uint32_t)f32_to_bf16(lo[0] * s) | ((uint32_t)f32_to_bf16(lo[1] * s) << 16);
    o[2 * j + 1] = (uint32_t)f32_to_bf16(hi[0] * s) | ((uint32_t)f32_to_bf16(hi[1] * s) << 16);
  }
  w[i] = make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_fp8_quantize_rows_bf16(const uint16_t* w, uint8_t* q, float* scale, int64_t rows,
                               int64_t K, void* stream) {
  TAO_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && K >= 0 && K % 8 == 0 && K < (1LL << 31),
                "fp8 quantize: K (%lld) must be a multiple of 8", (long long)K);
  if (rows == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(q, 8, "q");
  TAO_CHECK_ALIGN(scale, 4, "scale");
  launch(fp8_quantize_rows_kernel, dim3((unsigned)rows), dim3(256), 0, as_stream(stream),
         reinterpret_cast<const uint4*>(w), reinterpret_cast<uint2*>(q), scale, (int)(K / 8));
  return check_launch("fp8_quantize_rows_kernel");
}

int tao_fp8_dequant_bf16(const uint8_t* q, const float* scale, uint16_t* w, int64_t N, int64_t K,
                         void* stream) {
  TAO_CHECK_ARG(N >= 0 && K >= 0 && K % 8 == 0 && K < (1LL << 31),
                "fp8 dequant: K (%lld) must be a multiple of 8", (long long)K);
  const int64_t total8 = N * (K / 8);
  if (total8 == 0) return TAO_OK;
  TAO_CHECK_ARG(total8 / 256 < (1LL << 31), "fp8 dequant: tensor too large");
  TAO_CHECK_ALIGN(q, 8, "q");
  TAO_CHECK_ALIGN(scale, 4, "scale");
  TAO_CHECK_ALIGN(w, 16, "w");
  launch(fp8_dequant_kernel, dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint2*>(q), scale,
         reinterpret_cast<uint4*>(w), total8, (int)(K / 8));
  return check_launch("fp8_dequant_kernel");
}

}  // extern "C"
