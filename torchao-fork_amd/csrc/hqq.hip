// HQQ (half-quadratic quantization) int4 weight quantizer: Int4WeightOnlyConfig(use_hqq=True)
// on a bf16 GPU weight, fused. Replaces the reference's _choose_qparams_and_quantize_affine_hqq
// + optimize_weights_proximal_legacy + _convert_to_affinequantized_format
// (quant_primitives.py:1901-2111: 20 iterations of ~15 eager ops over an fp32 copy of the weight
// with a device-to-host copy in each) and the layout's pack.
//
// The arithmetic is the reference's CPU arithmetic, fp32 throughout (on a GPU the reference
// iterates in fp16; that is the one deliberate deviation). Per group of g consecutive weights of
// a row, W the fp32 values of the bf16 weight:
//     scale = min((1 / (max - min)) * 15, 2e4)      zero = rint(-min * scale)
//     iteration i (1 / beta_i from the host, beta_0 = 10, beta *= 1.01, at most 20):
//       Wq = clamp(rint(W * scale + zero), 0, 15)   Wr = (Wq - zero) / scale      d = W - Wr
//       We = sign(d) * relu(|d| - (1 / beta_i) * |d|^-0.3)
//       zero = sum_group(Wq - (W - We) * scale) / g
//       e_i = mean over the whole tensor of |d|;  stop after iteration i if e_i >= min(e_0..e_{i-1})
//     q = clamp(rint(W * scale + zero), 0, 15)   s = bf16(1 / scale)
//     z = bf16((8 - zero) * (1 / scale))
//   so W ~= (q - 8) * s + z, the tinygemm form every int4 kernel reads. Every line is its own
//   fp32 rounding (no contraction), divisions are IEEE-correct.
//
// The stop is one decision for the whole tensor, made on the device in three launches on the
// caller's stream (no host copy, no synchronisation, graph-capturable):
//   1. hqq_errors_kernel: all 20 iterations of every group in registers; writes only the
//      per-workgroup sums of |d| of every iteration (double) into the caller's scratch.
//   2. hqq_stop_kernel (one workgroup): adds the partials of every iteration in a fixed order in
//      double, applies the stop rule, writes the number of iterations to run.
//   3. hqq_quantize_kernel: the same arithmetic for that many iterations, then the nibbles in the
//      row-stream dword order of int4_quantize_kernel and (s, z) into scales_and_zeros.
// Two reads of W, no per-group scratch, every sum in a fixed order: run-to-run bit-equal.
// Decomposition as int4_quantize_kernel (quantize.hip): 16-B loads, 8 weights per thread, g / 8
// lanes per group, lane exchanges for the group's min, max and sum; tail lanes load a clamped
// address (they form whole groups of their own past the end) and add nothing to the error.
// The group sum (added in double and rounded once, where the CPU adds in fp32 in its own order)
// and the device pow differ from the CPU's by an fp32 ulp or so, and the iteration is
// discontinuous, so a small share of groups lands on other codes than the plain-torch function
// (tests/test_gpu_hqq.py bounds it); the scale never differs.
#include <cmath>

#include "tao_common.h"
#include "tao_reduce.h"

// every product, sum and difference below is a separate fp32 rounding
#pragma clang fp contract(off)

namespace tao {
namespace {

constexpr int kHqqIters = 20;    // the reference's opt_params["iters"]
constexpr int kHqqThreads = 256;

// 1 / beta_i, and below which |d| the shrink is certainly zero: relu(|d| - |d|^-0.3 / beta) > 0
// needs |d|^1.3 > 1 / beta; at |d| < 0.9 beta^(-1 / 1.3) the subtrahend is above 1.14 |d|, far
// beyond any rounding of pow, so those elements skip the pow with the same bits (a wave whose
// lanes all skip takes no pow at all: LLM weights of a few hundredths never reach the bound).
struct HqqInvBeta {
  float v[kHqqIters];
  float skip[kHqqIters];
};

__device__ __forceinline__ void hqq_load(const uint4* __restrict__ w, int64_t i, int64_t total8,
                                         float (&f)[8]) {
  const uint4 v = w[i < total8 ? i : total8 - 1];  // clamped: tail lanes still exchange
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = bf16lo_to_f32(d[j]);
    f[2 * j + 1] = bf16hi_to_f32(d[j]);
  }
}

template <int LPG>
__device__ __forceinline__ void hqq_init(const float (&f)[8], int lane, float& scale, float& zero) {
  float mn = f[0], mx = f[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) {
    mn = fminf(mn, f[j]);
    mx = fmaxf(mx, f[j]);
  }
  mn = wave_bfly<1, LPG>(mn, lane, [](float a, float b) { return fminf(a, b); });
  mx = wave_bfly<1, LPG>(mx, lane, [](float a, float b) { return fmaxf(a, b); });
  // torch forms `15 / tensor` as reciprocal(tensor) * 15: two roundings, an ulp off the true
  // quotient in about a quarter of the groups (and then a different rint(-min * scale) on a tie)
  const float rcp = 1.0f / (mx - mn);
  scale = fminf(rcp * 15.0f, 2e4f);  // max == min: inf -> 2e4
  zero = rintf(-mn * scale);
}

__device__ __forceinline__ float hqq_code(float w, float scale, float zero) {
  const float t = w * scale;
  return fminf(fmaxf(rintf(t + zero), 0.f), 15.f);
}

// Sum of a double over the LPG lanes of a group (ascending butterfly, as wave_bfly).
template <int O, int END>
__device__ __forceinline__ double hqq_group_sum(double x, int lane) {
  x += __builtin_bit_cast(double, xor_partner<O>(__builtin_bit_cast(uint64_t, x), lane));
  if constexpr (O * 2 < END) return hqq_group_sum<O * 2, END>(x, lane);
  return x;
}

// One proximal iteration of a group: returns this thread's sum of |d| (measured with the zero
// from before the update) and replaces zero by the group's new one (in every lane of the group).
// The g fp32 terms of the mean are added in double (error far below an fp32 ulp of the sum for
// g <= 256 terms of 24 bits) and rounded to fp32 once: the correctly rounded sum in effect,
// whatever the order, so the new zero is within the CPU sum's own rounding error of the CPU's.
template <int LPG>
__device__ __forceinline__ float hqq_step(const float (&f)[8], int lane, float scale,
                                          float inv_beta, float skip, float& zero) {
  float err = 0.f;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float wq = hqq_code(f[j], scale, zero);
    const float wr = (wq - zero) / scale;
    const float d = f[j] - wr;
    const float a = fabsf(d);
    // sign(d) * relu(|d| - (1 / beta) |d|^(p - 1)); 0 below the bound (d == 0 included)
    float we = 0.f;
    if (a >= skip) we = copysignf(fmaxf(a - inv_beta * powf(a, -0.3f), 0.f), d);
    const float u = (f[j] - we) * scale;
    acc += (double)(wq - u);
    err += a;
  }
  acc = hqq_group_sum<1, LPG>(acc, lane);
  zero = (float)acc / (float)(8 * LPG);
  return err;
}

// Pass 1. partial[it * gridDim.x + blockIdx.x] = this workgroup's sum of |d| in iteration it.
template <int LPG>
__global__ __launch_bounds__(kHqqThreads) void hqq_errors_kernel(const uint4* __restrict__ w,
                                                                 double* __restrict__ partial,
                                                                 int64_t total8, HqqInvBeta ib) {
  __shared__ float red[kHqqIters][kHqqThreads / 64];
  const int64_t i = (int64_t)blockIdx.x * kHqqThreads + threadIdx.x;
  const int lane = lane_id();
  float f[8];
  hqq_load(w, i, total8, f);
  float scale, zero;
  hqq_init<LPG>(f, lane, scale, zero);
  const float live = i < total8 ? 1.f : 0.f;
  for (int it = 0; it < kHqqIters; ++it) {
    const float e = wave_sum(hqq_step<LPG>(f, lane, scale, ib.v[it], ib.skip[it], zero) * live);
    if (lane == 0) red[it][threadIdx.x >> 6] = e;
  }
  __syncthreads();
  if (threadIdx.x < kHqqIters) {
    const float* r = red[threadIdx.x];
    partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] =
        (((double)r[0] + (double)r[1]) + (double)r[2]) + (double)r[3];
  }
}

// Pass 2 (one workgroup). Sums nparts partials per iteration in a fixed order (thread t takes
// t, t + 256, ..., then a fixed tree over the threads), then the reference's stop rule on
// e_i = sum_i / numel: the loop runs iteration i and leaves after it when e_i >= best.
__global__ __launch_bounds__(kHqqThreads) void hqq_stop_kernel(const double* __restrict__ partial,
                                                               int nparts, double numel,
                                                               int* __restrict__ iters_run) {
  __shared__ double red[kHqqThreads];
  __shared__ double e[kHqqIters];
  for (int it = 0; it < kHqqIters; ++it) {
    const double* p = partial + (size_t)it * nparts;
    double s = 0.0;
    for (int j = threadIdx.x; j < nparts; j += kHqqThreads) s += p[j];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = kHqqThreads / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) e[it] = red[0] / numel;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double best = 1e4;
    int n = kHqqIters;
    for (int it = 0; it < kHqqIters; ++it) {
      if (e[it] < best) {
        best = e[it];
      } else {
        n = it + 1;
        break;
      }
    }
    *iters_run = n;
  }
}

// Pass 3. *iters_run updates of every group's zero, then the packed codes and (s, z).
template <int LPG>
__global__ __launch_bounds__(kHqqThreads) void hqq_quantize_kernel(
    const uint4* __restrict__ w, uint32_t* __restrict__ packed, uint32_t* __restrict__ sz,
    const int* __restrict__ iters_run, int64_t total8, HqqInvBeta ib) {
  const int64_t i = (int64_t)blockIdx.x * kHqqThreads + threadIdx.x;
  const int lane = lane_id();
  float f[8];
  hqq_load(w, i, total8, f);
  float scale, zero;
  hqq_init<LPG>(f, lane, scale, zero);
  int n = *iters_run;
  n = n < 0 ? 0 : (n > kHqqIters ? kHqqIters : n);
  for (int it = 0; it < n; ++it) (void)hqq_step<LPG>(f, lane, scale, ib.v[it], ib.skip[it], zero);
  uint32_t out = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    out |= (uint32_t)hqq_code(f[j], scale, zero) << ((j & 1) * 16 + (j >> 1) * 4);
  if (i < total8) {
    packed[i] = out;
    if ((i & (LPG - 1)) == 0) {
      const float inv = 1.0f / scale;
      const float z = (8.0f - zero) * inv;
      sz[i / LPG] = (uint32_t)f32_to_bf16(inv) | ((uint32_t)f32_to_bf16(z) << 16);
    }
  }
}

template <int LPG>
void hqq_launch(const uint4* w, uint32_t* packed, uint32_t* sz, int* iters_run, double* partial,
                int64_t total8, const HqqInvBeta& ib, hipStream_t st) {
  const unsigned nblocks = (unsigned)((total8 + kHqqThreads - 1) / kHqqThreads);
  launch(hqq_errors_kernel<LPG>, dim3(nblocks), dim3(kHqqThreads), 0, st, w, partial, total8, ib);
  launch(hqq_stop_kernel, dim3(1), dim3(kHqqThreads), 0, st, (const double*)partial, (int)nblocks,
         (double)total8 * 8.0, iters_run);
  launch(hqq_quantize_kernel<LPG>, dim3(nblocks), dim3(kHqqThreads), 0, st, w, packed, sz,
         (const int*)iters_run, total8, ib);
}

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int64_t tao_int4_hqq_scratch_bytes(int64_t rows, int64_t K) {
  if (rows <= 0 || K <= 0) return 0;
  const int64_t total8 = rows * (K / 8);
  return (total8 + kHqqThreads - 1) / kHqqThreads * kHqqIters * (int64_t)sizeof(double);
}

int tao_int4_hqq_quantize_bf16(const uint16_t* w, uint32_t* packed, uint16_t* scales_and_zeros,
                               int32_t* iters_run, void* scratch, int64_t rows, int64_t K,
                               int64_t group_size, void* stream) {
  TAO_CHECK_ARG(group_size == 32 || group_size == 64 || group_size == 128 || group_size == 256,
                "int4 hqq quantize: group_size must be 32, 64, 128 or 256 (got %lld)",
                (long long)group_size);
  TAO_CHECK_ARG(rows >= 0 && K >= 0 && K % group_size == 0,
                "int4 hqq quantize: K (%lld) %% group_size (%lld) != 0", (long long)K,
                (long long)group_size);
  TAO_CHECK_ARG(iters_run != nullptr, "int4 hqq quantize: iters_run is null");
  TAO_CHECK_ALIGN(iters_run, 4, "iters_run");
  const int64_t total8 = rows * (K / 8);
  TAO_CHECK_ARG(total8 / kHqqThreads < (1LL << 31) - 1, "int4 hqq quantize: tensor too large");
  hipStream_t st = as_stream(stream);
  if (total8 == 0) {  // the loop of an empty tensor never runs
    if (hipMemsetAsync(iters_run, 0, sizeof(int32_t), st) != hipSuccess)
      return set_error(TAO_ERR_HIP, "int4 hqq quantize: memset failed");
    return TAO_OK;
  }
  TAO_CHECK_ARG(scratch != nullptr, "int4 hqq quantize: scratch is null");
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(packed, 4, "packed");
  TAO_CHECK_ALIGN(scales_and_zeros, 4, "scales_and_zeros");
  TAO_CHECK_ALIGN(scratch, 8, "scratch");
  // 1 / beta_i in double as the reference's Python loop forms them, then one cast to fp32
  HqqInvBeta ib;
  double beta = 1e1;
  for (int it = 0; it < kHqqIters; ++it) {
    ib.v[it] = (float)(1.0 / beta);
    ib.skip[it] = (float)(0.9 * pow(1.0 / beta, 1.0 / 1.3));
    beta *= 1.01;
  }
  const uint4* wv = reinterpret_cast<const uint4*>(w);
  uint32_t* szv = reinterpret_cast<uint32_t*>(scales_and_zeros);
  double* part = reinterpret_cast<double*>(scratch);
  switch (group_size) {
    case 32: hqq_launch<4>(wv, packed, szv, iters_run, part, total8, ib, st); break;
    case 64: hqq_launch<8>(wv, packed, szv, iters_run, part, total8, ib, st); break;
    case 128: hqq_launch<16>(wv, packed, szv, iters_run, part, total8, ib, st); break;
    default: hqq_launch<32>(wv, packed, szv, iters_run, part, total8, ib, st); break;
  }
  return check_launch("hqq_quantize_kernel");
}

}  // extern "C"
