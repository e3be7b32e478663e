// float8 (OCP e4m3fn) per-row-scaled weight-only linear, skinny-M (decode) path:
//   y[m][n] = bf16( (sum_k x[m][k] * f(w[n][k])) * scale[n] ) (+ bias[n] -> bf16)
// with f the exact e4m3fn -> real decode, the sum and the scale product in fp32.
// Replaces F.linear(x, weight.dequantize(), bias) at torchao/dtypes/floatx/float8_layout.py:391-396,
// which writes a bf16 copy of W (2 B per weight) on every call and reads it back in a library
// GEMM; here the 1-B codes are read once. The scale is applied once per output instead of once
// per weight.
//
// Same decomposition as int8_gemv.hip: a slice is 1024 k of one row = 64 lanes x 16 B; a wave
// owns RPW rows; Wk waves split K inside a workgroup; LDS combines the waves.
// Per lane: one v_cvt_scalef32_pk_bf16_fp8 (scale 1.0: exact, all finite e4m3fn values are bf16
// numbers) turns two codes into a bf16 pair, one v_dot2c_f32_bf16 multiplies it with the x pair
// as loaded: 1.0 VALU per weight and no x conversion (v_cvt_pk_f32_fp8 + v_fma_f32 would be 1.5
// plus the bf16 -> f32 shifts of x). No bias trick is needed: the codes decode signed.
#include "tao_common.h"
#include "tao_reduce.h"

namespace tao {

namespace {

// codes (2 sel, 2 sel + 1) of a dword -> bf16 pair, exact; NaN codes (0x7F, 0xFF) stay NaN
template <bool HI>
__device__ __forceinline__ uint32_t fp8_pair_bf16(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
}

template <int MT, int RPW>
__global__ __launch_bounds__(512) void fp8wo_gemv_kernel(
    const uint16_t* __restrict__ x, const uint4* __restrict__ w, const float* __restrict__ scale,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int M, int N, int K, int Wk,
    int G, int S) {
  constexpr int V = RPW * MT;
  extern __shared__ float red[];  // [G][Wk][V]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % Wk;
  const int rg = wave / Wk;
  const int row0 = (blockIdx.x * G + rg) * RPW;
  const int nchunk = K >> 4;  // 16-k (16-B) chunks per row

  float acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

  for (int s = wk; s < S; s += Wk) {
    const int c = s * 64 + lane;
    const bool cval = c < nchunk;
    const int cc = cval ? c : nchunk - 1;

    uint4 wv[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const int nn = n < N ? n : N - 1;
      wv[r] = ld_nt_u4(w + (size_t)nn * nchunk + cc);
    }
    // A lane past the row's last chunk loaded a clamped (valid) address and skips the math: its
    // codes may be NaN (an all-zero row quantizes to NaN codes), which 0 * w would not cancel.
    if (cval) {
      uint32_t wp[RPW][8];  // bf16 pairs (k, k + 1), in x's dword order
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const uint32_t wd[4] = {wv[r].x, wv[r].y, wv[r].z, wv[r].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          wp[r][2 * j] = fp8_pair_bf16<false>(wd[j]);
          wp[r][2 * j + 1] = fp8_pair_bf16<true>(wd[j]);
        }
      }
      // x is streamed one row of M at a time: 8 live dwords whatever M is.
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int mm = m < M ? m : M - 1;
        const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)mm * K + (size_t)cc * 16);
        const uint4 a = xp[0], b = xp[1];
        const uint32_t d8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          float d = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) d = dot2_bf16(d8[i], wp[r][i], d);
          acc[r][m] += d;
        }
      }
    }
  }

  float v[V];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) v[r * MT + m] = acc[r][m];
  wave_reduce_scatter<V>(v, lane);

  constexpr int T = Log2<V>::value;
  const bool owner = (lane & ((64 >> T) - 1)) == 0;
  const int idx = lane >> (6 - T);
  float total = v[0];
  bool writer = owner;
  int widx = idx;
  if (Wk > 1) {
    if (owner) red[(rg * Wk + wk) * V + idx] = v[0];
    __syncthreads();
    writer = (wk == 0) && (lane < V);
    widx = lane;
    if (writer) {
      total = 0.f;
      for (int kk = 0; kk < Wk; ++kk) total += red[(rg * Wk + kk) * V + widx];
    }
  }
  if (writer) {
    const int r = widx / MT, m = widx % MT;
    const int n = row0 + r;
    if (n < N && m < M) {
      // the fp32 sum times the fp32 scale, rounded once; then + bias, rounded again
      float o = round_bf16(total * scale[n]);
      if (bias != nullptr) o = round_bf16(o + bf16_to_f32(bias[n]));
      y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

template <int MT, int RPW>
int launch_gemv(const uint16_t* x, const uint8_t* w, const float* scale, const uint16_t* bias,
                uint16_t* y, int M, int N, int K, hipStream_t stream, int wk = 0, int g = 0) {
  const int nchunk = K / 16;
  const int S = (nchunk + 63) / 64;
  int Wk = S < 8 ? S : 8;
  int G = (8 / Wk) > 0 ? 8 / Wk : 1;
  if (wk > 0) Wk = wk < S ? wk : S;
  if (g > 0) G = g;
  while (G > 1 && Wk * G > 8) G >>= 1;  // __launch_bounds__(512)
  const int rows_per_wg = G * RPW;
  const int grid = (N + rows_per_wg - 1) / rows_per_wg;
  const size_t lds = (size_t)G * Wk * RPW * MT * sizeof(float);
  launch((fp8wo_gemv_kernel<MT, RPW>), dim3(grid), dim3(64 * Wk * G), lds, stream, x,
         reinterpret_cast<const uint4*>(w), scale, bias, y, M, N, K, Wk, G, S);
  return check_launch("fp8wo_gemv_kernel");
}

}  // namespace

int fp8wo_gemv(const uint16_t* x, const uint8_t* w, const float* scale, const uint16_t* bias,
               uint16_t* y, int64_t M, int64_t N, int64_t K, hipStream_t stream) {
  if (M <= 1) {
    // the int8 GEMV's M == 1 shape (same bytes, same decomposition: int8_gemv.hip): 4 rows per
    // wave, Wk = min(S, 8), one row group per workgroup; tao_tune_fp8_gemv overrides
    const int rpw = tuning().fp8_rpw, wk = tuning().fp8_wk;
    const int tg = tuning().fp8_g, g = tg > 0 ? tg : 1;
    if (rpw == 2)
      return launch_gemv<1, 2>(x, w, scale, bias, y, (int)M, (int)N, (int)K, stream, wk, g);
    if (rpw == 8)
      return launch_gemv<1, 8>(x, w, scale, bias, y, (int)M, (int)N, (int)K, stream, wk, g);
    return launch_gemv<1, 4>(x, w, scale, bias, y, (int)M, (int)N, (int)K, stream, wk, g);
  }
  if (M <= 2) return launch_gemv<2, 4>(x, w, scale, bias, y, (int)M, (int)N, (int)K, stream);
  if (M <= 4) return launch_gemv<4, 2>(x, w, scale, bias, y, (int)M, (int)N, (int)K, stream);
  return launch_gemv<8, 1>(x, w, scale, bias, y, (int)M, (int)N, (int)K, stream);
}

}  // namespace tao

extern "C" int tao_tune_fp8_gemv(int rows_per_wave, int waves_k, int row_groups) {
  TAO_CHECK_ARG(rows_per_wave == 0 || rows_per_wave == 2 || rows_per_wave == 4 ||
                    rows_per_wave == 8,
                "tune: fp8 rows_per_wave must be 0, 2, 4 or 8");
  TAO_CHECK_ARG(waves_k >= 0 && waves_k <= 8, "tune: fp8 waves_k must be in [0, 8]");
  TAO_CHECK_ARG(row_groups >= 0 && row_groups <= 8, "tune: fp8 row_groups must be in [0, 8]");
  TAO_CHECK_ARG(waves_k * row_groups <= 8, "tune: fp8 waves_k * row_groups must be <= 8");
  tao::tuning().fp8_rpw = rows_per_wave;
  tao::tuning().fp8_wk = waves_k;
  tao::tuning().fp8_g = row_groups;
  return TAO_OK;
}
