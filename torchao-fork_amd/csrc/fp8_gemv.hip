// float8 (OCP e4m3fn) per-row-scaled weight-only linear, skinny-M (decode) path:
//   y[m][n] = bf16( (sum_k x[m][k] * f(w[n][k])) * scale[n] ) (+ bias[n] -> bf16)
// with f the exact e4m3fn -> real decode, the sum and the scale product in fp32.
// Replaces F.linear(x, weight.dequantize(), bias) at torchao/dtypes/floatx/float8_layout.py:391-396,
// which writes a bf16 copy of W (2 B per weight) on every call and reads it back in a library
// GEMM; here the 1-B codes are read once. The scale is applied once per output instead of once
// per weight.
//
// The byte-weight decomposition of tao_gemv.h (a slice is 1024 k of one row); launcher and M
// dispatcher are the ones shared with int8wo_gemv_kernel (wo8_gemv).
// Per lane: one v_cvt_scalef32_pk_bf16_fp8 (scale 1.0: exact, all finite e4m3fn values are bf16
// numbers) turns two codes into a bf16 pair, one v_dot2c_f32_bf16 multiplies it with the x pair
// as loaded: 1.0 VALU per weight and no x conversion (v_cvt_pk_f32_fp8 + v_fma_f32 would be 1.5
// plus the bf16 -> f32 shifts of x). No bias trick is needed: the codes decode signed.
#include "tao_gemm.h"
#include "tao_gemv.h"

namespace tao {

TAO_DECODE_ERROR_WORD(fp8gemv_decode_status)

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

  const WgTotal<float> t = wg_combine<V>(v[0], red, lane, wk, rg, Wk);
  if (t.writer) {
    const int r = t.widx / MT, m = t.widx % MT;
    const int n = row0 + r;
    if (n < N && m < M) {
      // the fp32 sum times the fp32 scale, rounded once; then + bias, rounded again
      float o = round_bf16(t.total * scale[n]);
      if (bias != nullptr) o = round_bf16(o + bf16_to_f32(bias[n]));
      y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

struct Fp8Gemv {  // what wo8_gemv launches
  using scale_t = float;
  static constexpr const char* name = "fp8wo_gemv_kernel";
  template <int MT, int RPW>
  static auto kernel() {
    return fp8wo_gemv_kernel<MT, RPW>;
  }
};

// ---- the float8 policy of wo8_decode_kernel (tao_gemv.h; tao_fp8wo_decode_bf16; DESIGN.md §4.5,
// §4.11): fp8wo_gemv_kernel's slice arithmetic. The epilogues' a and b are the linear's own
// outputs bf16(sum * scale[n]). ----
struct Fp8Decode {
  using scale_t = float;
  static constexpr const char* name = "fp8wo_decode_kernel";
  static constexpr const char* what = "fp8 decode";
  // A lane past the row's last chunk loaded a clamped (valid) address and skips the math: its
  // codes may be NaN (an all-zero row quantizes to NaN codes), which 0 * w would not cancel.
  static constexpr bool kSkipTail = true;
  struct X {  // the chunk's 8 bf16 pairs as loaded: no conversion
    uint32_t d8[8];
  };
  static __device__ __forceinline__ X prep(uint4 a, uint4 b, bool) {
    return {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
  }
  static __device__ __forceinline__ float dot(const X& x, uint4 wv) {
    const uint32_t wd[4] = {wv.x, wv.y, wv.z, wv.w};
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d = dot2_bf16(x.d8[2 * j], fp8_pair_bf16<false>(wd[j]), d);
      d = dot2_bf16(x.d8[2 * j + 1], fp8_pair_bf16<true>(wd[j]), d);
    }
    return d;
  }
  // the fp32 sum times the fp32 scale, rounded once (fp8wo_gemv_kernel's no-bias epilogue)
  static __device__ __forceinline__ float out(float total, float scale) {
    return round_bf16(total * scale);
  }
  static __device__ __forceinline__ void flag_bad_kv_pos() { flag_decode_error(kDecodeErrKvPos); }
};

}  // namespace

int fp8wo_gemv(const uint16_t* x, const uint8_t* w, const float* scale, const uint16_t* bias,
               uint16_t* y, int64_t M, int64_t N, int64_t K, hipStream_t stream) {
  return wo8_gemv<Fp8Gemv>(x, w, scale, bias, y, (int)M, (int)N, (int)K, stream,
                            tuning().fp8_rpw, tuning().fp8_wk, tuning().fp8_g);
}

}  // namespace tao

extern "C" int tao_fp8wo_decode_bf16(const uint16_t* x, const uint8_t* w, const float* scale,
                                     int64_t N, int64_t K, const uint16_t* norm_weight, float eps,
                                     int epilogue, uint16_t* y, const float* freqs,
                                     const int64_t* pos, uint16_t* k_cache, uint16_t* v_cache,
                                     int64_t n_head, int64_t n_kv_head, int64_t head_dim,
                                     int64_t max_seq, void* stream) {
  using namespace tao;
  int rc = check_decode_epilogue("fp8 decode", epilogue, N);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(N >= 0 && N < (1LL << 31) && K > 0 && K < (1LL << 31),
                "fp8 decode: K (%lld) must be positive and N, K below 2^31", (long long)K);
  TAO_CHECK_ARG(K % 32 == 0, "fp8 decode: K (%lld) must be a multiple of 32", (long long)K);
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(y, 2, "y");
  if (norm_weight != nullptr) TAO_CHECK_ALIGN(norm_weight, 16, "norm_weight");
  TAO_CHECK_ALIGN(scale, 4, "scale");
  TAO_CHECK_ARG(norm_weight == nullptr || K <= 16384,
                "fp8 decode: K (%lld) must be <= 16384 with norm_weight (the RMSNorm prologue "
                "holds the token in registers)",
                (long long)K);
  DecodeFuse fu{};
  rc = check_decode_fuse("fp8 decode", epilogue, N, norm_weight, eps, y, freqs, pos, k_cache,
                         v_cache, n_head, n_kv_head, head_dim, max_seq, &fu);
  if (rc != TAO_OK) return rc;
  if (N == 0) return TAO_OK;
  const hipStream_t st = as_stream(stream);
  const Wo8Want want = fp8_decode_want(tuning().fp8_rpw, tuning().fp8_wk, tuning().fp8_g,
                                       norm_weight != nullptr);
  return dispatch_epilogue(epilogue, [&](auto epi) {
    return wo8_decode<Fp8Decode, decltype(epi)::value>(x, w, scale, y, (int)N, (int)K, want, st,
                                                       fu);
  });
}

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
