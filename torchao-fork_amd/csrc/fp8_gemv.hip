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

// ---- decode-step fusions of the M == 1 float8 weight-only GEMV (tao_fp8wo_decode_bf16) ------
// The fusions of tao_gemv.h on the e4m3fn weight stream: the structure of
// int8wo_decode_kernel with fp8wo_gemv_kernel's slice arithmetic, so a float8wo Llama layer is 5
// launches per token instead of 9. NPT > 0: the RMSNorm prologue, x normalised once per
// workgroup into LDS while the first weight slice is in flight (NPT 16-B pieces of x and of the
// norm weight per thread: K <= 8 NPT threads). The epilogues' a and b are the linear's own
// outputs bf16(sum * scale[n]). Tail lanes skip the math, as in fp8wo_gemv_kernel.
template <int RPW, int NPT, int EPI>
__global__ __launch_bounds__(512) void fp8wo_decode_kernel(
    const uint16_t* __restrict__ x, const uint4* __restrict__ w, const float* __restrict__ scale,
    uint16_t* __restrict__ y, int N, int K, int Wk, int G, int S, DecodeFuse fu) {
  constexpr bool PRO = NPT > 0;
  constexpr int V = RPW;
  // [G][Wk][V] partials | [16] wave sums of squares | (PRO) normalised x [K / 8] uint4
  extern __shared__ float red[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wk = wave % Wk;
  const int rg = wave / Wk;
  const int row0 = (blockIdx.x * G + rg) * RPW;
  const int nchunk = K >> 4;
  const int nx = K >> 3;
  float* ssr = red + G * Wk * V;
  uint4* xs = reinterpret_cast<uint4*>(red + ((G * Wk * V + 16 + 3) & ~3));

  uint4 wv[RPW];
  auto load_w = [&](int s) __attribute__((always_inline)) {
    const int c = s * 64 + lane;
    const int cc = c < nchunk ? c : nchunk - 1;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      wv[r] = ld_nt_u4(w + (size_t)(n < N ? n : N - 1) * nchunk + cc);
    }
  };

  uint4 xv[PRO ? NPT : 1], gv[PRO ? NPT : 1];
  if constexpr (PRO) {  // x and the norm weight first: their vmcnt wait does not wait for W
    const uint4* xr = reinterpret_cast<const uint4*>(x);
    const uint4* gr = reinterpret_cast<const uint4*>(fu.norm_w);
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      const int ic = i < nx ? i : nx - 1;
      xv[u] = xr[ic];
      gv[u] = gr[ic];
    }
  }
  load_w(wk);  // Wk <= S: every wave owns a slice
  if constexpr (PRO) {
    float ss = 0.f;
#pragma unroll
    for (int u = 0; u < NPT; ++u)
      ss = sumsq_piece(xv[u], threadIdx.x + u * (int)blockDim.x < nx, ss);
    ss = wave_sum(ss);
    if (lane == 0) ssr[wave] = ss;
    __syncthreads();
    float t = 0.f;
    for (int q = 0; q < G * Wk; ++q) t += ssr[q];
    const float r = rsqrtf(t / (float)K + fu.eps);
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      // int8wo_decode_kernel's image: piece i of 16-k chunk c = i >> 1 lands at
      // 2 c + ((i + (c >> 3)) & 1), the two halves of a pass on distinct bank groups
      if (i < nx) xs[(i & ~1) | ((i + (i >> 4)) & 1)] = rmsnorm_piece(xv[u], gv[u], r);
    }
    __syncthreads();
  }

  float acc[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) acc[r] = 0.f;
  for (int s = wk; s < S; s += Wk) {
    if (s != wk) load_w(s);
    const int c = s * 64 + lane;
    // A lane past the row's last chunk loaded a clamped (valid) address and skips the math: its
    // codes may be NaN (an all-zero row quantizes to NaN codes), which 0 * w would not cancel.
    if (c < nchunk) {
      uint4 a, b;
      if constexpr (PRO) {
        const int rot = (c >> 3) & 1;
        a = xs[2 * c + rot];
        b = xs[2 * c + (rot ^ 1)];
      } else {
        const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)c * 16);
        a = xp[0];
        b = xp[1];
      }
      const uint32_t d8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const uint32_t wd[4] = {wv[r].x, wv[r].y, wv[r].z, wv[r].w};
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          d = dot2_bf16(d8[2 * j], fp8_pair_bf16<false>(wd[j]), d);
          d = dot2_bf16(d8[2 * j + 1], fp8_pair_bf16<true>(wd[j]), d);
        }
        acc[r] += d;
      }
    }
  }

  float v[V];
#pragma unroll
  for (int r = 0; r < RPW; ++r) v[r] = acc[r];
  wave_reduce_scatter<V>(v, lane);
  const WgTotal<float> t = wg_combine<V>(v[0], red, lane, wk, rg, Wk);
  // the linear's bf16 output of row t.widx: the fp32 sum times the fp32 scale, rounded once
  // (fp8wo_gemv_kernel's no-bias epilogue)
  const int nrow = row0 + (t.widx < V ? t.widx : 0);
  const float o = round_bf16(t.total * scale[nrow < N ? nrow : N - 1]);
  if constexpr (EPI == kEpiNone) {
    if (t.writer && row0 + t.widx < N) y[row0 + t.widx] = f32_to_bf16(o);
  } else {
    pair_epilogue<EPI, RPW>(o, lane, wk, Wk, row0, N, y, fu,
                            [] { flag_decode_error(kDecodeErrKvPos); });
  }
}

template <int RPW, int NPT, int EPI>
int launch_fp8_decode(const uint16_t* x, const uint8_t* w, const float* scale, uint16_t* y, int N,
                      int K, GemvLaunchShape sh, hipStream_t stream, const DecodeFuse& fu) {
  const int grid = (N + sh.G * RPW - 1) / (sh.G * RPW);
  const size_t lds = (((size_t)sh.G * sh.Wk * RPW + 16 + 3) & ~(size_t)3) * sizeof(float) +
                     (NPT > 0 ? (size_t)K * 2 : 0);
  launch((fp8wo_decode_kernel<RPW, NPT, EPI>), dim3(grid), dim3(64 * sh.Wk * sh.G), lds, stream,
         x, reinterpret_cast<const uint4*>(w), scale, y, N, K, sh.Wk, sh.G, sh.S, fu);
  return check_launch("fp8wo_decode_kernel");
}

template <int EPI>
int fp8_decode(const uint16_t* x, const uint8_t* w, const float* scale, uint16_t* y, int N, int K,
               hipStream_t stream, const DecodeFuse& fu) {
  // Without the norm, fp8wo_gemv_kernel's M == 1 shape: 4 rows per wave, Wk = min(S, 8) waves
  // along K, one row group. With it every workgroup re-normalises the token, so fewer, larger
  // workgroups pay: 8 rows per wave, 4 waves along K (fused, 4 x 8 x 1 vs 8 x 4 x 1, us: 6144 x
  // 4096 7.9 vs 7.5, 28672 x 4096 25.3 vs 20.8, the 128256 x 4096 head 93.2 vs 75.4, 10240 x 8192
  // 20.2 vs 17.1, 57344 x 8192 93.2 vs 72.5; profiles/fp8_decode_shape_ab.jsonl).
  // tao_tune_fp8_gemv overrides both. The prologue needs K <= 8 x NPT x threads: row groups are
  // added while they fit 8 waves.
  const bool pro = fu.norm_w != nullptr;
  const int trpw = tuning().fp8_rpw > 0 ? tuning().fp8_rpw : (pro ? 8 : 4);
  const int twk = tuning().fp8_wk > 0 ? tuning().fp8_wk : (pro ? 4 : 8);
  const int tg = tuning().fp8_g > 0 ? tuning().fp8_g : 1;
  GemvLaunchShape sh = gemv_launch_shape(K / 16, twk, tg);
  while (pro && sh.Wk * sh.G * 2 <= 8 && 64 * sh.Wk * sh.G * 8 * 4 < K) sh.G *= 2;
  const int threads = 64 * sh.Wk * sh.G;
  if (threads > 512)
    return set_error(TAO_ERR_INVALID_ARGUMENT, "fp8 decode: %d waves along K exceed 8", sh.Wk);
  if (pro && threads * 8 * 4 < K)
    return set_error(TAO_ERR_INVALID_ARGUMENT,
                     "fp8 decode: K (%d) too long for the RMSNorm prologue of %d threads", K,
                     threads);
  const int npt = !pro ? 0 : (threads * 8 >= K ? 1 : threads * 8 * 2 >= K ? 2 : 4);
#define TAO_F8D(R, P) return launch_fp8_decode<R, P, EPI>(x, w, scale, y, N, K, sh, stream, fu)
  if (trpw == 8) {
    if (npt == 0) TAO_F8D(8, 0);
    if (npt == 1) TAO_F8D(8, 1);
    if (npt == 2) TAO_F8D(8, 2);
    TAO_F8D(8, 4);
  }
  if (trpw == 2) {
    if (npt == 0) TAO_F8D(2, 0);
    if (npt == 1) TAO_F8D(2, 1);
    if (npt == 2) TAO_F8D(2, 2);
    TAO_F8D(2, 4);
  }
  if (npt == 0) TAO_F8D(4, 0);
  if (npt == 1) TAO_F8D(4, 1);
  if (npt == 2) TAO_F8D(4, 2);
  TAO_F8D(4, 4);
#undef TAO_F8D
}

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
  switch (epilogue) {
    case kEpiSwiGLU: return fp8_decode<kEpiSwiGLU>(x, w, scale, y, (int)N, (int)K, st, fu);
    case kEpiRopeKV: return fp8_decode<kEpiRopeKV>(x, w, scale, y, (int)N, (int)K, st, fu);
    default: return fp8_decode<kEpiNone>(x, w, scale, y, (int)N, (int)K, st, fu);
  }
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
