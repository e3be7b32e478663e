// float8 dynamic-activation x float8-weight linear, per-row scales on both operands
// (Float8DynamicActivationFloat8WeightConfig, granularity PerRow, e4m3fn, version 1):
//
//   acc[m][n] = sum_k f(xq[m][k]) * f(wq[n][k])      f the exact e4m3fn decode; every product of
//                                                    two e4m3fn values is an fp32 number; the sum
//                                                    is formed in fp32
//   y[m][n]   = bf16( fp32(fp32(acc * xs[m]) * ws[n]) + fp32(bias[n]) )
//
// One rounding to bf16, with or without bias: the way a row-wise _scaled_mm epilogue is specified.
// (tao_fp8wo_linear_bf16 rounds to bf16 before the bias and once more after it.) No eps anywhere,
// as in the reference: an all-zero token or weight row quantises to scale 0.0 and NaN codes, and
// its output row / column is NaN.
//
//   1. tao_fp8_scaled_mm_bf16: replaces the torch._scaled_mm call of
//      _linear_fp8_act_fp8_weight_impl (torchao/dtypes/floatx/float8_layout.py:329-367).
//      M above the GEMV crossover: the Fp8Dyn instance of the shared skinny-GEMM template
//      (gemm_mfma.hip) on v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales; M at or below
//      it: the decode GEMV (below).
//   2. tao_fp8_dyn_linear_bf16 (one token): the activation quantisation
//      (_input_activation_quant_func_fp8 -> tao_fp8_quantize_rows_bf16's arithmetic, fp8_quant_row.h)
//      and the GEMV in one launch, as tao_int8_dyn_linear_bf16 does for int8: every workgroup
//      issues its first weight slice, quantises the token into LDS under that latency, then runs
//      the GEMV on the codes. Bit-identical to tao_fp8_quantize_rows_bf16 -> tao_fp8_scaled_mm_bf16.
//      More than one token is those two calls; the caller owns the code buffer between them (the
//      convention of the int8 dynamic path: no scratch is allocated here).
//   3. tao_fp8dq_decode_bf16 (one token, the Llama decode harness): 2 with an optional RMSNorm of
//      the token before its quantisation and a SwiGLU or RoPE + KV-write row-pair epilogue
//      (fp8dq_decode_kernel below).
//
// The decode GEMV of 1 and 2 is scaled_gemv_kernel (scaled_gemv.h: decomposition, hardware decode
// of both code streams, skipped tail lanes, the fused prologue's order of loads) under the policy
// Fp8DynFmt below, recorded as "fp8dyn_gemv_kernel". This format's own part: a lane's fp32 partial
// sums are added unscaled (a slice is 1024 k of one row); the two scales meet the workgroup's total
// in the epilogue; the fused launch takes the token's amax across the whole row, through LDS.
#include "scaled_gemv.h"
#include "tao_gemm.h"

// The epilogue is specified as separate fp32 roundings (mul, mul, add): no fused multiply-add.
#pragma clang fp contract(off)

namespace tao {

TAO_DECODE_ERROR_WORD(fp8dyn_decode_status)

namespace {

// The per-row policy of scaled_gemv_kernel: one fp32 scale per token and per weight row, met with
// the total in the epilogue (under this file's contract(off): two roundings, no fma with the bias).
struct Fp8DynFmt {
  using Args = ScaledGemvArgs<float>;  // xs [M], ws [N]
  using Scale = float;
  static constexpr const char* name = "fp8dyn_gemv_kernel";
  static constexpr const char* what = "fp8";
  static constexpr int kChunkShift = 4;
  static constexpr bool kRowScales = true, kFp4Weights = false;
  static constexpr int kBlockShift = 0;  // no blocks
  static __device__ __forceinline__ float row_scaled(float total, float xs, float ws) {
    return (total * xs) * ws;
  }
};

// M == 1, both overridden by tao_tune_fp8_gemv: on ready-made codes scaled_gemv's shape, the fused
// launch scaled_gemv_fused's.
template <bool FQ>
int gemv_m1(const Fp8DynFmt::Args& a, hipStream_t stream) {
  const int rpw = tuning().fp8_rpw > 0 ? tuning().fp8_rpw : (FQ ? 8 : 4);
  const int wk = tuning().fp8_wk > 0 ? tuning().fp8_wk : (FQ ? 4 : 8);
  const int g = tuning().fp8_g > 0 ? tuning().fp8_g : (FQ ? 2 : 1);
  if (rpw == 2) return scaled_gemv_launch<Fp8DynFmt, 1, 2, FQ>(a, wk, g, stream);
  if (rpw == 8) return scaled_gemv_launch<Fp8DynFmt, 1, 8, FQ>(a, wk, g, stream);
  return scaled_gemv_launch<Fp8DynFmt, 1, 4, FQ>(a, wk, g, stream);
}

// ---- decode-step fusions of the one-token launch (tao_fp8dq_decode_bf16) ---------------------
// scaled_gemv_kernel's fused path under Fp8DynFmt (one token, quantised per row inside every
// workgroup) as a sibling kernel with the fusions of tao_gemv.h: NORM, the RMSNorm of the token
// before its quantisation (rmsnorm_kernel's two roundings, then amax / scale / codes on the
// normalised bf16 values: the bytes tao_rmsnorm_bf16 -> tao_fp8_quantize_rows_bf16 produce up to
// the norm's fp32 sum order), and the row-pair epilogues on the linear's own bf16 output
// bf16((sum * xs) * ws[n]). NPT 16-B pieces of the token per thread (K <= 8 NPT threads), with
// NORM as many of the norm weight beside them.
struct Fp8DqDecodeArgs {
  const uint16_t* x;  // the bf16 token [K]
  const uint4* w;     // [N][K/16] e4m3fn codes
  const float* ws;    // [N] fp32
  uint16_t* y;
  int N, K, Wk, G, S;
  DecodeFuse fu;
};

template <int RPW, int NPT, int EPI, bool NORM>
__global__ __launch_bounds__(512) void fp8dq_decode_kernel(Fp8DqDecodeArgs a) {
  constexpr int V = RPW;
  // [G][Wk][V] fp32 partials | [8] wave sums of squares, then wave maxima | the token's codes [K]
  extern __shared__ float lds_f[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % a.Wk;
  const int rg = wave / a.Wk;
  const int row0 = (blockIdx.x * a.G + rg) * RPW;
  const int K = a.K, N = a.N, S = a.S, Wk = a.Wk;
  const int nchunk = K >> 4;  // 16-B (16-k) chunks per row
  const int nvec = K >> 3;    // 16-B pieces of the bf16 token
  const int nw = a.G * a.Wk;
  float* wred = lds_f + nw * V;
  uint4* xl = reinterpret_cast<uint4*>(lds_f + ((nw * V + 8 + 3) & ~3));

  uint4 wv[RPW];
  auto load_w = [&](int s) __attribute__((always_inline)) {
    const int c = s * 64 + lane;
    const int cc = c < nchunk ? c : nchunk - 1;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      wv[r] = ld_nt_u4(a.w + (size_t)(n < N ? n : N - 1) * nchunk + cc);
    }
  };

  // The token's (and the norm weight's) pieces are loaded BEFORE the first slice's weights:
  // vector loads retire in issue order, so the wait for x does not wait for the weights, and the
  // norm, the amax, the barriers and the quantisation into LDS run under the weight loads' latency.
  const uint4* xr = reinterpret_cast<const uint4*>(a.x);
  uint4 xv[NPT], gv[NORM ? NPT : 1];
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int i = threadIdx.x + u * (int)blockDim.x;
    const int ic = i < nvec ? i : nvec - 1;  // clamped duplicates do not change the max
    xv[u] = xr[ic];
    if constexpr (NORM) gv[u] = reinterpret_cast<const uint4*>(a.fu.norm_w)[ic];
  }
  load_w(wk);  // Wk <= S: every wave owns a slice
  if constexpr (NORM) {
    float ss = 0.f;
#pragma unroll
    for (int u = 0; u < NPT; ++u)
      ss = sumsq_piece(xv[u], threadIdx.x + u * (int)blockDim.x < nvec, ss);
    ss = wave_sum(ss);
    if (lane == 0) wred[wave] = ss;
    __syncthreads();
    float t = 0.f;
    for (int q = 0; q < nw; ++q) t += wred[q];
    const float rn = rsqrtf(t / (float)K + a.fu.eps);
#pragma unroll
    for (int u = 0; u < NPT; ++u) xv[u] = rmsnorm_piece(xv[u], gv[u], rn);
    __syncthreads();  // wred is reused for the amax below
  }
  float m = 0.f;
#pragma unroll
  for (int u = 0; u < NPT; ++u) m = fp8_amax8(xv[u], m);
  m = wave_max(m);
  if (lane == 0) wred[wave] = m;
  __syncthreads();
  float amax = wred[0];
  for (int q = 1; q < nw; ++q) amax = fmaxf(amax, wred[q]);
  const float st = fp8_row_scale(amax);
  uint2* xq = reinterpret_cast<uint2*>(xl);
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int i = threadIdx.x + u * (int)blockDim.x;
    if (i < nvec) xq[i] = fp8_quant8(xv[u], st);
  }
  __syncthreads();

  float acc[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) acc[r] = 0.f;
  for (int s = wk; s < S; s += Wk) {
    if (s != wk) load_w(s);
    const int c = s * 64 + lane;
    if (c < nchunk) {  // tail lanes skip the math: clamped codes may be NaN
      uint32_t xp[8];
      e4m3_chunk_bf16(xl[c], xp);
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        uint32_t wp[8];
        e4m3_chunk_bf16(wv[r], wp);
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d = dot2_bf16(xp[i], wp[i], d);
        acc[r] += d;
      }
    }
  }

  float v[V];
#pragma unroll
  for (int r = 0; r < RPW; ++r) v[r] = acc[r];
  wave_reduce_scatter<V>(v, lane);
  const WgTotal<float> t = wg_combine<V>(v[0], lds_f, lane, wk, rg, Wk);
  // the linear's bf16 output of row t.widx: tao_fp8_dyn_linear_bf16's fp32 epilogue without bias
  const int nrow = row0 + (t.widx < V ? t.widx : 0);
  const float o = round_bf16((t.total * st) * a.ws[nrow < N ? nrow : N - 1]);
  if constexpr (EPI == kEpiNone) {
    if (t.writer && row0 + t.widx < N) a.y[row0 + t.widx] = f32_to_bf16(o);
  } else {
    pair_epilogue<EPI, RPW>(o, lane, wk, Wk, row0, N, a.y, a.fu,
                            [] { flag_decode_error(kDecodeErrKvPos); });
  }
}

template <int RPW, int NPT, int EPI, bool NORM>
int launch_dq_decode_npt(const Fp8DqDecodeArgs& a, const Fp8DynLaunch& L, hipStream_t stream) {
  launch((fp8dq_decode_kernel<RPW, NPT, EPI, NORM>), dim3(L.grid), dim3(L.threads), L.lds, stream,
         a);
  return check_launch("fp8dq_decode_kernel");
}

template <int RPW, int EPI>
int launch_dq_decode(Fp8DqDecodeArgs a, int wk, int g, hipStream_t stream) {
  const bool norm = a.fu.norm_w != nullptr;
  const Fp8DynLaunch L = fp8dyn_launch_shape(a.N, a.K, RPW, 1, wk, g, true, norm ? 4 : 8);
  a.S = L.S;
  a.Wk = L.Wk;
  a.G = L.G;
  if (norm) {
    if (L.per <= 1) return launch_dq_decode_npt<RPW, 1, EPI, true>(a, L, stream);
    if (L.per <= 2) return launch_dq_decode_npt<RPW, 2, EPI, true>(a, L, stream);
    if (L.per <= 4) return launch_dq_decode_npt<RPW, 4, EPI, true>(a, L, stream);
  } else {
    if (L.per <= 1) return launch_dq_decode_npt<RPW, 1, EPI, false>(a, L, stream);
    if (L.per <= 2) return launch_dq_decode_npt<RPW, 2, EPI, false>(a, L, stream);
    if (L.per <= 4) return launch_dq_decode_npt<RPW, 4, EPI, false>(a, L, stream);
    if (L.per <= 8) return launch_dq_decode_npt<RPW, 8, EPI, false>(a, L, stream);
  }
  TAO_CHECK_ARG(false, "fp8dq decode: K (%d) too long for the token prologue of %d threads", a.K,
                L.threads);
  return TAO_OK;
}

// the fused launch's shape (gemv_m1<true>): 8 rows per wave, 4 waves along K, 2 row groups
template <int EPI>
int dq_decode(const Fp8DqDecodeArgs& a, hipStream_t stream) {
  const int rpw = tuning().fp8_rpw > 0 ? tuning().fp8_rpw : 8;
  const int wk = tuning().fp8_wk > 0 ? tuning().fp8_wk : 4;
  const int g = tuning().fp8_g > 0 ? tuning().fp8_g : 2;
  if (rpw == 2) return launch_dq_decode<2, EPI>(a, wk, g, stream);
  if (rpw == 4) return launch_dq_decode<4, EPI>(a, wk, g, stream);
  return launch_dq_decode<8, EPI>(a, wk, g, stream);
}

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_fp8_scaled_mm_bf16(const uint8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                           const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                           void* stream) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "fp8 scaled mm: negative size");
  TAO_CHECK_ARG(K % 16 == 0, "fp8 scaled mm: K (%lld) must be a multiple of 16", (long long)K);
  TAO_CHECK_ARG(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31) &&
                    M * K < (1LL << 32) && N * K < (1LL << 32),
                "fp8 scaled mm: size out of range (operands below 4 GiB)");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "fp8 scaled mm: K must be > 0");
  TAO_CHECK_ALIGN(xq, 16, "xq");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  TAO_CHECK_ALIGN(xs, 4, "xs");
  TAO_CHECK_ALIGN(ws, 4, "ws");
  if (fp8dyn_takes_gemv(M, N, K)) {
    const Fp8DynFmt::Args a{xq, xs, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                            (int)M, (int)N, (int)K, 0, 0, 0};
    if (M <= 1) return gemv_m1<false>(a, as_stream(stream));
    return scaled_gemv<Fp8DynFmt>(a, as_stream(stream));
  }
  return fp8_scaled_mm_launch(xq, xs, wq, ws, bias, y, (int)M, (int)N, (int)K, as_stream(stream));
}

int tao_fp8_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const float* ws,
                            const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                            void* stream) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "fp8 dyn linear: negative size");
  TAO_CHECK_ARG(M <= 1, "fp8 dyn linear: the fused path is one token (M <= 1, got %lld)",
                (long long)M);
  TAO_CHECK_ARG(K % 16 == 0, "fp8 dyn linear: K (%lld) must be a multiple of 16", (long long)K);
  TAO_CHECK_ARG(K <= 65536, "fp8 dyn linear: K (%lld) must be <= 65536 (token in LDS)",
                (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31), "fp8 dyn linear: size out of range");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "fp8 dyn linear: K must be > 0");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  TAO_CHECK_ALIGN(ws, 4, "ws");
  const Fp8DynFmt::Args a{x, nullptr, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                          1, (int)N, (int)K, 0, 0, 0};
  return gemv_m1<true>(a, as_stream(stream));
}

int tao_fp8dq_decode_bf16(const uint16_t* x, const uint8_t* wq, const float* ws, int64_t N,
                          int64_t K, const uint16_t* norm_weight, float eps, int epilogue,
                          uint16_t* y, const float* freqs, const int64_t* pos, uint16_t* k_cache,
                          uint16_t* v_cache, int64_t n_head, int64_t n_kv_head, int64_t head_dim,
                          int64_t max_seq, void* stream) {
  int rc = check_decode_epilogue("fp8dq decode", epilogue, N);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ARG(N >= 0 && N < (1LL << 31) && K > 0 && K < (1LL << 31),
                "fp8dq decode: K (%lld) must be positive and N, K below 2^31", (long long)K);
  TAO_CHECK_ARG(K % 16 == 0, "fp8dq decode: K (%lld) must be a multiple of 16", (long long)K);
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  TAO_CHECK_ALIGN(y, 2, "y");
  if (norm_weight != nullptr) TAO_CHECK_ALIGN(norm_weight, 16, "norm_weight");
  TAO_CHECK_ALIGN(ws, 4, "ws");
  TAO_CHECK_ARG(K <= (norm_weight != nullptr ? 16384 : 32768),
                "fp8dq decode: K (%lld) must be <= 32768, <= 16384 with norm_weight (the token "
                "prologue holds the token in registers)",
                (long long)K);
  Fp8DqDecodeArgs a{x, reinterpret_cast<const uint4*>(wq), ws, y, (int)N, (int)K, 0, 0, 0, {}};
  rc = check_decode_fuse("fp8dq decode", epilogue, N, norm_weight, eps, y, freqs, pos, k_cache,
                         v_cache, n_head, n_kv_head, head_dim, max_seq, &a.fu);
  if (rc != TAO_OK) return rc;
  if (N == 0) return TAO_OK;
  const hipStream_t st = as_stream(stream);
  return dispatch_epilogue(
      epilogue, [&](auto epi) { return dq_decode<decltype(epi)::value>(a, st); });
}

}  // extern "C"
