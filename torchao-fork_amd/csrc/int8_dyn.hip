// int8 dynamic-activation x int8-weight linear (Int8DynamicActivationInt8WeightConfig):
//   1. tao_int8_quant_per_token: x bf16 [M][K] -> (q int8 [M][K], s bf16 [M]), replacing
//      _int8_symm_per_token_reduced_range_quant (torchao/quantization/quant_api.py:1258-1273),
//      which the reference runs as ~6 eager kernels (amin/amax/div/round/clamp/cast);
//   2. tao_int8_scaled_mm_bf16: int32 MFMA GEMM with the fused two-scale epilogue, replacing
//      int_scaled_matmul + the weight-scale multiply (torchao/kernel/intmm.py:108-143,
//      torchao/dtypes/uintx/plain_layout.py:294-315). M > 4: the Int8Dyn instance of the
//      shared skinny-GEMM template in gemm_mfma.hip; M <= 4 (decode): int8dyn_gemv_kernel
//      below, exact int32 dot products (v_dot4_i32_i8) streamed like the int4 / int8 GEMVs;
//   3. tao_int8_dyn_linear_bf16 (M == 1): 1 + 2 in one launch — every workgroup quantises the
//      token into LDS (the per-token kernel's exact arithmetic) while its first weight slice
//      is in flight, then runs the GEMV on it: one launch per linear instead of two;
//   4. SmoothQuant on top of 1-3 (tao_int8_smooth_quant_bf16, tao_int8_smooth_linear_bf16): the
//      token is divided by the per-input-channel smoothing factor before it is quantised, per
//      token or with a calibrated per-tensor scale, replacing the `x / scale` of
//      WeightTensorWithLinearActivationScaleMetadata and _ActQuantizer's eager quantisation
//      (torchao/prototype/smoothquant/api.py:133-155). The quotient is never written to memory.
#include <atomic>

#include "int8_quant_row.h"
#include "tao_gemm.h"
#include "tao_gemv.h"

namespace tao {

TAO_DECODE_ERROR_WORD(int8dyn_decode_status)

// Launch shape override of the int8 decode GEMVs (tao_tune_int8_gemv; 0 = heuristic), shared
// with int8wo_gemv (int8_gemv.hip).

namespace {


// ---- int8 x int8 GEMV (decode) ------------------------------------------------------------------
// The byte-weight decomposition of tao_gemv.h (a slice is 1024 k of one row). Per lane and row:
// four v_dot4_i32_i8 per 16-B chunk into an int32 accumulator. Every partial sum is an exact
// integer (|acc| <= 127 * 127 * K < 2^31 for K < 133144), so the cross-lane and cross-wave
// reduction order cannot change the result: bit-identical to the MFMA path and the reference.
// Lanes past K read a clamped in-bounds chunk and a zeroed x, adding exactly 0.
//
// FQ (M == 1): x is the bf16 token. Each workgroup first issues its first slice's weight loads,
// then quantises the token into LDS with int8_quant_per_token_kernel's exact arithmetic (below)
// under their latency, so the per-token quantisation costs no launch of its own.
//
// SMQ (with FQ; SmoothQuant): the token's pieces are first divided by the smoothing factor's
// (fu.norm_w holds the factor [K]; div_piece_bf16, the bits of tao_act_prescale_bf16).
// kSmoothDyn then quantises per token with the 2^-7 scale clamp (token_scale_default_eps);
// kSmoothStatic takes the per-tensor scale from xs[0] instead: no amax and no barrier before the
// quantisation.
constexpr int kSmoothNone = 0, kSmoothDyn = 1, kSmoothStatic = 2;

struct Int8DynGemvArgs {
  const void* x;          // int8 q [M][K] (FQ: bf16 token [K])
  const uint16_t* xs;     // [M] bf16 per-token scales (FQ: unused; kSmoothStatic: the scale [1])
  const uint4* w;         // [N][K/16]
  const uint16_t* ws;     // [N]
  const uint16_t* bias;   // [N] or null
  uint16_t* y;            // [M][N]
  int M, N, K, Wk, G, S;
  // decode-step fusions (tao_int8dq_decode_bf16, FQ only): RMSNorm of the token before its
  // quantisation, SwiGLU / RoPE + KV-write epilogues
  DecodeFuse fu;
};

__device__ __forceinline__ int sdot4(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}

// per-token scale (token_scale), codes (quant8) and amax step (bf16_abs_max2): int8_quant_row.h

template <int MT, int RPW, int NPT, int EPI = kEpiNone, int SMQ = kSmoothNone>
__global__ __launch_bounds__(512) void int8dyn_gemv_kernel(Int8DynGemvArgs a) {
  constexpr bool FQ = NPT > 0;  // NPT: 16-B pieces of the bf16 token per thread (K <= 8 NPT T)
  static_assert(!FQ || MT == 1, "the fused quantisation is per token, M == 1");
  static_assert(EPI == kEpiNone || FQ, "epilogues: fused token");
  static_assert(SMQ == kSmoothNone || (FQ && EPI == kEpiNone),
                "smoothing: fused token, no epilogue");
  constexpr int V = RPW * MT;
  // [G][Wk][V] int partials | (FQ) [8] wave maxima | (FQ) token q [K] int8
  extern __shared__ int lds_i[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % a.Wk;
  const int rg = wave / a.Wk;
  const int row0 = (blockIdx.x * a.G + rg) * RPW;
  const int K = a.K, N = a.N, S = a.S, Wk = a.Wk;
  const int nchunk = K >> 4;  // 16-B (16-k) chunks per row
  const int nw = a.G * a.Wk;
  float* wmax = reinterpret_cast<float*>(lds_i + nw * V);
  uint4* xl = reinterpret_cast<uint4*>(lds_i + ((nw * V + 8 + 3) & ~3));

  int acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0;

  uint4 wv[RPW];
  // int8_gemv.hip's load_w_slice, written in place: through the helper the RPW = 8 instantiations
  // take 2-8 more VGPRs and the NPT = 16 ones spill 76 B/lane more (hipcc 7.2 resource report)
  auto load_w = [&](int s) __attribute__((always_inline)) {
    const int c = s * 64 + lane;
    const int cc = c < nchunk ? c : nchunk - 1;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      wv[r] = ld_nt_u4(a.w + (size_t)(n < N ? n : N - 1) * nchunk + cc);
    }
  };

  float sx[MT];
  if constexpr (FQ) {
    // The token's pieces are loaded BEFORE the first slice's weights: vector loads retire in
    // issue order, so the wait for x does not wait for the weights, and the amax, the two
    // barriers and the quantisation into LDS run under the weight loads' latency.
    const uint4* xr = reinterpret_cast<const uint4*>(a.x);
    const int nvec = K >> 3;
    uint4 xv[NPT], gv[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      xv[u] = xr[i < nvec ? i : nvec - 1];  // clamped, masked below
      if (SMQ != kSmoothNone || a.fu.norm_w != nullptr)
        gv[u] = reinterpret_cast<const uint4*>(a.fu.norm_w)[i < nvec ? i : nvec - 1];
    }
    load_w(wk);  // Wk <= S: every wave owns a slice
    if constexpr (SMQ != kSmoothNone) {
#pragma unroll
      for (int u = 0; u < NPT; ++u) xv[u] = div_piece_bf16(xv[u], gv[u]);
    } else if (a.fu.norm_w != nullptr) {
      // RMSNorm of the token (the unfused rmsnorm_kernel's roundings)
      float ss = 0.f;
#pragma unroll
      for (int u = 0; u < NPT; ++u)
        ss = sumsq_piece(xv[u], threadIdx.x + u * (int)blockDim.x < nvec, ss);
      ss = wave_sum(ss);
      if (lane == 0) wmax[wave] = ss;
      __syncthreads();
      float t = 0.f;
      for (int q = 0; q < nw; ++q) t += wmax[q];
      const float rn = rsqrtf(t / (float)K + a.fu.eps);
#pragma unroll
      for (int u = 0; u < NPT; ++u) xv[u] = rmsnorm_piece(xv[u], gv[u], rn);
      __syncthreads();  // wmax is reused for the amax below
    }
    // amax over K bf16, then quantise into LDS (int8_quant_per_token_kernel's arithmetic)
    float st;
    if constexpr (SMQ == kSmoothStatic) {
      st = bf16_to_f32(a.xs[0]);
    } else {
      float m = 0.f;
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const bool ok = threadIdx.x + u * (int)blockDim.x < nvec;
        const uint4 v = ok ? xv[u] : make_uint4(0u, 0u, 0u, 0u);
        m = bf16_abs_max2(v.x, m);
        m = bf16_abs_max2(v.y, m);
        m = bf16_abs_max2(v.z, m);
        m = bf16_abs_max2(v.w, m);
      }
      m = wave_max(m);
      if (lane == 0) wmax[wave] = m;
      __syncthreads();
      float amax = wmax[0];
      for (int w = 1; w < nw; ++w) amax = fmaxf(amax, wmax[w]);
      st = SMQ == kSmoothDyn ? token_scale_default_eps(amax) : token_scale(amax);
    }
    const float rs = round_bf16(1.f / st);
    uint2* xq = reinterpret_cast<uint2*>(xl);
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      if (i < nvec) xq[i] = quant8(xv[u], rs);
    }
    __syncthreads();
    sx[0] = st;
  } else {
    load_w(wk);
#pragma unroll
    for (int m = 0; m < MT; ++m) sx[m] = bf16_to_f32(a.xs[m < a.M ? m : a.M - 1]);
  }

  for (int s = wk; s < S; s += Wk) {
    if (s != wk) load_w(s);
    const int c = s * 64 + lane;
    const bool cval = c < nchunk;
    const int cc = cval ? c : nchunk - 1;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      uint4 xv;
      if constexpr (FQ) {
        xv = xl[cc];
      } else {
        const int mm = m < a.M ? m : a.M - 1;
        xv = reinterpret_cast<const uint4*>(a.x)[(size_t)mm * nchunk + cc];
      }
      const uint32_t keep = cval ? ~0u : 0u;  // lanes past K add exactly 0
      const uint32_t xd[4] = {xv.x & keep, xv.y & keep, xv.z & keep, xv.w & keep};
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        int d = acc[r][m];
        d = sdot4(xd[0], wv[r].x, d);
        d = sdot4(xd[1], wv[r].y, d);
        d = sdot4(xd[2], wv[r].z, d);
        d = sdot4(xd[3], wv[r].w, d);
        acc[r][m] = d;
      }
    }
  }

  int v[V];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) v[r * MT + m] = acc[r][m];
  wave_reduce_scatter<V>(v, lane);

  const WgTotal<int> t = wg_combine<V>(v[0], lds_i, lane, wk, rg, Wk);
  if constexpr (EPI == kEpiNone) {
    if (t.writer) {
      const int r = t.widx / MT, m = t.widx % MT;
      const int n = row0 + r;
      if (n < N && m < a.M) {
        // bf16(c) * x_scale, * w_scale, each rounded (intmm.py:133-137, plain_layout.py:301-315);
        // the MFMA path's Int8Dyn::epilogue
        float o = round_bf16(round_bf16((float)t.total) * sx[m]);
        o = round_bf16(o * bf16_to_f32(a.ws[n]));
        if (a.bias != nullptr) o = round_bf16(o + bf16_to_f32(a.bias[n]));
        a.y[(size_t)m * N + n] = f32_to_bf16(o);
      }
    }
  } else {
    // the linear's output of this lane's row
    const int nr = row0 + (t.widx < V ? t.widx : 0);
    float o = round_bf16(round_bf16((float)t.total) * sx[0]);
    o = round_bf16(o * bf16_to_f32(a.ws[nr < N ? nr : N - 1]));
    pair_epilogue<EPI, RPW>(o, lane, wk, Wk, row0, N, a.y, a.fu,
                            [] { flag_decode_error(kDecodeErrKvPos); });
  }
}

template <int MT, int RPW, int NPT, int EPI = kEpiNone, int SMQ = kSmoothNone>
int launch_dyn_gemv_npt(Int8DynGemvArgs a, int grid, int threads, size_t lds, hipStream_t stream) {
  launch((int8dyn_gemv_kernel<MT, RPW, NPT, EPI, SMQ>), dim3(grid), dim3(threads), lds, stream,
         a);
  return check_launch(SMQ == kSmoothDyn      ? "int8dyn_gemv_smooth_kernel"
                      : SMQ == kSmoothStatic ? "int8dyn_gemv_smooth_static_kernel"
                                             : "int8dyn_gemv_kernel");
}

// The workgroup of the fused (FQ) launch for this K: row groups doubled until the token fits the
// workgroup's registers (K <= 8 x 16 pieces x threads)
GemvLaunchShape dyn_gemv_fq_shape(int K, int wk, int g) {
  GemvLaunchShape sh = gemv_launch_shape(K / 16, wk, g);
  while (64 * sh.Wk * sh.G * 8 * 16 < K && sh.Wk * sh.G * 2 <= 8) sh.G *= 2;
  return sh;
}

// SmoothQuant prologue: the factor's pieces sit beside the token's, as the norm's do, so the
// deepest instantiation is 8 pieces per thread (16 would go to scratch); a longer K is the two
// launches (tao_int8_smooth_linear_fused).
constexpr int kSmoothMaxNPT = 8;

template <int MT, int RPW, bool FQ, int EPI = kEpiNone, int SMQ = kSmoothNone>
int launch_dyn_gemv(Int8DynGemvArgs a, int wk, int g, hipStream_t stream) {
  const GemvLaunchShape sh = FQ ? dyn_gemv_fq_shape(a.K, wk, g) : gemv_launch_shape(a.K / 16, wk, g);
  a.S = sh.S;
  a.Wk = sh.Wk;
  a.G = sh.G;
  const int rows_per_wg = a.G * RPW;
  const int grid = (a.N + rows_per_wg - 1) / rows_per_wg;
  const int nw = a.G * a.Wk;
  const int threads = 64 * nw;
  if (!FQ) {
    const size_t lds = (size_t)nw * RPW * MT * sizeof(int);
    return launch_dyn_gemv_npt<MT, RPW, 0>(a, grid, threads, lds, stream);
  }
  if constexpr (FQ) {
    const size_t lds = (((size_t)nw * RPW * MT + 8 + 3) & ~(size_t)3) * sizeof(int) + (size_t)a.K;
    const int per = (a.K / 8 + threads - 1) / threads;  // pieces per thread
    if (per <= 1) return launch_dyn_gemv_npt<MT, RPW, 1, EPI, SMQ>(a, grid, threads, lds, stream);
    if (per <= 2) return launch_dyn_gemv_npt<MT, RPW, 2, EPI, SMQ>(a, grid, threads, lds, stream);
    if (per <= 4) return launch_dyn_gemv_npt<MT, RPW, 4, EPI, SMQ>(a, grid, threads, lds, stream);
    if (per <= 8) return launch_dyn_gemv_npt<MT, RPW, 8, EPI, SMQ>(a, grid, threads, lds, stream);
    if constexpr (SMQ == kSmoothNone) {
      if (a.fu.norm_w == nullptr && per <= 16)  // (the norm's weight pieces double the registers)
        return launch_dyn_gemv_npt<MT, RPW, 16, EPI>(a, grid, threads, lds, stream);
    }
    TAO_CHECK_ARG(false, "int8 dyn linear: K (%d) too long for the token prologue", a.K);
  }
  return TAO_OK;
}

// M == 1 shape (experiments/sweep_int8.py, profiles/r1_sweep_int8.jsonl, fused path):
// K <= 4096: 4 rows per wave, 2 waves along K, 2 row groups (one for the 128256-row head);
// longer K: 8 rows per wave, 4 waves along K (4096x14336 11.5 us).
struct DynM1Shape {
  int rpw, wk, g;
};
DynM1Shape dyn_m1_shape(int N, int K) {
  const int S = (K / 16 + 63) / 64;
  DynM1Shape s{4, S < 2 ? S : 2, N >= 65536 ? 1 : 2};
  if (S > 4) s = DynM1Shape{8, 4, 1};
  const int trpw = tao::tuning().i8_rpw;
  const int twk = tao::tuning().i8_wk;
  const int tg = tao::tuning().i8_g;
  if (trpw > 0) s.rpw = trpw;
  if (twk > 0) s.wk = twk;
  if (tg > 0) s.g = tg;
  return s;
}

template <bool FQ, int EPI = kEpiNone, int SMQ = kSmoothNone>
int dyn_gemv_m1(Int8DynGemvArgs a, hipStream_t stream) {
  const DynM1Shape s = dyn_m1_shape(a.N, a.K);
  if (s.rpw == 2) return launch_dyn_gemv<1, 2, FQ, EPI, SMQ>(a, s.wk, s.g, stream);
  if (s.rpw == 8) return launch_dyn_gemv<1, 8, FQ, EPI, SMQ>(a, s.wk, s.g, stream);
  return launch_dyn_gemv<1, 4, FQ, EPI, SMQ>(a, s.wk, s.g, stream);
}

// Whether the SmoothQuant one-token launch serves this K on the M == 1 shape: the token and the
// factor fit kSmoothMaxNPT pieces per thread.
bool smooth_m1_fits(int N, int K) {
  const DynM1Shape s = dyn_m1_shape(N, K);
  const GemvLaunchShape sh = dyn_gemv_fq_shape(K, s.wk, s.g);
  const int threads = 64 * sh.Wk * sh.G;
  return (K / 8 + threads - 1) / threads <= kSmoothMaxNPT;
}

int int8dyn_gemv(Int8DynGemvArgs a, hipStream_t stream) {
  const int S = (a.K / 16 + 63) / 64;
  const int wk = S < 8 ? S : 8, g = (8 / wk) > 0 ? 8 / wk : 1;
  if (a.M <= 1) return dyn_gemv_m1<false>(a, stream);
  if (a.M <= 2) return launch_dyn_gemv<2, 4, false>(a, wk, g, stream);
  return launch_dyn_gemv<4, 2, false>(a, wk, g, stream);
}

// ---- per-token quantisation ------------------------------------------------------------------
constexpr int kQBlock = 256;

__global__ __launch_bounds__(kQBlock) void int8_quant_per_token_kernel(
    const uint16_t* __restrict__ x, int8_t* __restrict__ q, uint16_t* __restrict__ scale, int K) {
  __shared__ float wmax[kQBlock / 64];
  const int row = blockIdx.x;
  const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * K);
  const int nvec = K / 8;  // 8 bf16 per 16-B vector
  float m = 0.f;
  for (int i = threadIdx.x; i < nvec; i += kQBlock) {
    const uint4 v = xr[i];
    m = bf16_abs_max2(v.x, m);
    m = bf16_abs_max2(v.y, m);
    m = bf16_abs_max2(v.z, m);
    m = bf16_abs_max2(v.w, m);
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  float amax = wmax[0];
#pragma unroll
  for (int w = 1; w < kQBlock / 64; ++w) amax = fmaxf(amax, wmax[w]);

  // scale = clamp(bf16(amax / 127), min = 1e-5) in bf16 (quant_primitives.py:1548-1554 with
  // quant range [-127, 127]); the clamp minimum is compared after bf16 rounding.
  const float s = token_scale(amax);
  if (threadIdx.x == 0) scale[row] = f32_to_bf16(s);
  // q = clamp(round(bf16(x * bf16(1/s))), -127, 127)  (quant_primitives.py:449-453)
  const float r = round_bf16(1.f / s);
  uint2* qr = reinterpret_cast<uint2*>(q + (size_t)row * K);
  for (int i = threadIdx.x; i < nvec; i += kQBlock) qr[i] = quant8(xr[i], r);
}

// One wave per token for K <= 64 * 8 * NV (the prefill shapes): the wave's 16-B pieces of the
// token stay in registers between the amax and the quantisation, so the token is read once
// (the block kernel above re-reads it after its barrier: a second dependent round trip) and the
// amax is a DPP wave reduction with no LDS barrier. Same arithmetic, bit-identical output.
// 4 tokens per 256-thread workgroup.
constexpr int kQWaves = 4;
template <int NV>
__global__ __launch_bounds__(64 * kQWaves) void int8_quant_per_token_wave_kernel(
    const uint16_t* __restrict__ x, int8_t* __restrict__ q, uint16_t* __restrict__ scale, int M,
    int K) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kQWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= M) return;  // wave-uniform
  const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * K);
  const int nvec = K / 8;
  uint4 v[NV];
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int i = lane + 64 * u;
    v[u] = xr[i < nvec ? i : nvec - 1];  // clamped duplicates do not change the max
  }
  float m = 0.f;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    m = bf16_abs_max2(v[u].x, m);
    m = bf16_abs_max2(v[u].y, m);
    m = bf16_abs_max2(v[u].z, m);
    m = bf16_abs_max2(v[u].w, m);
  }
  m = wave_max(m);
  const float s = token_scale(m);
  if (lane == 0) scale[row] = f32_to_bf16(s);
  const float r = round_bf16(1.f / s);
  uint2* qr = reinterpret_cast<uint2*>(q + (size_t)row * K);
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int i = lane + 64 * u;
    if (i < nvec) qr[i] = quant8(v[u], r);
  }
}

int launch_quant_per_token(const uint16_t* x, int8_t* q, uint16_t* scale, int M, int K,
                           hipStream_t stream) {
  const int nv = (K / 8 + 63) / 64;
  const dim3 grid((unsigned)((M + kQWaves - 1) / kQWaves)), block(64 * kQWaves);
  if (tuning().quant_block == 0) {
    if (nv <= 2) {
      launch(int8_quant_per_token_wave_kernel<2>, grid, block, 0, stream, x, q, scale, M, K);
      return check_launch("int8_quant_per_token_wave_kernel");
    }
    if (nv <= 4) {
      launch(int8_quant_per_token_wave_kernel<4>, grid, block, 0, stream, x, q, scale, M, K);
      return check_launch("int8_quant_per_token_wave_kernel");
    }
    if (nv <= 8) {
      launch(int8_quant_per_token_wave_kernel<8>, grid, block, 0, stream, x, q, scale, M, K);
      return check_launch("int8_quant_per_token_wave_kernel");
    }
    if (nv <= 16) {
      launch(int8_quant_per_token_wave_kernel<16>, grid, block, 0, stream, x, q, scale, M, K);
      return check_launch("int8_quant_per_token_wave_kernel");
    }
  }
  launch(int8_quant_per_token_kernel, dim3((unsigned)M), dim3(kQBlock), 0, stream, x, q, scale,
         K);
  return check_launch("int8_quant_per_token_kernel");
}

// ---- SmoothQuant: fused smooth + quantise ----------------------------------------------------
// t = bf16(x / smooth) (div_piece_bf16: tao_act_prescale_bf16's bits), then the amax, scale and
// codes of to_affine_quantized_intx(t, SYMMETRIC, per token, int8, quant_min=-127) with its
// default eps (token_scale_default_eps). The token and the factor are read once and t stays in
// registers. Both shapes of the plain quantizer above: one wave per token for K <= 64 * 8 * NV ...
template <int NV>
__global__ __launch_bounds__(64 * kQWaves) void int8_smooth_quant_wave_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ smooth, int8_t* __restrict__ q,
    uint16_t* __restrict__ scale, int M, int K) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kQWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= M) return;  // wave-uniform
  const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * K);
  const uint4* sr = reinterpret_cast<const uint4*>(smooth);
  const int nvec = K / 8;
  uint4 v[NV], g[NV];
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int i = lane + 64 * u;
    const int ic = i < nvec ? i : nvec - 1;  // clamped duplicates do not change the max
    v[u] = xr[ic];
    g[u] = sr[ic];
  }
  float m = 0.f;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    v[u] = div_piece_bf16(v[u], g[u]);
    m = bf16_abs_max2(v[u].x, m);
    m = bf16_abs_max2(v[u].y, m);
    m = bf16_abs_max2(v[u].z, m);
    m = bf16_abs_max2(v[u].w, m);
  }
  m = wave_max(m);
  const float s = token_scale_default_eps(m);
  if (lane == 0) scale[row] = f32_to_bf16(s);
  const float r = round_bf16(1.f / s);
  uint2* qr = reinterpret_cast<uint2*>(q + (size_t)row * K);
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int i = lane + 64 * u;
    if (i < nvec) qr[i] = quant8(v[u], r);
  }
}

// ... and one workgroup of T threads per token for longer K, 8 pieces per thread (K <= 64 T):
// the wave maxima cross through LDS, the pieces still stay in registers.
constexpr int kSmoothBlockNP = 8;
template <int T>
__global__ __launch_bounds__(T) void int8_smooth_quant_block_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ smooth, int8_t* __restrict__ q,
    uint16_t* __restrict__ scale, int K) {
  __shared__ float wmax[T / 64];
  const int row = blockIdx.x;
  const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * K);
  const uint4* sr = reinterpret_cast<const uint4*>(smooth);
  const int nvec = K / 8;
  uint4 v[kSmoothBlockNP];
  float m = 0.f;
#pragma unroll
  for (int u = 0; u < kSmoothBlockNP; ++u) {
    const int i = threadIdx.x + T * u;
    const int ic = i < nvec ? i : nvec - 1;
    v[u] = div_piece_bf16(xr[ic], sr[ic]);
    m = bf16_abs_max2(v[u].x, m);
    m = bf16_abs_max2(v[u].y, m);
    m = bf16_abs_max2(v[u].z, m);
    m = bf16_abs_max2(v[u].w, m);
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  float amax = wmax[0];
#pragma unroll
  for (int w = 1; w < T / 64; ++w) amax = fmaxf(amax, wmax[w]);
  const float s = token_scale_default_eps(amax);
  if (threadIdx.x == 0) scale[row] = f32_to_bf16(s);
  const float r = round_bf16(1.f / s);
  uint2* qr = reinterpret_cast<uint2*>(q + (size_t)row * K);
#pragma unroll
  for (int u = 0; u < kSmoothBlockNP; ++u) {
    const int i = threadIdx.x + T * u;
    if (i < nvec) qr[i] = quant8(v[u], r);
  }
}

// Static activation quantisation (_ActQuantizer.static_quantize: to_affine_quantized_intx_static
// with one scale for the whole tensor): q = clamp(rint(bf16(t * bf16(1 / s))), -127, 127), s read
// from device memory. Element-wise: no reduction, no barrier; a thread keeps the factor's piece
// across the rows blockIdx.y walks. scale[m] = s for every row, the per-row vector
// tao_int8_scaled_mm_bf16 takes.
__global__ __launch_bounds__(256) void int8_smooth_quant_static_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ smooth,
    const uint16_t* __restrict__ act_scale, uint2* __restrict__ q, uint16_t* __restrict__ scale,
    int M, int nx) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= nx) return;
  const uint16_t sb = act_scale[0];
  const float r = round_bf16(1.f / bf16_to_f32(sb));
  const uint4 sv = smooth[i];
  for (int m = (int)blockIdx.y; m < M; m += (int)gridDim.y) {
    const size_t o = (size_t)m * nx + i;
    q[o] = quant8(div_piece_bf16(x[o], sv), r);
    if (i == 0) scale[m] = sb;
  }
}

int launch_smooth_quant(const uint16_t* x, const uint16_t* smooth, const uint16_t* act_scale,
                        int8_t* q, uint16_t* scale, int M, int K, hipStream_t stream) {
  if (act_scale != nullptr) {
    const int nx = K / 8;
    const unsigned rows = (unsigned)(M < 1024 ? M : 1024);
    launch(int8_smooth_quant_static_kernel, dim3((unsigned)((nx + 255) / 256), rows), dim3(256), 0,
           stream, reinterpret_cast<const uint4*>(x), reinterpret_cast<const uint4*>(smooth),
           act_scale, reinterpret_cast<uint2*>(q), scale, M, nx);
    return check_launch("int8_smooth_quant_static_kernel");
  }
  const int nv = (K / 8 + 63) / 64;
  const dim3 grid((unsigned)((M + kQWaves - 1) / kQWaves)), block(64 * kQWaves);
  if (nv <= 16) {
    if (nv <= 2)
      launch(int8_smooth_quant_wave_kernel<2>, grid, block, 0, stream, x, smooth, q, scale, M, K);
    else if (nv <= 4)
      launch(int8_smooth_quant_wave_kernel<4>, grid, block, 0, stream, x, smooth, q, scale, M, K);
    else if (nv <= 8)
      launch(int8_smooth_quant_wave_kernel<8>, grid, block, 0, stream, x, smooth, q, scale, M, K);
    else
      launch(int8_smooth_quant_wave_kernel<16>, grid, block, 0, stream, x, smooth, q, scale, M, K);
    return check_launch("int8_smooth_quant_wave_kernel");
  }
  if (K <= 64 * 256)
    launch(int8_smooth_quant_block_kernel<256>, dim3((unsigned)M), dim3(256), 0, stream, x, smooth,
           q, scale, K);
  else  // K <= 65536, checked by the caller
    launch(int8_smooth_quant_block_kernel<1024>, dim3((unsigned)M), dim3(1024), 0, stream, x,
           smooth, q, scale, K);
  return check_launch("int8_smooth_quant_block_kernel");
}

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_int8_quant_per_token(const uint16_t* x, int8_t* q, uint16_t* scale, int64_t M,
                             int64_t K, void* stream) {
  TAO_CHECK_ARG(M >= 0 && K >= 0, "int8 quant: negative size");
  TAO_CHECK_ARG(K % 16 == 0, "int8 quant: K (%lld) must be a multiple of 16", (long long)K);
  TAO_CHECK_ARG(M < (1LL << 31) && K < (1LL << 31), "int8 quant: size out of range");
  if (M == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(q, 8, "q");
  return launch_quant_per_token(x, q, scale, (int)M, (int)K, as_stream(stream));
}

// per-token quant kernel choice (A/B only): 0 = one wave per token (default), 1 = the
// 256-thread block kernel
int tao_tune_int8_quant(int block) {
  TAO_CHECK_ARG(block == 0 || block == 1, "tune: int8 quant block must be 0 or 1");
  tuning().quant_block = block;
  return TAO_OK;
}

int tao_int8_scaled_mm_bf16(const int8_t* xq, const uint16_t* xs, const int8_t* wq,
                            const uint16_t* ws, const uint16_t* bias, uint16_t* y, int64_t M,
                            int64_t N, int64_t K, void* stream) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "int8 scaled mm: negative size");
  TAO_CHECK_ARG(K % 16 == 0, "int8 scaled mm: K (%lld) must be a multiple of 16", (long long)K);
  TAO_CHECK_ARG(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31),
                "int8 scaled mm: size out of range");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "int8 scaled mm: K must be > 0");
  TAO_CHECK_ALIGN(xq, 16, "xq");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  if (M <= 4) {
    Int8DynGemvArgs a{xq, xs, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                      (int)M, (int)N, (int)K, 0, 0, 0};
    return int8dyn_gemv(a, as_stream(stream));
  }
  return int8_scaled_mm_launch(xq, xs, wq, ws, bias, y, (int)M, (int)N, (int)K,
                               as_stream(stream));
}

int tao_int8_dyn_linear_bf16(const uint16_t* x, const int8_t* wq, const uint16_t* ws,
                             const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                             void* stream) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "int8 dyn linear: negative size");
  TAO_CHECK_ARG(M <= 1, "int8 dyn linear: the fused path is one token (M <= 1, got %lld)",
                (long long)M);
  TAO_CHECK_ARG(K % 16 == 0, "int8 dyn linear: K (%lld) must be a multiple of 16", (long long)K);
  TAO_CHECK_ARG(K <= 65536, "int8 dyn linear: K (%lld) must be <= 65536 (token in LDS)",
                (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31), "int8 dyn linear: size out of range");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "int8 dyn linear: K must be > 0");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  Int8DynGemvArgs a{x, nullptr, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                    1, (int)N, (int)K, 0, 0, 0};
  return dyn_gemv_m1<true>(a, as_stream(stream));
}

int tao_int8_smooth_quant_bf16(const uint16_t* x, const uint16_t* smooth,
                               const uint16_t* act_scale, int8_t* q, uint16_t* scale, int64_t M,
                               int64_t K, void* stream) {
  TAO_CHECK_ARG(M >= 0 && K >= 0, "int8 smooth quant: negative size");
  TAO_CHECK_ARG(K % 16 == 0, "int8 smooth quant: K (%lld) must be a multiple of 16",
                (long long)K);
  TAO_CHECK_ARG(M < (1LL << 31) && K <= 65536,
                "int8 smooth quant: M must be < 2^31 and K (%lld) <= 65536", (long long)K);
  if (M == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ARG(x != nullptr && smooth != nullptr && q != nullptr && scale != nullptr,
                "int8 smooth quant: x, smooth, q and scale are required");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(smooth, 16, "smooth");
  TAO_CHECK_ALIGN(q, 8, "q");
  return launch_smooth_quant(x, smooth, act_scale, q, scale, (int)M, (int)K, as_stream(stream));
}

// The M == 1 routing, measured (experiments/bench_smoothquant.py, profiles/smoothquant_bench.jsonl,
// smoothquant_bench_boundary.jsonl; us per linear, one launch vs two launches).
// Dynamic: the one launch wins wherever it fits (4096^2 6.4 vs 9.4, 4096x14336 14.8 vs 16.8,
// 4096x16384 16.1 vs 18.4). Static: the two-launch form has no reduction to wait for, and past
// K = 8192 every workgroup's own division of the whole token costs more than the saved launch
// (4096x8192 9.05 vs 9.43, 4096x11008 13.2 vs 12.9, 4096x14336 14.5 vs 13.2, 4096x16384 16.7 vs
// 14.5): one launch up to K = 8192.
int tao_int8_smooth_linear_fused(int64_t M, int64_t N, int64_t K, int is_static) {
  if (M != 1 || N <= 0 || N >= (1LL << 31) || K <= 0 || K % 16 != 0 || K > 65536) return 0;
  if (is_static && K > 8192) return 0;
  return smooth_m1_fits((int)N, (int)K) ? 1 : 0;
}

int tao_int8_smooth_linear_bf16(const uint16_t* x, const uint16_t* smooth,
                                const uint16_t* act_scale, const int8_t* wq, const uint16_t* ws,
                                const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                                int64_t K, void* stream) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "int8 smooth linear: negative size");
  TAO_CHECK_ARG(M <= 1, "int8 smooth linear: the fused path is one token (M <= 1, got %lld)",
                (long long)M);
  TAO_CHECK_ARG(K % 16 == 0, "int8 smooth linear: K (%lld) must be a multiple of 16",
                (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31), "int8 smooth linear: size out of range");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "int8 smooth linear: K must be > 0");
  TAO_CHECK_ARG(K <= 65536 && smooth_m1_fits((int)N, (int)K),
                "int8 smooth linear: K (%lld) too long for the one launch: "
                "tao_int8_smooth_quant_bf16 then tao_int8_scaled_mm_bf16", (long long)K);
  TAO_CHECK_ARG(x != nullptr && smooth != nullptr && wq != nullptr && ws != nullptr &&
                    y != nullptr,
                "int8 smooth linear: x, smooth, wq, ws and y are required");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(smooth, 16, "smooth");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  Int8DynGemvArgs a{x, act_scale, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                    1, (int)N, (int)K, 0, 0, 0};
  a.fu.norm_w = smooth;
  if (act_scale != nullptr) return dyn_gemv_m1<true, kEpiNone, kSmoothStatic>(a, as_stream(stream));
  return dyn_gemv_m1<true, kEpiNone, kSmoothDyn>(a, as_stream(stream));
}

int tao_int8dq_decode_bf16(const uint16_t* x, const int8_t* wq, const uint16_t* ws, int64_t N,
                           int64_t K, const uint16_t* norm_weight, float eps, int epilogue,
                           uint16_t* y, const float* freqs, const int64_t* pos, uint16_t* k_cache,
                           uint16_t* v_cache, int64_t n_head, int64_t n_kv_head, int64_t head_dim,
                           int64_t max_seq, void* stream) {
  TAO_CHECK_ARG(N >= 0 && K > 0 && K % 16 == 0 && K <= 32768 && N < (1LL << 31),
                "int8dq decode: K (%lld) must be a positive multiple of 16, <= 32768",
                (long long)K);
  int rc = check_decode_epilogue("int8dq decode", epilogue, N);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  Int8DynGemvArgs a{x, nullptr, reinterpret_cast<const uint4*>(wq), ws, nullptr, y,
                    1, (int)N, (int)K, 0, 0, 0};
  if (norm_weight != nullptr) TAO_CHECK_ALIGN(norm_weight, 16, "norm_weight");
  rc = check_decode_fuse("int8dq decode", epilogue, N, norm_weight, eps, y, freqs, pos, k_cache,
                         v_cache, n_head, n_kv_head, head_dim, max_seq, &a.fu);
  if (rc != TAO_OK) return rc;
  if (N == 0) return TAO_OK;
  const hipStream_t st = as_stream(stream);
  return dispatch_epilogue(
      epilogue, [&](auto epi) { return dyn_gemv_m1<true, decltype(epi)::value>(a, st); });
}

int tao_tune_int8_gemv(int rows_per_wave, int waves_k, int row_groups) {
  TAO_CHECK_ARG(rows_per_wave == 0 || rows_per_wave == 2 || rows_per_wave == 4 ||
                    rows_per_wave == 8,
                "tune: rows_per_wave must be 0 (auto), 2, 4 or 8");
  TAO_CHECK_ARG(waves_k >= 0 && row_groups >= 0 && waves_k * (row_groups ? row_groups : 1) <= 8,
                "tune: waves_k * row_groups must be <= 8");
  tao::tuning().i8_rpw = rows_per_wave;
  tao::tuning().i8_wk = waves_k;
  tao::tuning().i8_g = row_groups;
  return TAO_OK;
}

}  // extern "C"
