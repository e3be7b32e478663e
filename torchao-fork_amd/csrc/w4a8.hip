// W4A8 linear: int8 dynamic per-token activations x int4 per-channel weights packed two per byte
// (Int8DynamicActivationInt4WeightConfig(layout=CutlassInt4PackedLayout())), all-integer product:
//   acc[m][n] = sum_k xq[m][k] * wq[n][k]                  (exact int32)
//   y[m][n]   = bf16( fp32(acc) * xs[m] * ws[n] + fp32(bias[n]) )
//   1. tao_int8_quant_per_token_f32: x bf16 [M][K] -> (q int8 [M][K], s fp32 [M]), replacing
//      _int8_symm_cutlass_quant (torchao/quantization/quant_api.py:1299-1308);
//   2. tao_int4_quantize_rows_packed_bf16: w bf16 [N][K] -> (packed nibbles [N][K/2], s fp32 [N]),
//      replacing _int4_symm_cutlass_quant (quant_api.py:1311-1323) and the layout's from_plain;
//   3. tao_w4a8_scaled_mm_bf16: replaces torchao::rowwise_scaled_linear_cutlass_s8s4
//      (torchao/dtypes/uintx/cutlass_int4_packed_layout.py:176-189), which the reference builds
//      for sm80 only. M <= 2, and M <= 4 on weights of at most 32 Mi elements: w4a8_gemv_kernel
//      below; above: the Int8DynW4 instance of gemm_mfma_kernel (gemm_mfma_policy.h);
//   4. tao_w4a8_dyn_linear_bf16 (M == 1): 1 + 3 in one launch, int8dyn_gemv_kernel's scheme.
// Storage is the reference's: byte j of a row holds element 2 j in its low nibble and element
// 2 j + 1 in its high nibble. Nothing is reordered in memory.
//
// Nibble expansion: for a dword w of eight nibbles, (w << 4) & 0xF0F0F0F0 and w & 0xF0F0F0F0 are
// the even and the odd elements times 16 as int8 lanes (the nibble's sign bit lands on the byte's):
// two VALU operations per eight weights, no sign extension. The x codes are paired the same way
// (even elements in one dword, odd in the next). The factor 16 is exact and leaves the int32 sum by
// an arithmetic shift: |16 acc| <= 16 * 8 * 128 * K = 16384 K < 2^31 for K < 131072, checked.
#include "int8_quant_row.h"
#include "tao_gemm.h"
#include "tao_gemv.h"
#include "w4a8_quant_row.h"

// The epilogue is specified as separate fp32 roundings (mul, mul, add): no fused multiply-add.
#pragma clang fp contract(off)

namespace tao {
namespace {

constexpr int kW4MaxK = 131072;  // exclusive: the x16 sum stays inside int32 below it

// ---- W4A8 GEMV (decode) -------------------------------------------------------------------------
// The byte-weight decomposition of tao_gemv.h: a 16-B chunk is 32 k of one row, a slice 2048 k.
// Per lane and row: the chunk's four dwords expanded to eight int8 dwords and eight v_dot4_i32_i8
// into an int32 accumulator. Every partial sum is an exact integer, so no reduction order can
// change a bit. Lanes past K read a clamped in-bounds chunk and a zeroed x, adding exactly 0.
//
// FQ (M == 1): x is the bf16 token. Each workgroup first issues its first slice's weight loads,
// then quantises the token into LDS with the per-token quantizer's exact arithmetic
// (w4a8_quant_row.h) under their latency, storing each 8-k group de-interleaved (w4a8_quant8_eo).
// Without FQ the int8 codes come from memory in element order and are de-interleaved in registers,
// two v_perm_b32 per 8 k, shared by the wave's rows.
struct W4A8GemvArgs {
  const void* x;          // int8 q [M][K] (FQ: bf16 token [K])
  const float* xs;        // [M] per-token scales (FQ: unused)
  const uint4* w;         // [N][K/32]
  const float* ws;        // [N]
  const uint16_t* bias;   // [N] or null
  uint16_t* y;            // [M][N]
  int M, N, K, Wk, G, S;
};

__device__ __forceinline__ int sdot4(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}

constexpr uint32_t kNibHi = 0xF0F0F0F0u;

template <int MT, int RPW, int NPT>
__global__ __launch_bounds__(512) void w4a8_gemv_kernel(W4A8GemvArgs a) {
  constexpr bool FQ = NPT > 0;  // NPT: 16-B pieces of the bf16 token per thread (K <= 8 NPT T)
  static_assert(!FQ || MT == 1, "the fused quantisation is per token, M == 1");
  constexpr int V = RPW * MT;
  // [G][Wk][V] int partials | (FQ) [8] wave maxima | (FQ) token q [K] int8, de-interleaved
  extern __shared__ int lds_i[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % a.Wk;
  const int rg = wave / a.Wk;
  const int row0 = (blockIdx.x * a.G + rg) * RPW;
  const int K = a.K, N = a.N, S = a.S, Wk = a.Wk;
  const int nchunk = K >> 5;  // 16-B (32-k) chunks per row
  const int nw = a.G * a.Wk;
  float* wmax = reinterpret_cast<float*>(lds_i + nw * V);
  uint4* xl = reinterpret_cast<uint4*>(lds_i + ((nw * V + 8 + 3) & ~3));

  int acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0;

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

  float sx[MT];
  if constexpr (FQ) {
    // The token's pieces are loaded BEFORE the first slice's weights: vector loads retire in
    // issue order, so the wait for x does not wait for the weights.
    const uint4* xr = reinterpret_cast<const uint4*>(a.x);
    const int nvec = K >> 3;
    uint4 xv[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      xv[u] = xr[i < nvec ? i : nvec - 1];  // clamped, masked below
    }
    load_w(wk);  // Wk <= S: every wave owns a slice
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
    const float st = cutlass_row_scale(amax, kW4A8ActHalf);
    const float rs = 1.f / st;
    uint2* xq = reinterpret_cast<uint2*>(xl);
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      if (i < nvec) xq[i] = w4a8_quant8_eo(xv[u], rs);
    }
    __syncthreads();
    sx[0] = st;
  } else {
    load_w(wk);
#pragma unroll
    for (int m = 0; m < MT; ++m) sx[m] = a.xs[m < a.M ? m : a.M - 1];
  }

  for (int s = wk; s < S; s += Wk) {
    if (s != wk) load_w(s);
    const int c = s * 64 + lane;
    const bool cval = c < nchunk;
    const int cc = cval ? c : nchunk - 1;
    const uint32_t keep = cval ? ~0u : 0u;  // lanes past K add exactly 0
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      // xe[g] / xo[g]: the even / odd elements of the chunk's 8-k group g
      uint32_t xe[4], xo[4];
      if constexpr (FQ) {
        const uint4 p = xl[2 * cc], q = xl[2 * cc + 1];
        xe[0] = p.x & keep, xo[0] = p.y & keep, xe[1] = p.z & keep, xo[1] = p.w & keep;
        xe[2] = q.x & keep, xo[2] = q.y & keep, xe[3] = q.z & keep, xo[3] = q.w & keep;
      } else {
        const int mm = m < a.M ? m : a.M - 1;
        const uint4* xp = reinterpret_cast<const uint4*>(a.x) + ((size_t)mm * nchunk + cc) * 2;
        const uint4 p = xp[0], q = xp[1];
        const uint32_t d[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          xe[g] = __builtin_amdgcn_perm(d[2 * g + 1], d[2 * g], 0x06040200u) & keep;
          xo[g] = __builtin_amdgcn_perm(d[2 * g + 1], d[2 * g], 0x07050301u) & keep;
        }
      }
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const uint32_t wd[4] = {wv[r].x, wv[r].y, wv[r].z, wv[r].w};
        int d = acc[r][m];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          d = sdot4(xe[g], (wd[g] << 4) & kNibHi, d);
          d = sdot4(xo[g], wd[g] & kNibHi, d);
        }
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
  if (t.writer) {
    const int r = t.widx / MT, m = t.widx % MT;
    const int n = row0 + r;
    if (n < N && m < a.M) {
      // the x16 of the expansion leaves exactly; then the MFMA path's Int8DynW4::epi
      float o = ((float)(t.total >> 4) * sx[m]) * a.ws[n];
      if (a.bias != nullptr) o = o + bf16_to_f32(a.bias[n]);
      a.y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

template <int MT, int RPW, int NPT>
int launch_w4a8_gemv_npt(W4A8GemvArgs a, int grid, int threads, size_t lds, hipStream_t stream) {
  launch((w4a8_gemv_kernel<MT, RPW, NPT>), dim3(grid), dim3(threads), lds, stream, a);
  return check_launch("w4a8_gemv_kernel");
}

template <int MT, int RPW, bool FQ>
int launch_w4a8_gemv(W4A8GemvArgs a, int wk, int g, hipStream_t stream) {
  GemvLaunchShape sh = gemv_launch_shape(a.K / 32, wk, g);
  // FQ: row groups doubled until the token fits the workgroup's registers (K <= 8 x 16 x threads)
  while (FQ && 64 * sh.Wk * sh.G * 8 * 16 < a.K && sh.Wk * sh.G * 2 <= 8) sh.G *= 2;
  a.S = sh.S;
  a.Wk = sh.Wk;
  a.G = sh.G;
  const int rows_per_wg = a.G * RPW;
  const int grid = (a.N + rows_per_wg - 1) / rows_per_wg;
  const int nw = a.G * a.Wk;
  const int threads = 64 * nw;
  if (!FQ) {
    const size_t lds = (size_t)nw * RPW * MT * sizeof(int);
    return launch_w4a8_gemv_npt<MT, RPW, 0>(a, grid, threads, lds, stream);
  }
  if constexpr (FQ) {
    const size_t lds = (((size_t)nw * RPW * MT + 8 + 3) & ~(size_t)3) * sizeof(int) + (size_t)a.K;
    const int per = (a.K / 8 + threads - 1) / threads;  // pieces per thread
    if (per <= 1) return launch_w4a8_gemv_npt<MT, RPW, 1>(a, grid, threads, lds, stream);
    if (per <= 2) return launch_w4a8_gemv_npt<MT, RPW, 2>(a, grid, threads, lds, stream);
    if (per <= 4) return launch_w4a8_gemv_npt<MT, RPW, 4>(a, grid, threads, lds, stream);
    if (per <= 8) return launch_w4a8_gemv_npt<MT, RPW, 8>(a, grid, threads, lds, stream);
    if (per <= 16) return launch_w4a8_gemv_npt<MT, RPW, 16>(a, grid, threads, lds, stream);
    TAO_CHECK_ARG(false, "w4a8 dyn linear: K (%d) too long for the token prologue", a.K);
  }
  return TAO_OK;
}

// M == 1 shape: the int8 dynamic GEMV's rule (int8_dyn.hip dyn_m1_shape) on this format's
// 2048-k slices, not re-measured: up to 4 slices 4 rows per wave, 2 waves along K, 2 row groups
// (one for a 128256-row head); longer K: 8 rows per wave, 4 waves along K. tao_tune_int8_gemv
// overrides each of the three.
template <bool FQ>
int w4a8_gemv_m1(W4A8GemvArgs a, hipStream_t stream) {
  const int S = (a.K / 32 + 63) / 64;
  int rpw = 4, wk = S < 2 ? S : 2, g = a.N >= 65536 ? 1 : 2;
  if (S > 4) rpw = 8, wk = 4, g = 1;
  if (tuning().i8_rpw > 0) rpw = tuning().i8_rpw;
  if (tuning().i8_wk > 0) wk = tuning().i8_wk;
  if (tuning().i8_g > 0) g = tuning().i8_g;
  if (rpw == 2) return launch_w4a8_gemv<1, 2, FQ>(a, wk, g, stream);
  if (rpw == 8) return launch_w4a8_gemv<1, 8, FQ>(a, wk, g, stream);
  return launch_w4a8_gemv<1, 4, FQ>(a, wk, g, stream);
}

// The GEMV serves up to 4 tokens (MT <= 4). Built-in route, measured on the scaled mm forced
// either way (experiments/bench_w4a8.py --boundary, profiles/w4a8_bench_boundary.jsonl; us, GEMV vs
// MFMA): M = 2 wins on the GEMV at every shape (4096^2 4.2 vs 5.7, 14336x4096 8.3 vs 8.8,
// 4096x14336 8.4 vs 9.5); M = 3, 4 win on it for the 16 and 24 Mi-element weights (4096^2 5.1 vs
// 5.8, 6144x4096 6.0 vs 7.1) and lose for the 56 Mi ones (14336x4096 11.5 vs 8.8, 4096x14336 13.1 vs
// 9.6): the weight-only linears' rule (use_gemv, gemm_mfma.hip). tao_tune_linear_crossover moves
// the boundary for A/B measurement (0: this rule).
constexpr int kW4GemvMaxM = 4;
bool w4a8_takes_gemv(int64_t M, int64_t N, int64_t K) {
  const int v = tuning().max_gemv_m;
  if (v > 0) return M <= (v < kW4GemvMaxM ? v : kW4GemvMaxM);
  return M <= 2 || (M <= kW4GemvMaxM && N * K <= (32LL << 20));
}

int w4a8_gemv(W4A8GemvArgs a, hipStream_t stream) {
  const int S = (a.K / 32 + 63) / 64;
  const int wk = S < 8 ? S : 8, g = (8 / wk) > 0 ? 8 / wk : 1;
  if (a.M <= 1) return w4a8_gemv_m1<false>(a, stream);
  if (a.M <= 2) return launch_w4a8_gemv<2, 4, false>(a, wk, g, stream);
  return launch_w4a8_gemv<4, 2, false>(a, wk, g, stream);
}

// ---- the two quantizers ------------------------------------------------------------------------
// One row per workgroup of T threads; PACK4: the weight quantizer (H = 7.5, [-8, 7], nibbles),
// else the token quantizer (H = 127.5, [-128, 127], bytes). The row is read twice (amax, codes).
constexpr int kQBlock = 256;

template <bool PACK4>
__global__ __launch_bounds__(kQBlock) void w4a8_quant_row_kernel(const uint16_t* __restrict__ x,
                                                                 uint8_t* __restrict__ q,
                                                                 float* __restrict__ scale,
                                                                 int K) {
  __shared__ float wmax[kQBlock / 64];
  const size_t row = blockIdx.x;
  const uint4* xr = reinterpret_cast<const uint4*>(x + row * K);
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
  const float s = cutlass_row_scale(amax, PACK4 ? kW4A8WgtHalf : kW4A8ActHalf);
  if (threadIdx.x == 0) scale[row] = s;
  const float r = 1.f / s;
  if constexpr (PACK4) {
    uint32_t* qr = reinterpret_cast<uint32_t*>(q + row * (K / 2));
    for (int i = threadIdx.x; i < nvec; i += kQBlock) qr[i] = w4a8_quant8_nib(xr[i], r);
  } else {
    uint2* qr = reinterpret_cast<uint2*>(q + row * K);
    for (int i = threadIdx.x; i < nvec; i += kQBlock) qr[i] = w4a8_quant8(xr[i], r);
  }
}

// One wave per token for K <= 64 * 8 * NV (the prefill shapes), int8_quant_per_token_wave_kernel's
// scheme (int8_dyn.hip): the token is read once and stays in registers, no LDS barrier. Same
// arithmetic, bit-identical output. 4 tokens per 256-thread workgroup.
constexpr int kQWaves = 4;
template <int NV>
__global__ __launch_bounds__(64 * kQWaves) void w4a8_quant_per_token_wave_kernel(
    const uint16_t* __restrict__ x, uint8_t* __restrict__ q, float* __restrict__ scale, int M,
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
  const float s = cutlass_row_scale(m, kW4A8ActHalf);
  if (lane == 0) scale[row] = s;
  const float r = 1.f / s;
  uint2* qr = reinterpret_cast<uint2*>(q + (size_t)row * K);
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int i = lane + 64 * u;
    if (i < nvec) qr[i] = w4a8_quant8(v[u], r);
  }
}

int launch_w4a8_quant_per_token(const uint16_t* x, int8_t* q, float* scale, int M, int K,
                                hipStream_t stream) {
  uint8_t* qb = reinterpret_cast<uint8_t*>(q);
  const int nv = (K / 8 + 63) / 64;
  const dim3 grid((unsigned)((M + kQWaves - 1) / kQWaves)), block(64 * kQWaves);
  if (nv <= 16) {
    if (nv <= 2)
      launch(w4a8_quant_per_token_wave_kernel<2>, grid, block, 0, stream, x, qb, scale, M, K);
    else if (nv <= 4)
      launch(w4a8_quant_per_token_wave_kernel<4>, grid, block, 0, stream, x, qb, scale, M, K);
    else if (nv <= 8)
      launch(w4a8_quant_per_token_wave_kernel<8>, grid, block, 0, stream, x, qb, scale, M, K);
    else
      launch(w4a8_quant_per_token_wave_kernel<16>, grid, block, 0, stream, x, qb, scale, M, K);
    return check_launch("w4a8_quant_per_token_wave_kernel");
  }
  launch(w4a8_quant_row_kernel<false>, dim3((unsigned)M), dim3(kQBlock), 0, stream, x, qb, scale,
         K);
  return check_launch("w4a8_quant_row_kernel");
}

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_int8_quant_per_token_f32(const uint16_t* x, int8_t* q, float* scale, int64_t M, int64_t K,
                                 void* stream) {
  TAO_CHECK_ARG(M >= 0 && K >= 0, "int8 quant (f32 scale): negative size");
  TAO_CHECK_ARG(K % 8 == 0, "int8 quant (f32 scale): K (%lld) must be a multiple of 8",
                (long long)K);
  TAO_CHECK_ARG(M < (1LL << 31) && K < (1LL << 31), "int8 quant (f32 scale): size out of range");
  if (M == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ARG(x != nullptr && q != nullptr && scale != nullptr,
                "int8 quant (f32 scale): x, q and scale are required");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(q, 8, "q");
  TAO_CHECK_ALIGN(scale, 4, "scale");
  return launch_w4a8_quant_per_token(x, q, scale, (int)M, (int)K, as_stream(stream));
}

int tao_int4_quantize_rows_packed_bf16(const uint16_t* w, uint8_t* q, float* scale, int64_t rows,
                                       int64_t K, void* stream) {
  TAO_CHECK_ARG(rows >= 0 && K >= 0, "int4 packed quantize: negative size");
  TAO_CHECK_ARG(K % 8 == 0, "int4 packed quantize: K (%lld) must be a multiple of 8",
                (long long)K);
  TAO_CHECK_ARG(rows < (1LL << 31) && K < (1LL << 31), "int4 packed quantize: size out of range");
  if (rows == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ARG(w != nullptr && q != nullptr && scale != nullptr,
                "int4 packed quantize: w, q and scale are required");
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(q, 4, "q");
  TAO_CHECK_ALIGN(scale, 4, "scale");
  launch(w4a8_quant_row_kernel<true>, dim3((unsigned)rows), dim3(kQBlock), 0, as_stream(stream), w,
         q, scale, (int)K);
  return check_launch("w4a8_quant_row_kernel");
}

int tao_w4a8_scaled_mm_bf16(const int8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                            const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                            void* stream) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "w4a8 scaled mm: negative size");
  TAO_CHECK_ARG(K % 32 == 0, "w4a8 scaled mm: K (%lld) must be a multiple of 32", (long long)K);
  TAO_CHECK_ARG(K < kW4MaxK, "w4a8 scaled mm: K (%lld) must be below %d (int32 sum of x16 codes)",
                (long long)K, kW4MaxK);
  TAO_CHECK_ARG(M < (1LL << 31) && N < (1LL << 31) && M * K < (1LL << 32) &&
                    N * (K / 2) < (1LL << 32),
                "w4a8 scaled mm: size out of range (each operand below 4 GiB)");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "w4a8 scaled mm: K must be > 0");
  TAO_CHECK_ARG(xq != nullptr && xs != nullptr && wq != nullptr && ws != nullptr && y != nullptr,
                "w4a8 scaled mm: xq, xs, wq, ws and y are required");
  TAO_CHECK_ALIGN(xq, 16, "xq");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  TAO_CHECK_ALIGN(xs, 4, "xs");
  TAO_CHECK_ALIGN(ws, 4, "ws");
  if (w4a8_takes_gemv(M, N, K)) {
    W4A8GemvArgs a{xq, xs, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                   (int)M, (int)N, (int)K, 0, 0, 0};
    return w4a8_gemv(a, as_stream(stream));
  }
  return w4a8_scaled_mm_launch(xq, xs, wq, ws, bias, y, (int)M, (int)N, (int)K,
                               as_stream(stream));
}

int tao_w4a8_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const float* ws,
                             const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                             void* stream) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "w4a8 dyn linear: negative size");
  TAO_CHECK_ARG(M <= 1, "w4a8 dyn linear: the fused path is one token (M <= 1, got %lld)",
                (long long)M);
  TAO_CHECK_ARG(K % 32 == 0, "w4a8 dyn linear: K (%lld) must be a multiple of 32", (long long)K);
  TAO_CHECK_ARG(K <= 65536, "w4a8 dyn linear: K (%lld) must be <= 65536 (token in LDS)",
                (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31), "w4a8 dyn linear: size out of range");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "w4a8 dyn linear: K must be > 0");
  TAO_CHECK_ARG(x != nullptr && wq != nullptr && ws != nullptr && y != nullptr,
                "w4a8 dyn linear: x, wq, ws and y are required");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(wq, 16, "wq");
  TAO_CHECK_ALIGN(ws, 4, "ws");
  W4A8GemvArgs a{x, nullptr, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                 1, (int)N, (int)K, 0, 0, 0};
  return w4a8_gemv_m1<true>(a, as_stream(stream));
}

}  // extern "C"
