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
//      v_mfma_scale_f32_16x16x128_f8f6f4; M at or below it: mx_gemv_kernel below.
//   3. tao_mx_dyn_linear_bf16 (one token): 1 and 2 in one launch. Every workgroup issues its first
//      weight slice, quantises the token into LDS (codes and scale bytes, the arithmetic of 1: a
//      block's scale depends on that block alone, so there is no row-wide reduction and no barrier
//      before the codes are written), then runs the GEMV on the codes. Bit-identical to 1 -> 2.
//
// mx_gemv_kernel: the byte-weight decomposition, tail, epilogue and launch shape of tao_gemv.h, as
// fp8dyn_gemv_kernel (fp8_dyn.hip): both code streams decoded in hardware
// (v_cvt_scalef32_pk_bf16_fp8 with scale 1.0, exact), one v_dot2c_f32_bf16 per code pair. A lane's
// 16-B chunk is half a block; its fp32 partial sum is scaled by the block's 2^(xs + ws - 254)
// with one v_ldexp_f32 (exact short of fp32 overflow / underflow, so scaling the two halves of a
// block apart equals scaling their sum), then accumulated in fp32.
#include "fp8_dyn_host.h"
#include "fp8_quant_row.h"
#include "mx_block.h"
#include "tao_gemm.h"
#include "tao_gemv.h"

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
struct MxGemvArgs {
  const void* x;         // e4m3fn codes [M][K] (FQ: the bf16 token [K])
  const uint8_t* xs;     // [M][K/32] E8M0 bytes (unused with FQ)
  const uint4* w;        // [N][K/16] e4m3fn codes
  const uint8_t* ws;     // [N][K/32] E8M0 bytes
  const uint16_t* bias;  // [N] bf16 or null
  uint16_t* y;           // [M][N]
  int M, N, K, Wk, G, S;
};

// codes (2 sel, 2 sel + 1) of a dword -> bf16 pair, exact
template <bool HI>
__device__ __forceinline__ uint32_t mx_pair_bf16(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
}
// the 16 codes of a 16-B chunk -> 8 bf16 pairs (k, k + 1) in k order
__device__ __forceinline__ void mx_chunk_bf16(const uint4 v, uint32_t (&p)[8]) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[2 * j] = mx_pair_bf16<false>(d[j]);
    p[2 * j + 1] = mx_pair_bf16<true>(d[j]);
  }
}

// NPT > 0 (FQ, M == 1): x is the bf16 token, NPT 16-B pieces of it per thread (K <= 8 NPT T).
template <int MT, int RPW, int NPT>
__global__ __launch_bounds__(512) void mx_gemv_kernel(MxGemvArgs a) {
  constexpr bool FQ = NPT > 0;
  static_assert(!FQ || MT == 1, "the fused quantisation is one token");
  constexpr int V = RPW * MT;
  // [G][Wk][V] fp32 partials | (FQ) the token's codes [K] | (FQ) its scale bytes [K/32]
  extern __shared__ float lds_f[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % a.Wk;
  const int rg = wave / a.Wk;
  const int row0 = (blockIdx.x * a.G + rg) * RPW;
  const int K = a.K, N = a.N, S = a.S, Wk = a.Wk;
  const int nchunk = K >> 4;  // 16-B (16-k) chunks per row; chunk c lies in block c >> 1
  const int nblk = K >> 5;
  const int nw = a.G * a.Wk;
  uint4* xl = reinterpret_cast<uint4*>(lds_f + ((nw * V + 8 + 3) & ~3));
  uint8_t* xsl = reinterpret_cast<uint8_t*>(xl) + K;

  float acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

  // a slice's codes and the scale byte of the lane's block; rows and chunks clamped in bounds
  uint4 wv[RPW];
  uint32_t wsb[RPW];
  auto load_w = [&](int s) __attribute__((always_inline)) {
    const int c = s * 64 + lane;
    const int cc = c < nchunk ? c : nchunk - 1;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const size_t nn = (size_t)(n < N ? n : N - 1);
      wv[r] = ld_nt_u4(a.w + nn * nchunk + cc);
      wsb[r] = a.ws[nn * nblk + (cc >> 1)];
    }
  };

  if constexpr (FQ) {
    // The token's pieces are loaded BEFORE the first slice's weights: vector loads retire in
    // issue order, so the wait for x does not wait for the weights, and the quantisation into LDS
    // runs under the weight loads' latency. Four consecutive threads hold one block (K / 8 is a
    // multiple of 4, so a group of four is whole or clamped as a whole).
    const uint4* xr = reinterpret_cast<const uint4*>(a.x);
    const int nvec = K >> 3;
    uint4 xv[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      xv[u] = xr[i < nvec ? i : nvec - 1];
    }
    load_w(wk);  // Wk <= S: every wave owns a slice
    uint2* xq = reinterpret_cast<uint2*>(xl);
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      uint32_t m = mx_amax8(xv[u], 0u);
      uint32_t o = (uint32_t)__shfl_xor((int)m, 1);
      m = m > o ? m : o;
      o = (uint32_t)__shfl_xor((int)m, 2);
      m = m > o ? m : o;
      const uint32_t byte = mx_scale_byte(m);
      if (i < nvec) {
        xq[i] = fp8_quant8(xv[u], mx_divisor(byte));
        if ((i & 3) == 0) xsl[i >> 2] = (uint8_t)byte;
      }
    }
    __syncthreads();
  } else {
    load_w(wk);
  }

  for (int s = wk; s < S; s += Wk) {
    if (s != wk) load_w(s);
    const int c = s * 64 + lane;
    const bool cval = c < nchunk;
    const int cc = cval ? c : nchunk - 1;
    if (cval) {  // a lane past the row's last chunk skips the math
      uint32_t wp[RPW][8];
#pragma unroll
      for (int r = 0; r < RPW; ++r) mx_chunk_bf16(wv[r], wp[r]);
      // x is streamed one row of M at a time
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        uint4 xc;
        uint32_t xb;
        if constexpr (FQ) {
          xc = xl[cc];
          xb = xsl[cc >> 1];
        } else {
          const size_t mm = (size_t)(m < a.M ? m : a.M - 1);
          xc = reinterpret_cast<const uint4*>(a.x)[mm * nchunk + cc];
          xb = a.xs[mm * nblk + (cc >> 1)];
        }
        uint32_t xp[8];
        mx_chunk_bf16(xc, xp);
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          float d = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) d = dot2_bf16(xp[i], wp[r][i], d);
          acc[r][m] += mx_scaled(d, xb, wsb[r]);
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

  const WgTotal<float> t = wg_combine<V>(v[0], lds_f, lane, wk, rg, Wk);
  if (t.writer) {
    const int r = t.widx / MT, m = t.widx % MT;
    const int n = row0 + r;
    if (n < N && m < a.M) {
      float o = t.total;
      if (a.bias != nullptr) o = o + bf16_to_f32(a.bias[n]);
      a.y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

template <int MT, int RPW, int NPT>
int launch_gemv_npt(MxGemvArgs a, int grid, int threads, size_t lds, hipStream_t stream) {
  launch((mx_gemv_kernel<MT, RPW, NPT>), dim3(grid), dim3(threads), lds, stream, a);
  return check_launch("mx_gemv_kernel");
}

// fp8dyn_gemv_kernel's launch shape (fp8_dyn_host.h); the fused launch keeps the token's K / 32
// scale bytes behind its codes.
template <int MT, int RPW, bool FQ>
int launch_gemv(MxGemvArgs a, int wk, int g, hipStream_t stream) {
  const Fp8DynLaunch L = fp8dyn_launch_shape(a.N, a.K, RPW, MT, wk, g, FQ);
  a.S = L.S;
  a.Wk = L.Wk;
  a.G = L.G;
  if constexpr (!FQ) {
    return launch_gemv_npt<MT, RPW, 0>(a, L.grid, L.threads, L.lds, stream);
  } else {
    const size_t lds = L.lds + (size_t)((a.K / 32 + 15) & ~15);
    if (L.per <= 1) return launch_gemv_npt<MT, RPW, 1>(a, L.grid, L.threads, lds, stream);
    if (L.per <= 2) return launch_gemv_npt<MT, RPW, 2>(a, L.grid, L.threads, lds, stream);
    if (L.per <= 4) return launch_gemv_npt<MT, RPW, 4>(a, L.grid, L.threads, lds, stream);
    if (L.per <= 8) return launch_gemv_npt<MT, RPW, 8>(a, L.grid, L.threads, lds, stream);
    if (L.per <= 16) return launch_gemv_npt<MT, RPW, 16>(a, L.grid, L.threads, lds, stream);
    TAO_CHECK_ARG(false, "mx dyn linear: K (%d) too long for the token prologue", a.K);
  }
  return TAO_OK;
}

// The shapes of the float8 dynamic GEMV (fp8_dyn.hip gemv_m1, fp8dyn_gemv): M == 1 on ready-made
// codes 4 rows per wave, Wk = min(S, 8), one row group; the fused launch 8 rows per wave, 4 waves
// along K, 2 row groups; M > 1 keeps V = RPW * MT = 8 partials per lane, 8 waves per workgroup.
int mx_gemv(MxGemvArgs a, hipStream_t stream) {
  if (a.M <= 1) return launch_gemv<1, 4, false>(a, 8, 1, stream);
  if (a.M <= 2) return launch_gemv<2, 4, false>(a, 8, 8, stream);
  if (a.M <= 4) return launch_gemv<4, 2, false>(a, 8, 8, stream);
  return launch_gemv<8, 1, false>(a, 8, 8, stream);
}

int check_mx_sizes(const char* what, int64_t M, int64_t N, int64_t K) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "%s: negative size", what);
  TAO_CHECK_ARG(K % 32 == 0, "%s: K (%lld) must be a multiple of 32 (the MX block size)", what,
                (long long)K);
  return TAO_OK;
}

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
    MxGemvArgs a{xq, xs, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                 (int)M, (int)N, (int)K, 0, 0, 0};
    return mx_gemv(a, as_stream(stream));
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
  MxGemvArgs a{x, nullptr, reinterpret_cast<const uint4*>(wq), ws, bias, y,
               1, (int)N, (int)K, 0, 0, 0};
  return launch_gemv<1, 8, true>(a, 4, 2, as_stream(stream));
}

}  // extern "C"
