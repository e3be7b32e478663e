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
//      inside v_mfma_scale_f32_16x16x128_f8f6f4; M at or below it: mxw4_gemv_kernel below.
//   3. tao_mxfp4w_dyn_linear_bf16 (one token): the e4m3fn block quantizer of mx_fp8.hip into LDS,
//      then the same GEMV, in one launch. Bit-identical to tao_mx_quantize_rows_bf16 -> 2.
//
// mxw4_gemv_kernel: the decomposition, tail, epilogue and launch shape of tao_gemv.h, as
// mx_gemv_kernel. A lane's 16-B weight chunk is one whole 32-k block (its x is 32 B of e4m3fn).
// Both code streams are decoded in hardware with scale 1.0 (exact): v_cvt_scalef32_pk_bf16_fp4
// turns byte j of a weight dword into the bf16 pair (low nibble, high nibble) = (w[2j+1], w[2j]);
// the x dword has its byte pairs swapped by one v_perm_b32 before v_cvt_scalef32_pk_bf16_fp8, so
// its pairs come out as (x[2j+1], x[2j]) too, and one v_dot2c_f32_bf16 takes each pair. (Where a
// lane holds more tokens than rows, MT = 4 and 8, the weight dwords have their nibbles exchanged
// instead, 3 instructions per dword, and x stays in k order.) The x pairs are converted once per
// token and reused by the wave's RPW rows. The block's fp32 partial
// sum is scaled by 2^(xs + ws - 254) with one v_ldexp_f32 and accumulated in fp32.
#include "fp8_dyn_host.h"
#include "fp8_quant_row.h"
#include "mx_block.h"
#include "tao_gemm.h"
#include "tao_gemv.h"

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
struct Mx4GemvArgs {
  const void* x;         // e4m3fn codes [M][K] (FQ: the bf16 token [K])
  const uint8_t* xs;     // [M][K/32] E8M0 bytes (unused with FQ)
  const uint4* w;        // [N][K/32] 16-B chunks of e2m1 codes (one block each)
  const uint8_t* ws;     // [N][K/32] E8M0 bytes
  const uint16_t* bias;  // [N] bf16 or null
  uint16_t* y;           // [M][N]
  int M, N, K, Wk, G, S;
};

// the 16 e4m3fn codes of a 16-B piece -> 8 bf16 pairs in k order; SWAP: pair 2 j + h =
// (x[4j+2h+1], x[4j+2h]), swapped within the pair, the order the e2m1 converter gives the
// weight's stored bytes
template <bool SWAP>
__device__ __forceinline__ void mx4_x16_bf16(const uint4 v, uint32_t* p) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t s = SWAP ? __builtin_amdgcn_perm(d[j], d[j], 0x02030001u) : d[j];  // 1 0 3 2
    p[2 * j] = __builtin_bit_cast(uint32_t,
                                  __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(s, 1.0f, false));
    p[2 * j + 1] = __builtin_bit_cast(uint32_t,
                                      __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(s, 1.0f, true));
  }
}
// byte B of a weight dword -> the bf16 pair (low nibble, high nibble) = (w[2B+1], w[2B]) of the
// stored bytes
template <int B>
__device__ __forceinline__ uint32_t mx4_w_pair(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, B));
}
// the nibbles of every byte exchanged: the converter then gives (w[2B], w[2B+1])
__device__ __forceinline__ uint32_t mx4_swap_nibbles(uint32_t v) {
  return ((v << 4) & 0xF0F0F0F0u) | ((v >> 4) & 0x0F0F0F0Fu);
}
__device__ __forceinline__ uint4 mx4_swap_nibbles(const uint4 v) {
  return make_uint4(mx4_swap_nibbles(v.x), mx4_swap_nibbles(v.y), mx4_swap_nibbles(v.z),
                    mx4_swap_nibbles(v.w));
}
// sum over the block's 32 k of x * w, from the 16 x pairs and the 16-B weight chunk (in the same
// order within the pairs)
__device__ __forceinline__ float mx4_block_dot(const uint32_t (&xp)[16], const uint4 wv) {
  const uint32_t d[4] = {wv.x, wv.y, wv.z, wv.w};
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s = dot2_bf16(xp[4 * j + 0], mx4_w_pair<0>(d[j]), s);
    s = dot2_bf16(xp[4 * j + 1], mx4_w_pair<1>(d[j]), s);
    s = dot2_bf16(xp[4 * j + 2], mx4_w_pair<2>(d[j]), s);
    s = dot2_bf16(xp[4 * j + 3], mx4_w_pair<3>(d[j]), s);
  }
  return s;
}

// NPT > 0 (FQ, M == 1): x is the bf16 token, NPT 16-B pieces of it per thread (K <= 8 NPT T).
template <int MT, int RPW, int NPT>
__global__ __launch_bounds__(512) void mxw4_gemv_kernel(Mx4GemvArgs a) {
  constexpr bool FQ = NPT > 0;
  static_assert(!FQ || MT == 1, "the fused quantisation is one token");
  constexpr int V = RPW * MT;
  // The pairs of one side are put in the other's order where that takes fewer instructions per
  // block: the x side (2 v_perm_b32 per 16-B piece and token) or the weight side (3 per dword and
  // row, before the conversion).
  constexpr bool SWAPW = 12 * RPW < 8 * MT;
  // [G][Wk][V] fp32 partials | (FQ) the token's codes [K] | (FQ) its scale bytes [K/32]
  extern __shared__ float lds_f[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % a.Wk;
  const int rg = wave / a.Wk;
  const int row0 = (blockIdx.x * a.G + rg) * RPW;
  const int K = a.K, N = a.N, S = a.S, Wk = a.Wk;
  const int nblk = K >> 5;  // 16-B weight chunks per row = blocks per row
  const int nw = a.G * a.Wk;
  uint4* xl = reinterpret_cast<uint4*>(lds_f + ((nw * V + 8 + 3) & ~3));
  uint8_t* xsl = reinterpret_cast<uint8_t*>(xl) + K;

  float acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

  // a slice's codes and the scale byte of the lane's block; rows and blocks clamped in bounds
  uint4 wv[RPW];
  uint32_t wsb[RPW];
  auto load_w = [&](int s) __attribute__((always_inline)) {
    const int c = s * 64 + lane;
    const int cc = c < nblk ? c : nblk - 1;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const size_t nn = (size_t)(n < N ? n : N - 1);
      wv[r] = ld_nt_u4(a.w + nn * nblk + cc);
      wsb[r] = a.ws[nn * nblk + cc];
    }
  };

  if constexpr (FQ) {
    // mx_gemv_kernel's prologue: the token's pieces are loaded before the first slice's weights,
    // quantised to e4m3fn blocks into LDS under the weight loads' latency. Four consecutive
    // threads hold one block.
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
    const bool cval = c < nblk;
    const int cc = cval ? c : nblk - 1;
    if (cval) {  // a lane past the row's last block skips the math
      if constexpr (SWAPW) {
#pragma unroll
        for (int r = 0; r < RPW; ++r) wv[r] = mx4_swap_nibbles(wv[r]);
      }
      // x is streamed one row of M at a time; its pairs serve the wave's RPW rows
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        uint4 x0, x1;
        uint32_t xb;
        if constexpr (FQ) {
          x0 = xl[2 * cc];
          x1 = xl[2 * cc + 1];
          xb = xsl[cc];
        } else {
          const size_t mm = (size_t)(m < a.M ? m : a.M - 1);
          const uint4* xr = reinterpret_cast<const uint4*>(a.x) + (mm * nblk + cc) * 2;
          x0 = xr[0];
          x1 = xr[1];
          xb = a.xs[mm * nblk + cc];
        }
        uint32_t xp[16];
        mx4_x16_bf16<!SWAPW>(x0, xp);
        mx4_x16_bf16<!SWAPW>(x1, xp + 8);
#pragma unroll
        for (int r = 0; r < RPW; ++r)
          acc[r][m] += mx_scaled(mx4_block_dot(xp, wv[r]), xb, wsb[r]);
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
int launch_gemv_npt(Mx4GemvArgs a, int grid, int threads, size_t lds, hipStream_t stream) {
  launch((mxw4_gemv_kernel<MT, RPW, NPT>), dim3(grid), dim3(threads), lds, stream, a);
  return check_launch("mxw4_gemv_kernel");
}

// fp8dyn_launch_shape (fp8_dyn_host.h) with 32-k chunks: S slices of 64 blocks, and for the fused
// launch the token's K code bytes and K / 32 scale bytes behind the partials, K / 8 token pieces
// over the workgroup's threads (row groups added while the token does not fit 16 pieces a thread).
template <int MT, int RPW, bool FQ>
int launch_gemv(Mx4GemvArgs a, int wk, int g, hipStream_t stream) {
  const GemvLaunchShape sh = gemv_launch_shape(a.K / 32, wk, g);
  a.S = sh.S;
  a.Wk = sh.Wk;
  a.G = sh.G;
  while (FQ && (int64_t)64 * a.Wk * a.G * 8 * 16 < a.K && a.Wk * a.G * 2 <= 8) a.G *= 2;
  const int rows_per_wg = a.G * RPW;
  const int grid = (int)(((int64_t)a.N + rows_per_wg - 1) / rows_per_wg);
  const int nw = a.G * a.Wk;
  const int threads = 64 * nw;
  if constexpr (!FQ) {
    return launch_gemv_npt<MT, RPW, 0>(a, grid, threads, (size_t)nw * RPW * MT * sizeof(float),
                                       stream);
  } else {
    const size_t lds = (((size_t)nw * RPW * MT + 8 + 3) & ~(size_t)3) * sizeof(float) +
                       (size_t)a.K + (size_t)((a.K / 32 + 15) & ~15);
    const int per = (a.K / 8 + threads - 1) / threads;
    if (per <= 1) return launch_gemv_npt<MT, RPW, 1>(a, grid, threads, lds, stream);
    if (per <= 2) return launch_gemv_npt<MT, RPW, 2>(a, grid, threads, lds, stream);
    if (per <= 4) return launch_gemv_npt<MT, RPW, 4>(a, grid, threads, lds, stream);
    if (per <= 8) return launch_gemv_npt<MT, RPW, 8>(a, grid, threads, lds, stream);
    if (per <= 16) return launch_gemv_npt<MT, RPW, 16>(a, grid, threads, lds, stream);
    TAO_CHECK_ARG(false, "mxfp4w dyn linear: K (%d) too long for the token prologue", a.K);
  }
  return TAO_OK;
}

// mx_gemv's shapes: M == 1 on ready-made codes 4 rows per wave, up to 8 waves along K, one row
// group; M > 1 keeps V = RPW * MT = 8 partials per lane, 8 waves per workgroup.
int mxw4_gemv(Mx4GemvArgs a, hipStream_t stream) {
  if (a.M <= 1) return launch_gemv<1, 4, false>(a, 8, 1, stream);
  if (a.M <= 2) return launch_gemv<2, 4, false>(a, 8, 8, stream);
  if (a.M <= 4) return launch_gemv<4, 2, false>(a, 8, 8, stream);
  return launch_gemv<8, 1, false>(a, 8, 8, stream);
}

int check_mx4_sizes(const char* what, int64_t M, int64_t N, int64_t K) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "%s: negative size", what);
  TAO_CHECK_ARG(K % 32 == 0, "%s: K (%lld) must be a multiple of 32 (the MX block size)", what,
                (long long)K);
  return TAO_OK;
}

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_mxfp4_quantize_rows_bf16(const uint16_t* x, uint8_t* q, uint8_t* scale, int64_t M,
                                 int64_t K, void* stream) {
  const int rc = check_mx4_sizes("mxfp4 quantize", M, 0, K);
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
  const int rc = check_mx4_sizes("mxfp4w scaled mm", M, N, K);
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
    Mx4GemvArgs a{xq, xs, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                  (int)M, (int)N, (int)K, 0, 0, 0};
    return mxw4_gemv(a, as_stream(stream));
  }
  return mxfp4w_scaled_mm_launch(xq, xs, wq, ws, bias, y, (int)M, (int)N, (int)K,
                                 as_stream(stream));
}

int tao_mxfp4w_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const uint8_t* ws,
                               const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                               void* stream) {
  const int rc = check_mx4_sizes("mxfp4w dyn linear", M, N, K);
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
  Mx4GemvArgs a{x, nullptr, reinterpret_cast<const uint4*>(wq), ws, bias, y,
                1, (int)N, (int)K, 0, 0, 0};
  return launch_gemv<1, 8, true>(a, 4, 2, as_stream(stream));
}

}  // extern "C"
