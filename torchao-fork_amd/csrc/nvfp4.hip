// NVFP4 inference linear (NVFP4InferenceConfig, torchao/prototype/mx_formats/nvfp4_tensor.py):
// e2m1 codes, two per byte, one e4m3fn scale byte per 16 codes of a row, and an optional fp32
// per-tensor scale on top. Row quantizer, activation snap, dequantizer and the decode GEMV behind
// tao_nvfp4_quantize_rows_bf16, tao_nvfp4_act_qdq_bf16, tao_nvfp4_dequant_bf16 and
// tao_nvfp4_linear_bf16. The layouts, the served shapes and the route's default boundary are in
// nvfp4_host.h; the rule, the GEMV's tile, launch and tail are the weight-only front end's
// (wo_host.h, tao_gemv.h).
//
// Storage is the reference's: element 2 j of a row in the HIGH nibble of byte j (pack_uint4), the
// scales row-major [rows][K / 16] or in the swizzled 128 x 4 layout (nvfp4_scale_offset). The
// per-tensor scales are read from device memory inside the kernels: no host synchronisation.
//
//   quantize, per block of 16, fp32 (nvfp4_quantize of the reference, on the CPU):
//       b    = amax|x| / 6                   (/ per_tensor_scale as well, where there is one)
//       s    = e4m3fn_rne(clamp(b, 2^-6, 448))
//       code = e2m1_rne_sat(clamp(x / (s  or  per_tensor_scale * s), -6, 6))
//     every division is the IEEE fp32 quotient.
//   snap (DYNAMIC mode's activation): the same arithmetic, output bf16(value(code) * s). The
//     product has at most 2 + 4 significant bits and lies between 2^-10 and 2^11, so it is a bf16
//     number: the snap rounds nothing.
//   dequantize: bf16(value(code) * float(t)), t = s, or bf16(bf16(per_tensor_scale) * s) where
//     there is a per-tensor scale: the bits of the reference's to_dtype(bf16) with a 0-dim scale.
//   linear, both modes:
//       y[m][n] = bf16(alpha * sum_b s[n][b] * (sum_{k in b} xq[m][k] * value(code[n][k])) + bias[n])
//     fp32 sums, one rounding; alpha = the weight's per-tensor scale (1 if absent) times the
//     activation's (DYNAMIC); xq = x, or x snapped (DYNAMIC).
//
// The hardware converter v_cvt_scalef32_pk_bf16_fp4 takes only the exponent of its fp32 scale
// operand (measured on gfx950: a scale of 1.75 * 2^-3 scales by 2^-3), so it cannot apply an e4m3
// scale. The GEMV therefore decodes with scale 1.0 (exact: every e2m1 value is a bf16 number),
// sums a block's 16 exact products x * value(code) with 8 v_dot2_f32_bf16, and applies the block's
// scale to that partial sum with one v_fma_f32: one more VALU per 16 weights.
//
// GEMV: the decomposition of tao_gemv.h with a lane chunk of 32 k: 16 B of codes (one non-temporal
// load) and the chunk's 2 scale bytes (one 2-B load, adjacent in either layout), decoded to fp32 by
// the hardware e4m3 converter. DYN (one token): the workgroup snaps the token into LDS first, with
// the snap kernel's arithmetic, so DYNAMIC decode is one launch, bit-identical to the snap kernel
// followed by the plain GEMV.
//
// MFMA route (M above the GEMV's boundary): the Nvfp4WO policy of gemm_mfma_kernel
// (gemm_mfma_policy.h) on the same bytes, with the same epilogue, reached through
// tao_tune_nvfp4_mfma until the route rule names it.
#include "fp8_convert.h"
#include "mx_block.h"
#include "nvfp4_host.h"
#include "tao_gemm.h"
#include "tao_gemv.h"

namespace tao {

namespace {

typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// ---- block arithmetic ---------------------------------------------------------------------------
__device__ __forceinline__ float e4m3_to_f32(uint32_t byte) {
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(byte, 1.0f, false)[0];
}
// both scale bytes of a lane chunk (a 2-B load) as fp32
__device__ __forceinline__ f32x2_t e4m3x2_to_f32(uint32_t two) {
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(two, 1.0f, false);
}
// byte B of a code dword -> (low nibble, high nibble) = (w[2B+1], w[2B]) as fp32 / as a bf16 pair
template <int B>
__device__ __forceinline__ f32x2_t e2m1_pair_f32(uint32_t w) {
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, B);
}
template <int B>
__device__ __forceinline__ uint32_t e2m1_pair_bf16(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, B));
}
// the nibbles of every byte exchanged: the converters then give (w[2B], w[2B+1])
__device__ __forceinline__ uint32_t swap_nibbles(uint32_t v) {
  return ((v << 4) & 0xF0F0F0F0u) | ((v >> 4) & 0x0F0F0F0Fu);
}

// A block's scale from its amax (a bf16 magnitude pattern): the byte, its value and the divisor of
// the block's elements. pts: the per-tensor scale in device memory, or null.
struct Nvfp4Scale {
  uint32_t byte;
  float val, div;
};
__device__ __forceinline__ Nvfp4Scale nvfp4_block_scale(uint32_t amax15, const float* pts) {
  float b = bf16_to_f32(amax15) / 6.0f;
  float p = 1.0f;
  if (pts != nullptr) {
    p = *pts;
    b = b / p;
  }
  b = fminf(fmaxf(b, 0.015625f), 448.0f);
  Nvfp4Scale s;
  s.byte = f32_to_e4m3fn_rne(b);
  s.val = e4m3_to_f32(s.byte);
  s.div = pts != nullptr ? p * s.val : s.val;
  return s;
}
// the 8 bf16 of one 16-B piece -> 8 nibbles, element 2 j in the high nibble of byte j
__device__ __forceinline__ uint32_t nvfp4_quant8(const uint4 v, float div) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t o = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = (j & 1) ? bf16hi_to_f32(d[j >> 1]) : bf16lo_to_f32(d[j >> 1]);
    const float y = fminf(fmaxf(x / div, -6.0f), 6.0f);
    o |= mxfp4_code(y) << (8 * (j >> 1) + ((j & 1) ? 0 : 4));
  }
  return o;
}
// 8 codes (one dword) -> 8 bf16 of value(code) * t, in element order. Exact for t = an e4m3 value.
__device__ __forceinline__ uint4 nvfp4_decode8(uint32_t c, float t) {
  const f32x2_t p[4] = {e2m1_pair_f32<0>(c), e2m1_pair_f32<1>(c), e2m1_pair_f32<2>(c),
                        e2m1_pair_f32<3>(c)};
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = (uint32_t)f32_to_bf16(p[j][1] * t) | ((uint32_t)f32_to_bf16(p[j][0] * t) << 16);
  return make_uint4(o[0], o[1], o[2], o[3]);
}
// One block of 16 bf16 (a, b) snapped to its NVFP4 grid: quantize, then decode under the scale.
__device__ __forceinline__ void nvfp4_snap16(uint4& a, uint4& b, const float* pts) {
  const Nvfp4Scale s = nvfp4_block_scale(mx_amax8(b, mx_amax8(a, 0u)), pts);
  a = nvfp4_decode8(nvfp4_quant8(a, s.div), s.val);
  b = nvfp4_decode8(nvfp4_quant8(b, s.div), s.val);
}

// ---- quantizer ----------------------------------------------------------------------------------
// One thread per scale position of the (SWZ: padded) [prows][pcols] scale matrix: a position inside
// [rows][cols] quantizes its block (two 16-B loads, one 8-B store, one scale byte), a padding
// position of the swizzled layout stores a zero byte, as to_blocked leaves it.
template <bool SWZ>
__global__ __launch_bounds__(256) void nvfp4_quantize_rows_kernel(
    const uint4* __restrict__ x, uint2* __restrict__ q, uint8_t* __restrict__ scale,
    const float* __restrict__ pts, int rows, int cols, int pcols, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int64_t r = t / pcols;
  const int c = (int)(t - r * pcols);
  const int64_t so = SWZ ? nvfp4_scale_offset(r, c, pcols >> 2) : t;
  if (r < rows && c < cols) {
    const int64_t b = r * cols + c;
    const uint4 lo = x[2 * b], hi = x[2 * b + 1];
    const Nvfp4Scale s = nvfp4_block_scale(mx_amax8(hi, mx_amax8(lo, 0u)), pts);
    q[b] = make_uint2(nvfp4_quant8(lo, s.div), nvfp4_quant8(hi, s.div));
    scale[so] = (uint8_t)s.byte;
  } else {
    scale[so] = 0;
  }
}

// ---- activation snap ------------------------------------------------------------------------------
// One thread per block: two 16-B loads in, two 16-B stores out.
__global__ __launch_bounds__(256) void nvfp4_act_qdq_kernel(const uint4* __restrict__ x,
                                                            uint4* __restrict__ y,
                                                            const float* __restrict__ pts,
                                                            int64_t nblocks) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nblocks) return;
  uint4 lo = x[2 * b], hi = x[2 * b + 1];
  nvfp4_snap16(lo, hi, pts);
  y[2 * b] = lo;
  y[2 * b + 1] = hi;
}

// ---- dequantizer --------------------------------------------------------------------------------
// Streaming: one thread per block (8 B of codes and the scale byte in, two 16-B stores out).
template <bool SWZ>
__global__ __launch_bounds__(256) void nvfp4_dequant_kernel(const u32x2_t* __restrict__ q,
                                                            const uint8_t* __restrict__ scale,
                                                            const float* __restrict__ pts,
                                                            uint4* __restrict__ w, int cols,
                                                            int64_t nblocks) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nblocks) return;
  const int64_t r = b / cols;
  const int64_t so = SWZ ? nvfp4_scale_offset(r, b - r * cols, nvfp4_col_tiles(cols)) : b;
  float t = e4m3_to_f32(scale[so]);
  if (pts != nullptr) t = round_bf16(round_bf16(*pts) * t);
  const u32x2_t c = __builtin_nontemporal_load(q + b);
  st_nt_u4(w + 2 * b, nvfp4_decode8(c[0], t));
  st_nt_u4(w + 2 * b + 1, nvfp4_decode8(c[1], t));
}

// ---- decode GEMV ----------------------------------------------------------------------------------
// K % 64 == 0: a row is nchunk = K / 32 whole lane chunks, its scales K / 16 bytes (row-major) or
// the c % 4 groups of its swizzled tile row; chunk c's two bytes start at scale column 2 c.
template <int MT, int RPW, bool SWZ, bool DYN>
__global__ __launch_bounds__(512) void nvfp4_gemv_kernel(
    const uint16_t* __restrict__ x, const uint4* __restrict__ w, const uint8_t* __restrict__ ws,
    const float* __restrict__ w_pts, const float* __restrict__ a_pts,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int M, int N, int K, int Wk, int G,
    int S) {
  static_assert(!DYN || MT == 1, "the fused snap is one token");
  constexpr int V = RPW * MT;
  constexpr bool SWAPW = MT >= 4;  // exchange the weight's nibbles (else rotate x's pairs)
  // [G][Wk][V] partials | (DYN) the snapped token, [K / 8] uint4
  extern __shared__ __attribute__((aligned(16))) float red[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % Wk;
  const int rg = wave / Wk;
  const int row0 = (blockIdx.x * G + rg) * RPW;
  const int nchunk = K / kNvfp4ChunkK;
  const int scols = K / kNvfp4Block;
  uint4* xs = reinterpret_cast<uint4*>(red + ((G * Wk * V + 3) & ~3));

  if constexpr (DYN) {
    const uint4* xr = reinterpret_cast<const uint4*>(x);
    for (int b = threadIdx.x; b < scols; b += (int)blockDim.x) {
      uint4 lo = xr[2 * b], hi = xr[2 * b + 1];
      nvfp4_snap16(lo, hi, a_pts);
      xs[2 * b] = lo;
      xs[2 * b + 1] = hi;
    }
    __syncthreads();
  }

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
    uint32_t sv[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const int nn = n < N ? n : N - 1;
      wv[r] = ld_nt_u4(w + (size_t)nn * nchunk + cc);
      const size_t so = SWZ ? (size_t)nvfp4_scale_offset(nn, 2 * cc, scols >> 2)
                            : (size_t)nn * scols + 2 * cc;
      sv[r] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(ws + so));
    }
    // A lane past the row's last chunk loaded clamped (valid) addresses and adds nothing.
    if (cval) {
      uint32_t wp[RPW][16];  // bf16 pairs of value(code), in the order of xd below
      f32x2_t sc[RPW];
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const uint32_t d[4] = {wv[r].x, wv[r].y, wv[r].z, wv[r].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t v = SWAPW ? swap_nibbles(d[j]) : d[j];
          wp[r][4 * j + 0] = e2m1_pair_bf16<0>(v);
          wp[r][4 * j + 1] = e2m1_pair_bf16<1>(v);
          wp[r][4 * j + 2] = e2m1_pair_bf16<2>(v);
          wp[r][4 * j + 3] = e2m1_pair_bf16<3>(v);
        }
        sc[r] = e4m3x2_to_f32(sv[r]);
      }
      // x is streamed one row of M at a time: 16 live dwords whatever M is.
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int mm = m < M ? m : M - 1;
        const uint4* xp = DYN ? xs + 4 * (size_t)cc
                              : reinterpret_cast<const uint4*>(x + (size_t)mm * K +
                                                               (size_t)cc * kNvfp4ChunkK);
        uint32_t xd[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint4 a = xp[q];
          xd[4 * q] = a.x, xd[4 * q + 1] = a.y, xd[4 * q + 2] = a.z, xd[4 * q + 3] = a.w;
        }
        if constexpr (!SWAPW) {  // (x[2i], x[2i+1]) -> (x[2i+1], x[2i]): the converter's order
#pragma unroll
          for (int i = 0; i < 16; ++i) xd[i] = __builtin_amdgcn_alignbit(xd[i], xd[i], 16);
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          float d0 = 0.f, d1 = 0.f;  // the chunk's two blocks
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            d0 = dot2_bf16(xd[i], wp[r][i], d0);
            d1 = dot2_bf16(xd[8 + i], wp[r][8 + i], d1);
          }
          acc[r][m] = fmaf(d1, sc[r][1], fmaf(d0, sc[r][0], acc[r][m]));
        }
      }
    }
  }

  // the tail, written out in each GEMV kernel (tao_gemv.h, "the plain weight-only GEMVs' tail")
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
      // the per-tensor scales and the bias meet the fp32 total; one rounding
      float alpha = w_pts != nullptr ? *w_pts : 1.0f;
      if (a_pts != nullptr) alpha *= *a_pts;
      float o = t.total * alpha;
      if (bias != nullptr) o += bf16_to_f32(bias[n]);
      y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

struct Nvfp4Args {
  const uint16_t* x;
  const uint4* w;
  const uint8_t* ws;
  const float *w_pts, *a_pts;
  const uint16_t* bias;
  uint16_t* y;
  int N, K;
};

// wk, g: tao_tune_nvfp4's, 0 = the default shape (tao_gemv.h wo_gemv_launch)
template <int MT, int RPW, bool SWZ, bool DYN>
int nvfp4_gemv_launch(const Nvfp4Args& a, const uint16_t* x, uint16_t* y, int M,
                      hipStream_t stream, int wk, int g) {
  const WoGemvLaunch L = wo_gemv_launch(a.K / kNvfp4ChunkK, a.N, MT, RPW, wk, g);
  const size_t lds = DYN ? ((L.lds + 15) & ~(size_t)15) + (size_t)a.K * 2 : L.lds;
  launch(nvfp4_gemv_kernel<MT, RPW, SWZ, DYN>, dim3(L.grid), dim3(L.threads), lds, stream, x, a.w,
         a.ws, a.w_pts, a.a_pts, a.bias, y, M, a.N, a.K, L.Wk, L.G, L.S);
  return check_launch("nvfp4_gemv_kernel");
}

template <bool SWZ, bool DYN>
int nvfp4_gemv(const Nvfp4Args& a, const uint16_t* x, uint16_t* y, int m, hipStream_t st,
               const WoTune& tu) {
  return dispatch_gemv_tile(m, tu.rpw, [&](auto mt, auto rpw) {
    constexpr int MT = decltype(mt)::value;
    return nvfp4_gemv_launch<MT, decltype(rpw)::value, SWZ, DYN && MT == 1>(a, x, y, m, st, tu.wk,
                                                                           tu.g);
  });
}

// the longest token the fused snap stages: 2 K bytes of LDS beside the reduction's
constexpr int64_t kNvfp4DynMaxK = 16384;

int check_nvfp4_quant(const char* what, int64_t rows, int64_t K, const void* x, const void* out) {
  TAO_CHECK_ARG(rows >= 0 && K >= 0 && rows < (1LL << 31) && K < (1LL << 31),
                "%s: rows and K must be in [0, 2^31)", what);
  TAO_CHECK_ARG(K % kNvfp4Block == 0, "%s: K (%lld) must be a multiple of 16", what, (long long)K);
  if (rows == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(out, 16, what);
  return TAO_OK;
}

}  // namespace

}  // namespace tao

extern "C" int tao_nvfp4_quantize_rows_bf16(const uint16_t* x, uint8_t* qdata, uint8_t* scales,
                                            const float* per_tensor_scale, int64_t rows, int64_t K,
                                            int swizzled, void* stream) {
  using namespace tao;
  if (int rc = check_nvfp4_quant("nvfp4 quantize", rows, K, x, qdata)) return rc;
  TAO_CHECK_ARG(swizzled == 0 || swizzled == 1, "nvfp4 quantize: swizzled must be 0 or 1");
  if (rows == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(per_tensor_scale, 4, "per_tensor_scale");
  const int cols = (int)(K / kNvfp4Block);
  const int pcols = swizzled ? (int)nvfp4_col_tiles(cols) * 4 : cols;
  const int64_t total = swizzled ? nvfp4_scale_bytes(rows, K, true) : rows * cols;
  const dim3 grid((unsigned)((total + 255) / 256));
  const uint4* x4 = reinterpret_cast<const uint4*>(x);
  uint2* q2 = reinterpret_cast<uint2*>(qdata);
  if (swizzled)
    launch(nvfp4_quantize_rows_kernel<true>, grid, dim3(256), 0, as_stream(stream), x4, q2, scales,
           per_tensor_scale, (int)rows, cols, pcols, total);
  else
    launch(nvfp4_quantize_rows_kernel<false>, grid, dim3(256), 0, as_stream(stream), x4, q2,
           scales, per_tensor_scale, (int)rows, cols, pcols, total);
  return check_launch("nvfp4_quantize_rows_kernel");
}

extern "C" int tao_nvfp4_act_qdq_bf16(const uint16_t* x, uint16_t* y,
                                      const float* per_tensor_scale, int64_t rows, int64_t K,
                                      void* stream) {
  using namespace tao;
  if (int rc = check_nvfp4_quant("nvfp4 act qdq", rows, K, x, y)) return rc;
  if (rows == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(per_tensor_scale, 4, "per_tensor_scale");
  const int64_t nblocks = rows * (K / kNvfp4Block);
  launch(nvfp4_act_qdq_kernel, dim3((unsigned)((nblocks + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint4*>(x), reinterpret_cast<uint4*>(y),
         per_tensor_scale, nblocks);
  return check_launch("nvfp4_act_qdq_kernel");
}

extern "C" int tao_nvfp4_dequant_bf16(const uint8_t* qdata, const uint8_t* scales,
                                      const float* per_tensor_scale, uint16_t* w, int64_t N,
                                      int64_t K, int swizzled, void* stream) {
  using namespace tao;
  if (int rc = check_nvfp4_quant("nvfp4 dequant", N, K, w, qdata)) return rc;
  TAO_CHECK_ARG(swizzled == 0 || swizzled == 1, "nvfp4 dequant: swizzled must be 0 or 1");
  if (N == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(per_tensor_scale, 4, "per_tensor_scale");
  const int64_t nblocks = N * (K / kNvfp4Block);
  const dim3 grid((unsigned)((nblocks + 255) / 256));
  const u32x2_t* q2 = reinterpret_cast<const u32x2_t*>(qdata);
  uint4* w4 = reinterpret_cast<uint4*>(w);
  if (swizzled)
    launch(nvfp4_dequant_kernel<true>, grid, dim3(256), 0, as_stream(stream), q2, scales,
           per_tensor_scale, w4, (int)(K / kNvfp4Block), nblocks);
  else
    launch(nvfp4_dequant_kernel<false>, grid, dim3(256), 0, as_stream(stream), q2, scales,
           per_tensor_scale, w4, (int)(K / kNvfp4Block), nblocks);
  return check_launch("nvfp4_dequant_kernel");
}

extern "C" int tao_nvfp4_linear_route(int64_t M, int64_t N, int64_t K) {
  return tao::nvfp4_route(M, N, K, tao::tuning().nvfp4.route, tao::tuning().nvfp4.max_m,
                          tao::tuning().nvfp4_mfma);
}

extern "C" int tao_nvfp4_linear_fused_snap(int64_t M, int64_t K) {
  return M == 1 && K <= tao::kNvfp4DynMaxK;
}

extern "C" int tao_nvfp4_linear_bf16(const uint16_t* x, const uint8_t* qdata,
                                     const uint8_t* scales, const float* per_tensor_scale,
                                     const float* act_per_tensor_scale, const uint16_t* bias,
                                     uint16_t* y, int64_t M, int64_t N, int64_t K, int swizzled,
                                     int dynamic, void* stream) {
  using namespace tao;
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && M < (1LL << 31) && N < (1LL << 31) &&
                    K < (1LL << 31),
                "nvfp4 linear: K (%lld) must be positive and M, N, K below 2^31", (long long)K);
  TAO_CHECK_ARG(K % 64 == 0, "nvfp4 linear: K (%lld) must be a multiple of 64", (long long)K);
  TAO_CHECK_ARG(N % 16 == 0, "nvfp4 linear: N (%lld) must be a multiple of 16", (long long)N);
  TAO_CHECK_ARG((swizzled == 0 || swizzled == 1) && (dynamic == 0 || dynamic == 1),
                "nvfp4 linear: swizzled and dynamic must be 0 or 1");
  TAO_CHECK_ARG(!dynamic || tao_nvfp4_linear_fused_snap(M, K) || M == 0,
                "nvfp4 linear: the fused snap is one token of K <= %lld (got M = %lld, K = %lld); "
                "snap with tao_nvfp4_act_qdq_bf16 first",
                (long long)kNvfp4DynMaxK, (long long)M, (long long)K);
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(qdata, 16, "qdata");
  TAO_CHECK_ALIGN(scales, 2, "scales");
  TAO_CHECK_ALIGN(per_tensor_scale, 4, "per_tensor_scale");
  TAO_CHECK_ALIGN(act_per_tensor_scale, 4, "act_per_tensor_scale");
  TAO_CHECK_ALIGN(y, 2, "y");
  if (bias != nullptr) TAO_CHECK_ALIGN(bias, 2, "bias");
  const hipStream_t st = as_stream(stream);
  const WoTune& tu = tuning().nvfp4;
  const Nvfp4Args a{x, reinterpret_cast<const uint4*>(qdata), scales, per_tensor_scale,
                    act_per_tensor_scale, bias, y, (int)N, (int)K};
  // the Nvfp4WO policy of gemm_mfma_kernel where the rule names it (tao_tune_nvfp4_mfma); x is
  // already snapped in DYNAMIC mode (the rule keeps one token, the fused snap's, on the GEMV)
  if (nvfp4_route(M, N, K, tu.route, tu.max_m, tuning().nvfp4_mfma) == kWoRouteMfma)
    return nvfp4_mm_launch(x, qdata, scales, per_tensor_scale, act_per_tensor_scale, bias, y,
                           (int)M, (int)N, (int)K, swizzled, st);
  if (dynamic)
    return swizzled ? nvfp4_gemv<true, true>(a, x, y, 1, st, tu)
                    : nvfp4_gemv<false, true>(a, x, y, 1, st, tu);
  return for_gemv_pieces(x, y, M, N, K, [&](const uint16_t* xm, uint16_t* ym, int m) {
    return swizzled ? nvfp4_gemv<true, false>(a, xm, ym, m, st, tu)
                    : nvfp4_gemv<false, false>(a, xm, ym, m, st, tu);
  });
}

extern "C" int tao_tune_nvfp4(int route, int max_gemv_m, int rows_per_wave, int waves_k,
                              int row_groups) {
  using namespace tao;
  if (int rc = check_wo_tune("nvfp4", route, max_gemv_m, rows_per_wave, waves_k, row_groups))
    return rc;
  tuning().nvfp4 = {route, max_gemv_m, rows_per_wave, waves_k, row_groups};
  return TAO_OK;
}

extern "C" int tao_tune_nvfp4_mfma(int on) {
  TAO_CHECK_ARG(on == 0 || on == 1, "tune: nvfp4 mfma must be 0 (built-in route) or 1");
  tao::tuning().nvfp4_mfma = on;
  return TAO_OK;
}
