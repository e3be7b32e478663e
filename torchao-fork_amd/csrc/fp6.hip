// FP6 (e3m2 / e2m3) weight-only linear (FPXWeightOnlyConfig): row quantizer, dequantizer and the
// decode GEMV behind tao_fp6_quantize_rows_bf16, tao_fp6_dequant_bf16 and tao_fp6_linear_bf16
// (torchao/dtypes/floatx/floatx_tensor_core_layout.py). The formats' arithmetic and the storage
// are in fp6_codec.h; the route rule and the GEMV's tile choice are in fp6_host.h.
//
//   quantize, per row:   s = bf16(max(amax|w|, 1e-12) / max_normal)     the IEEE fp32 quotient
//                        code = fp6_rne_sat(float(w) / float(s))         again a true division
//   dequantize:          w^ = bf16(float(value(code)) * float(s))
//   linear:              y = bf16(float(sum_k x[k] value(code[n][k])) * float(s[n])) (+ bias -> bf16)
//
// Replaces the reference's quant_llm_linear (a CUDA kernel its ROCm build does not compile) and
// F.linear(x, weight.dequantize()).
//
// GEMV: the decomposition of tao_gemv.h with a lane chunk of GRP 32-code groups (24 B each; GRP = 1
// is the measured default, fp6_host.h): one
// v_cvt_scalef32_pk32_bf16_{bf6,fp6} per group with scale 1.0 (exact: every fp6 value is a bf16
// number), then 16 v_dot2_f32_bf16 against x as loaded; the row scale meets the fp32 total once.
#include "fp6_codec.h"
#include "fp6_host.h"
#include "tao_gemv.h"

namespace tao {

namespace {

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// ---- quantizer --------------------------------------------------------------------------------
// One workgroup per row; K % 32 == 0. Pass 1: amax over 16-B pieces; pass 2 (the row again, from
// L2): one thread per 32-code group, four 16-B loads in, three 8-B stores out.
// A NaN in the row does not reach amax (fmaxf drops it) and takes the masked code the normal branch
// of fp6_encode makes of it, inside its own field; an inf gives s = inf, every finite weight a
// signed zero code and the inf itself (inf / inf = NaN) such a NaN code. The reference writes s = inf / NaN and other arbitrary codes.
template <int FMT>
__global__ __launch_bounds__(256) void fp6_quantize_rows_kernel(const uint4* __restrict__ w,
                                                                uint32_t* __restrict__ codes,
                                                                uint16_t* __restrict__ scale,
                                                                int K) {
  __shared__ float red[4];
  const int K8 = K >> 3, ngroup = K >> 5;
  const uint4* row = w + (size_t)blockIdx.x * K8;
  float amax = 0.f;
  for (int i = threadIdx.x; i < K8; i += 256) {
    const uint4 v = row[i];
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      amax = fmaxf(amax, fmaxf(fabsf(bf16lo_to_f32(d[j])), fabsf(bf16hi_to_f32(d[j]))));
  }
  amax = wave_max(amax);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float s = fp6_row_scale<FMT>(amax);
  if (threadIdx.x == 0) scale[blockIdx.x] = f32_to_bf16(s);
  u32x2_t* out = reinterpret_cast<u32x2_t*>(codes + (size_t)blockIdx.x * ngroup * kFp6GroupDwords);
  for (int g = threadIdx.x; g < ngroup; g += 256) {
    uint32_t c[32];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 v = row[4 * g + q];
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[8 * q + 2 * j] = fp6_encode<FMT>(bf16lo_to_f32(d[j]) / s);
        c[8 * q + 2 * j + 1] = fp6_encode<FMT>(bf16hi_to_f32(d[j]) / s);
      }
    }
    uint32_t o[6];
    fp6_pack32(c, o);
#pragma unroll
    for (int q = 0; q < 3; ++q) out[3 * g + q] = u32x2_t{o[2 * q], o[2 * q + 1]};
  }
}

// ---- dequantizer ------------------------------------------------------------------------------
// Streaming: one thread per 32-code group (24 B in, three 8-B loads) and four 16-B stores (64 B out).
template <int FMT>
__global__ __launch_bounds__(256) void fp6_dequant_kernel(const u32x2_t* __restrict__ codes,
                                                          const uint16_t* __restrict__ scale,
                                                          uint4* __restrict__ w, int64_t ngroups,
                                                          int row_groups) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ngroups) return;
  const float s = bf16_to_f32(scale[i / row_groups]);
  uint32_t c[6];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const u32x2_t v = __builtin_nontemporal_load(codes + 3 * i + q);
    c[2 * q] = v[0];
    c[2 * q + 1] = v[1];
  }
  uint32_t p[16];
  fp6_decode32<FMT>(c, p);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t d = p[4 * q + j];
      o[j] = (uint32_t)f32_to_bf16(bf16lo_to_f32(d) * s) |
             ((uint32_t)f32_to_bf16(bf16hi_to_f32(d) * s) << 16);
    }
    st_nt_u4(w + 4 * i + q, make_uint4(o[0], o[1], o[2], o[3]));
  }
}

// ---- decode GEMV ------------------------------------------------------------------------------
// A lane's chunk: GRP groups = 6 GRP dwords at dword offset 6 GRP c of the row. GRP == 2: 48 B,
// 16-B aligned (a row is a multiple of 48 B), three 16-B loads; GRP == 1: 24 B, three 8-B loads.
template <int GRP>
__device__ __forceinline__ void fp6_load_chunk(const uint32_t* __restrict__ p,
                                               uint32_t (&c)[6 * GRP]) {
  if constexpr (GRP == 2) {
    const u32x4_t* q = reinterpret_cast<const u32x4_t*>(p);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const u32x4_t v = __builtin_nontemporal_load(q + i);
      c[4 * i] = v[0], c[4 * i + 1] = v[1], c[4 * i + 2] = v[2], c[4 * i + 3] = v[3];
    }
  } else {
    const u32x2_t* q = reinterpret_cast<const u32x2_t*>(p);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const u32x2_t v = __builtin_nontemporal_load(q + i);
      c[2 * i] = v[0], c[2 * i + 1] = v[1];
    }
  }
}

// y[m][n] = bf16(float(sum_k x[m][k] v[n][k]) * s[n]) (+ bias -> bf16), fp32 sums. K % 64 == 0, so
// a row is nchunk = K / (32 GRP) whole chunks for either GRP.
template <int FMT, int MT, int RPW, int GRP>
__global__ __launch_bounds__(512) void fp6wo_gemv_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ w,
    const uint16_t* __restrict__ scale, const uint16_t* __restrict__ bias,
    uint16_t* __restrict__ y, int M, int N, int K, int Wk, int G, int S) {
  constexpr int V = RPW * MT;
  constexpr int CD = kFp6GroupDwords * GRP;  // dwords per chunk
  extern __shared__ float red[];             // [G][Wk][V]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % Wk;
  const int rg = wave / Wk;
  const int row0 = (blockIdx.x * G + rg) * RPW;
  const int nchunk = K / (kFp6Group * GRP);
  const size_t row_dwords = (size_t)nchunk * CD;

  float acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

  for (int s = wk; s < S; s += Wk) {
    const int c = s * 64 + lane;
    const bool cval = c < nchunk;
    const int cc = cval ? c : nchunk - 1;

    uint32_t wv[RPW][CD];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const int nn = n < N ? n : N - 1;
      fp6_load_chunk<GRP>(w + (size_t)nn * row_dwords + (size_t)cc * CD, wv[r]);
    }
    // A lane past the row's last chunk loaded clamped (valid) addresses and adds nothing.
    if (cval) {
#pragma unroll
      for (int g = 0; g < GRP; ++g) {
        uint32_t wp[RPW][16];  // bf16 pairs (k, k + 1), in x's dword order
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          const uint32_t cg[6] = {wv[r][6 * g],     wv[r][6 * g + 1], wv[r][6 * g + 2],
                                  wv[r][6 * g + 3], wv[r][6 * g + 4], wv[r][6 * g + 5]};
          fp6_decode32<FMT>(cg, wp[r]);
        }
        // x is streamed one row of M at a time: 16 live dwords whatever M is.
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int mm = m < M ? m : M - 1;
          const uint4* xp = reinterpret_cast<const uint4*>(
              x + (size_t)mm * K + ((size_t)cc * GRP + g) * kFp6Group);
          uint32_t xd[16];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint4 a = xp[q];
            xd[4 * q] = a.x, xd[4 * q + 1] = a.y, xd[4 * q + 2] = a.z, xd[4 * q + 3] = a.w;
          }
#pragma unroll
          for (int r = 0; r < RPW; ++r) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) d = dot2_bf16(xd[i], wp[r][i], d);
            acc[r][m] += d;
          }
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
      // the row scale once per output, rounded; then + bias, rounded again (out + bias)
      float o = round_bf16(t.total * bf16_to_f32(scale[n]));
      if (bias != nullptr) o = round_bf16(o + bf16_to_f32(bias[n]));
      y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

// wk, g: 0 = the default shape, Wk = min(S, 8) waves along K and as many row groups as fit 8 waves
// (M > 1), one row group at M == 1: the byte-weight GEMVs' choice (tao_gemv.h wo8_gemv).
template <int FMT, int MT, int RPW, int GRP>
int fp6_gemv_launch(const uint16_t* x, const uint32_t* w, const uint16_t* scale,
                    const uint16_t* bias, uint16_t* y, int M, int N, int K, hipStream_t stream,
                    int wk, int g) {
  const GemvLaunchShape sh =
      gemv_launch_shape(K / (kFp6Group * GRP), wk > 0 ? wk : 8, g > 0 ? g : (MT == 1 ? 1 : 8));
  const int rows_per_wg = sh.G * RPW;
  const int grid = (N + rows_per_wg - 1) / rows_per_wg;
  const size_t lds = (size_t)sh.G * sh.Wk * RPW * MT * sizeof(float);
  launch(fp6wo_gemv_kernel<FMT, MT, RPW, GRP>, dim3(grid), dim3(64 * sh.Wk * sh.G), lds, stream, x,
         w, scale, bias, y, M, N, K, sh.Wk, sh.G, sh.S);
  return check_launch("fp6wo_gemv_kernel");
}

template <int FMT, int GRP>
int fp6_gemv(const uint16_t* x, const uint32_t* w, const uint16_t* scale, const uint16_t* bias,
             uint16_t* y, int m, int N, int K, hipStream_t st, const Tuning& tu) {
  const Fp6GemvTile tile = fp6_gemv_tile(m);
#define TAO_FP6(MT, RPW) \
  return fp6_gemv_launch<FMT, MT, RPW, GRP>(x, w, scale, bias, y, m, N, K, st, tu.fp6_wk, tu.fp6_g)
  if (tile.mt == 1) {
    if (tu.fp6_rpw == 2) TAO_FP6(1, 2);
    if (tu.fp6_rpw == 8) TAO_FP6(1, 8);
    TAO_FP6(1, 4);
  }
  if (tile.mt == 2) TAO_FP6(2, 4);
  if (tile.mt == 4) TAO_FP6(4, 2);
  TAO_FP6(8, 1);
#undef TAO_FP6
}

int check_fp6_format(const char* what, int ebits, int mbits) {
  TAO_CHECK_ARG(fp6_format_of(ebits, mbits) >= 0,
                "%s: (ebits, mbits) = (%d, %d) is not served; served: (3, 2) and (2, 3)", what,
                ebits, mbits);
  return TAO_OK;
}

}  // namespace

}  // namespace tao

extern "C" int tao_fp6_quantize_rows_bf16(const uint16_t* w, uint32_t* codes, uint16_t* scale,
                                          int64_t rows, int64_t K, int ebits, int mbits,
                                          void* stream) {
  using namespace tao;
  if (int rc = check_fp6_format("fp6 quantize", ebits, mbits)) return rc;
  TAO_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && K >= 0 && K % kFp6Group == 0 && K < (1LL << 31),
                "fp6 quantize: K (%lld) must be a multiple of 32", (long long)K);
  if (rows == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(codes, 8, "codes");
  TAO_CHECK_ALIGN(scale, 2, "scale");
  const uint4* w4 = reinterpret_cast<const uint4*>(w);
  if (fp6_format_of(ebits, mbits) == 0)
    launch(fp6_quantize_rows_kernel<0>, dim3((unsigned)rows), dim3(256), 0, as_stream(stream), w4,
           codes, scale, (int)K);
  else
    launch(fp6_quantize_rows_kernel<1>, dim3((unsigned)rows), dim3(256), 0, as_stream(stream), w4,
           codes, scale, (int)K);
  return check_launch("fp6_quantize_rows_kernel");
}

extern "C" int tao_fp6_dequant_bf16(const uint32_t* codes, const uint16_t* scale, uint16_t* w,
                                    int64_t N, int64_t K, int ebits, int mbits, void* stream) {
  using namespace tao;
  if (int rc = check_fp6_format("fp6 dequant", ebits, mbits)) return rc;
  TAO_CHECK_ARG(N >= 0 && K >= 0 && K % kFp6Group == 0 && K < (1LL << 31),
                "fp6 dequant: K (%lld) must be a multiple of 32", (long long)K);
  const int64_t ngroups = N * (K / kFp6Group);
  if (ngroups == 0) return TAO_OK;
  TAO_CHECK_ARG(ngroups / 256 < (1LL << 31), "fp6 dequant: tensor too large");
  TAO_CHECK_ALIGN(codes, 8, "codes");
  TAO_CHECK_ALIGN(scale, 2, "scale");
  TAO_CHECK_ALIGN(w, 16, "w");
  const dim3 grid((unsigned)((ngroups + 255) / 256));
  const u32x2_t* c2 = reinterpret_cast<const u32x2_t*>(codes);
  uint4* w4 = reinterpret_cast<uint4*>(w);
  if (fp6_format_of(ebits, mbits) == 0)
    launch(fp6_dequant_kernel<0>, grid, dim3(256), 0, as_stream(stream), c2, scale, w4, ngroups,
           (int)(K / kFp6Group));
  else
    launch(fp6_dequant_kernel<1>, grid, dim3(256), 0, as_stream(stream), c2, scale, w4, ngroups,
           (int)(K / kFp6Group));
  return check_launch("fp6_dequant_kernel");
}

extern "C" int tao_fp6_linear_route(int64_t M, int64_t N, int64_t K) {
  return tao::fp6_route(M, N, K, tao::tuning().fp6_route, tao::tuning().fp6_max_m);
}

extern "C" int tao_fp6_linear_bf16(const uint16_t* x, const uint32_t* codes, const uint16_t* scale,
                                   const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                                   int64_t K, int ebits, int mbits, void* stream) {
  using namespace tao;
  if (int rc = check_fp6_format("fp6 linear", ebits, mbits)) return rc;
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && M < (1LL << 31) && N < (1LL << 31) &&
                    K < (1LL << 31),
                "fp6 linear: K (%lld) must be positive and M, N, K below 2^31", (long long)K);
  TAO_CHECK_ARG(K % 64 == 0, "fp6 linear: K (%lld) must be a multiple of 64", (long long)K);
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(codes, 16, "codes");
  TAO_CHECK_ALIGN(scale, 2, "scale");
  TAO_CHECK_ALIGN(y, 2, "y");
  if (bias != nullptr) TAO_CHECK_ALIGN(bias, 2, "bias");
  const hipStream_t st = as_stream(stream);
  const Tuning& tu = tuning();
  const int fmt = fp6_format_of(ebits, mbits);
  const int grp = fp6_chunk_groups(tu.fp6_groups);
  // 8-token pieces: one launch wherever the route rule chose the GEMV, a sequence of them where
  // a caller forces it beyond (or calls this entry on a shape the op would dequantize)
  for (int64_t m0 = 0; m0 < M; m0 += kFp6GemvMaxM) {
    const int m = (int)(M - m0 < kFp6GemvMaxM ? M - m0 : kFp6GemvMaxM);
    const uint16_t* xm = x + m0 * K;
    uint16_t* ym = y + m0 * N;
    int rc;
    if (fmt == 0)
      rc = grp == 1 ? fp6_gemv<0, 1>(xm, codes, scale, bias, ym, m, (int)N, (int)K, st, tu)
                    : fp6_gemv<0, 2>(xm, codes, scale, bias, ym, m, (int)N, (int)K, st, tu);
    else
      rc = grp == 1 ? fp6_gemv<1, 1>(xm, codes, scale, bias, ym, m, (int)N, (int)K, st, tu)
                    : fp6_gemv<1, 2>(xm, codes, scale, bias, ym, m, (int)N, (int)K, st, tu);
    if (rc != TAO_OK) return rc;
  }
  return TAO_OK;
}

extern "C" int tao_tune_fp6(int route, int max_gemv_m, int rows_per_wave, int waves_k,
                            int row_groups, int chunk_groups) {
  using namespace tao;
  TAO_CHECK_ARG(route >= kFp6RouteAuto && route <= kFp6RouteDequantMm,
                "tune: fp6 route must be 0 (auto), 1 (gemv) or 2 (dequant + mm)");
  TAO_CHECK_ARG(max_gemv_m >= 0, "tune: fp6 max_gemv_m must be >= 0");
  TAO_CHECK_ARG(rows_per_wave == 0 || rows_per_wave == 2 || rows_per_wave == 4 ||
                    rows_per_wave == 8,
                "tune: fp6 rows_per_wave must be 0, 2, 4 or 8");
  TAO_CHECK_ARG(waves_k >= 0 && waves_k <= 8, "tune: fp6 waves_k must be in [0, 8]");
  TAO_CHECK_ARG(row_groups >= 0 && row_groups <= 8, "tune: fp6 row_groups must be in [0, 8]");
  TAO_CHECK_ARG(waves_k * row_groups <= 8, "tune: fp6 waves_k * row_groups must be <= 8");
  TAO_CHECK_ARG(chunk_groups >= 0 && chunk_groups <= 2,
                "tune: fp6 chunk_groups must be 0 (built-in), 1 (24 B) or 2 (48 B)");
  Tuning& tu = tuning();
  tu.fp6_route = route;
  tu.fp6_max_m = max_gemv_m;
  tu.fp6_rpw = rows_per_wave;
  tu.fp6_wk = waves_k;
  tu.fp6_g = row_groups;
  tu.fp6_groups = chunk_groups;
  return TAO_OK;
}
