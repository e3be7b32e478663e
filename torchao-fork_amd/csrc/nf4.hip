// NF4 (QLoRA) weight-only linear: block quantizer, flat dequantizer and the decode GEMV behind
// tao_nf4_quantize_blocks_bf16, tao_nf4_dequant_bf16 and tao_nf4_linear_bf16
// (torchao/dtypes/nf4tensor.py). The format's arithmetic is in nf4_block.h; the route rule and
// the GEMV's tile choice are in nf4_host.h.
//
// Replaces F.linear(x, weight.to(x.dtype)) of the reference's LinearNF4 (torchao/dtypes/
// nf4tensor.py:1037-1048), which rebuilds a bf16 copy of W with about ten eager torch ops on every
// call, and the numel x 16 difference tensor of its quantizer (:858-864).
//
// GEMV: the decomposition of tao_gemv.h with a 16-B chunk of 32 codes, so a slice is 2048 k of
// one row and a chunk is half a block: the lane builds its block's scaled level table once per
// chunk (16 multiplies, 8 roundings: bf16(level * s), the very w^ the dequantizer writes) and looks
// all 32 codes up with byte permutes; v_dot2c_f32_bf16 then takes the pairs with x as loaded.
#include "nf4_block.h"
#include "nf4_host.h"
#include "tao_gemv.h"

namespace tao {

namespace {

// ---- quantizer ------------------------------------------------------------------------------
// One thread per 8 weights (one 16-B load), 8 lanes per block: the block's absmax by three
// exchanges inside the lane octet, then 16 compares per weight in registers:
//   v = bf16(w / a), code = first j minimising bf16(|bf16(v - level[j])|), a NaN v takes code 0
// (every difference is NaN and torch.min returns the first; an all-zero block is 0 / 0).
__global__ __launch_bounds__(256) void nf4_quantize_blocks_kernel(
    const uint4* __restrict__ w, const uint16_t* __restrict__ levels, uint32_t* __restrict__ codes,
    uint16_t* __restrict__ absmax, int64_t npiece) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // npiece is a multiple of 8 and the grid is rounded up to whole workgroups of 256: an octet is
  // inside or outside as a whole, so the exchanges below never meet a returned lane.
  if (i >= npiece) return;
  const int lane = threadIdx.x & 63;
  float lv[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) lv[j] = bf16_to_f32(levels[j]);
  const uint4 v4 = w[i];
  const uint32_t d[4] = {v4.x, v4.y, v4.z, v4.w};
  float e[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    e[2 * j] = bf16lo_to_f32(d[j]);
    e[2 * j + 1] = bf16hi_to_f32(d[j]);
  }
  // max |w| with torch's NaN propagation: fmaxf drops NaNs, so they are tracked apart
  float a = 0.f;
  uint32_t nan = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a = fmaxf(a, fabsf(e[j]));
    nan |= (e[j] != e[j]) ? 1u : 0u;
  }
  a = fmaxf(a, xor_partner<1>(a, lane));
  nan |= xor_partner<1>(nan, lane);
  a = fmaxf(a, xor_partner<2>(a, lane));
  nan |= xor_partner<2>(nan, lane);
  // DPP row_half_mirror: lane ^ 7; after the two steps above the lanes of a quad agree, so this
  // is the other quad's value
  a = fmaxf(a, xor_partner<4>(a, lane));
  nan |= xor_partner<4>(nan, lane);
  if (nan) a = __uint_as_float(0x7FC00000u);
  if ((lane & 7) == 0) absmax[i >> 3] = f32_to_bf16(a);

  uint32_t out = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = round_bf16(e[j] / a);
    uint32_t best = 0u;
    float bd = round_bf16(fabsf(round_bf16(v - lv[0])));
#pragma unroll
    for (uint32_t c = 1; c < 16; ++c) {
      const float dd = round_bf16(fabsf(round_bf16(v - lv[c])));
      const bool lt = dd < bd;  // strict: the first of equal differences stays; NaN never wins
      best = lt ? c : best;
      bd = lt ? dd : bd;
    }
    // element 2 q + r of the piece -> byte q, high nibble for r == 0
    out |= best << (8 * (j >> 1) + ((j & 1) ? 0 : 4));
  }
  codes[i] = out;
}

// ---- dequantizer ------------------------------------------------------------------------------
// Flat and streaming: one thread per dword of codes (8 weights, 0.516 B in) and one 16-B store
// (2 B per weight out); blocks may straddle rows, the tensor's shape does not enter.
__global__ __launch_bounds__(256) void nf4_dequant_kernel(
    const uint32_t* __restrict__ codes, const int8_t* __restrict__ qs,
    const uint16_t* __restrict__ qf, const uint16_t* __restrict__ mean,
    const uint16_t* __restrict__ levels, uint4* __restrict__ w, int64_t npiece) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npiece) return;
  uint32_t lv[8];
  nf4_load_levels(levels, lv);
  const float s = nf4_block_scaler(qs, qf, bf16_to_f32(mean[0]), i >> 3);
  const Nf4Table t = nf4_scaled_table(lv, s);
  uint32_t o[4];
  nf4_decode8(t, ld_nt(codes + i), o);
  st_nt_u4(w + i, make_uint4(o[0], o[1], o[2], o[3]));
}

// ---- decode GEMV ------------------------------------------------------------------------------
// y[m][n] = bf16(sum_k x[m][k] * w^[n][k]) (+ bias -> bf16), fp32 sums. K % 64 == 0: a row is a
// whole number of blocks, so row n's block of chunk c is n * (K / 64) + c / 2.
template <int MT, int RPW>
__global__ __launch_bounds__(512) void nf4_gemv_kernel(
    const uint16_t* __restrict__ x, const uint4* __restrict__ w, const int8_t* __restrict__ qs,
    const uint16_t* __restrict__ qf, const uint16_t* __restrict__ mean,
    const uint16_t* __restrict__ levels, const uint16_t* __restrict__ bias,
    uint16_t* __restrict__ y, int M, int N, int K, int Wk, int G, int S) {
  constexpr int V = RPW * MT;
  extern __shared__ float red[];  // [G][Wk][V]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % Wk;
  const int rg = wave / Wk;
  const int row0 = (blockIdx.x * G + rg) * RPW;
  const int nchunk = K >> 5;  // 32-k (16-B) chunks per row
  const int nblk = K >> 6;    // blocks per row
  uint32_t lv[8];
  nf4_load_levels(levels, lv);
  const float mu = bf16_to_f32(mean[0]);

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
    float sc[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const int nn = n < N ? n : N - 1;
      wv[r] = ld_nt_u4(w + (size_t)nn * nchunk + cc);
      sc[r] = nf4_block_scaler(qs, qf, mu, (int64_t)nn * nblk + (cc >> 1));
    }
    // A lane past the row's last chunk loaded clamped (valid) addresses and skips the math: a
    // scaler may be NaN or inf, which 0 * w would not cancel.
    if (cval) {
      if constexpr (MT == 1) {
        // one token: x stays in registers, each row is decoded and consumed at once
        const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)cc * 32);
        uint32_t xd[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint4 a = xp[q];
          xd[4 * q] = a.x, xd[4 * q + 1] = a.y, xd[4 * q + 2] = a.z, xd[4 * q + 3] = a.w;
        }
#if TAO_NF4_FETCH == 2  // (variant build) x paired as nf4_decode8_split pairs the weights
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const uint32_t a = xd[2 * q], b = xd[2 * q + 1];
          xd[2 * q] = __builtin_amdgcn_perm(b, a, 0x05040100u);
          xd[2 * q + 1] = __builtin_amdgcn_perm(b, a, 0x07060302u);
        }
#endif
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          const Nf4Table t = nf4_scaled_table(lv, sc[r]);
          const uint32_t wd[4] = {wv[r].x, wv[r].y, wv[r].z, wv[r].w};
          float d = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            uint32_t p[4];
#if TAO_NF4_FETCH == 2
            nf4_decode8_split(t, wd[j], p);
#else
            nf4_decode8(t, wd[j], p);
#endif
#pragma unroll
            for (int i = 0; i < 4; ++i) d = dot2_bf16(xd[4 * j + i], p[i], d);
          }
          acc[r][0] += d;
        }
      } else {
        uint32_t wp[RPW][16];  // bf16 pairs (k, k + 1), in x's dword order
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          const Nf4Table t = nf4_scaled_table(lv, sc[r]);
          const uint32_t wd[4] = {wv[r].x, wv[r].y, wv[r].z, wv[r].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            uint32_t p[4];
            nf4_decode8(t, wd[j], p);
#pragma unroll
            for (int i = 0; i < 4; ++i) wp[r][4 * j + i] = p[i];
          }
        }
        // x is streamed one row of M at a time: 16 live dwords whatever M is.
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int mm = m < M ? m : M - 1;
          const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)mm * K + (size_t)cc * 32);
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
      // the fp32 sum rounded once; then + bias, rounded again (the reference's out + bias)
      float o = round_bf16(t.total);
      if (bias != nullptr) o = round_bf16(o + bf16_to_f32(bias[n]));
      y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

// wk, g: 0 = the default shape, Wk = min(S, 8) waves along K and as many row groups as fit 8 waves
// (M > 1), one row group at M == 1: the byte-weight GEMVs' choice (tao_gemv.h wo8_gemv).
template <int MT, int RPW>
int nf4_gemv_launch(const uint16_t* x, const uint8_t* w, const int8_t* qs, const uint16_t* qf,
                    const uint16_t* mean, const uint16_t* levels, const uint16_t* bias,
                    uint16_t* y, int M, int N, int K, hipStream_t stream, int wk, int g) {
  const GemvLaunchShape sh =
      gemv_launch_shape(K / 32, wk > 0 ? wk : 8, g > 0 ? g : (MT == 1 ? 1 : 8));
  const int rows_per_wg = sh.G * RPW;
  const int grid = (N + rows_per_wg - 1) / rows_per_wg;
  const size_t lds = (size_t)sh.G * sh.Wk * RPW * MT * sizeof(float);
  launch(nf4_gemv_kernel<MT, RPW>, dim3(grid), dim3(64 * sh.Wk * sh.G), lds, stream, x,
         reinterpret_cast<const uint4*>(w), qs, qf, mean, levels, bias, y, M, N, K, sh.Wk, sh.G,
         sh.S);
  return check_launch("nf4_gemv_kernel");
}

}  // namespace

}  // namespace tao

extern "C" int tao_nf4_quantize_blocks_bf16(const uint16_t* w, const uint16_t* levels,
                                            uint8_t* codes, uint16_t* absmax, int64_t numel,
                                            void* stream) {
  using namespace tao;
  TAO_CHECK_ARG(numel >= 0 && numel % kNf4Block == 0,
                "nf4 quantize: numel (%lld) must be a multiple of the block size 64",
                (long long)numel);
  TAO_CHECK_ARG(numel / 8 < (1LL << 31) * 256, "nf4 quantize: numel (%lld) too large",
                (long long)numel);
  if (numel == 0) return TAO_OK;
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(levels, 2, "levels");
  TAO_CHECK_ALIGN(codes, 4, "codes");
  TAO_CHECK_ALIGN(absmax, 2, "absmax");
  const int64_t npiece = numel / 8;
  launch(nf4_quantize_blocks_kernel, dim3((unsigned)((npiece + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint4*>(w), levels,
         reinterpret_cast<uint32_t*>(codes), absmax, npiece);
  return check_launch("nf4_quantize_blocks_kernel");
}

extern "C" int tao_nf4_dequant_bf16(const uint8_t* codes, const int8_t* qscalers,
                                    const uint16_t* qfactor, const uint16_t* mean,
                                    const uint16_t* levels, uint16_t* w, int64_t numel,
                                    void* stream) {
  using namespace tao;
  TAO_CHECK_ARG(numel >= 0 && numel % kNf4Block == 0,
                "nf4 dequant: numel (%lld) must be a multiple of the block size 64",
                (long long)numel);
  TAO_CHECK_ARG(numel / 8 < (1LL << 31) * 256, "nf4 dequant: numel (%lld) too large",
                (long long)numel);
  if (numel == 0) return TAO_OK;
  TAO_CHECK_ALIGN(codes, 4, "codes");
  TAO_CHECK_ALIGN(qfactor, 2, "qfactor");
  TAO_CHECK_ALIGN(mean, 2, "mean");
  TAO_CHECK_ALIGN(levels, 4, "levels");
  TAO_CHECK_ALIGN(w, 16, "w");
  const int64_t npiece = numel / 8;
  launch(nf4_dequant_kernel, dim3((unsigned)((npiece + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint32_t*>(codes), qscalers, qfactor, mean,
         levels, reinterpret_cast<uint4*>(w), npiece);
  return check_launch("nf4_dequant_kernel");
}

extern "C" int tao_nf4_linear_route(int64_t M, int64_t N, int64_t K) {
  return tao::nf4_route(M, N, K, tao::tuning().nf4_route, tao::tuning().nf4_max_m);
}

extern "C" int tao_nf4_linear_bf16(const uint16_t* x, const uint8_t* codes,
                                   const int8_t* qscalers, const uint16_t* qfactor,
                                   const uint16_t* mean, const uint16_t* levels,
                                   const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                                   int64_t K, void* stream) {
  using namespace tao;
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && M < (1LL << 31) && N < (1LL << 31) &&
                    K < (1LL << 31),
                "nf4 linear: K (%lld) must be positive and M, N, K below 2^31", (long long)K);
  TAO_CHECK_ARG(K % kNf4Block == 0, "nf4 linear: K (%lld) must be a multiple of the block size 64",
                (long long)K);
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(codes, 16, "codes");
  TAO_CHECK_ALIGN(qfactor, 2, "qfactor");
  TAO_CHECK_ALIGN(mean, 2, "mean");
  TAO_CHECK_ALIGN(levels, 4, "levels");
  TAO_CHECK_ALIGN(y, 2, "y");
  if (bias != nullptr) TAO_CHECK_ALIGN(bias, 2, "bias");
  const hipStream_t st = as_stream(stream);
  const Tuning& tu = tuning();
  // 8-token pieces: one launch wherever the route rule chose the GEMV, a sequence of them where
  // a caller forces it beyond (or calls this entry on a shape the op would dequantize)
  for (int64_t m0 = 0; m0 < M; m0 += kNf4GemvMaxM) {
    const int m = (int)(M - m0 < kNf4GemvMaxM ? M - m0 : kNf4GemvMaxM);
    const uint16_t* xm = x + m0 * K;
    uint16_t* ym = y + m0 * N;
    const Nf4GemvTile tile = nf4_gemv_tile(m);
    int rc;
#define TAO_NF4(MT, RPW)                                                                         \
  rc = nf4_gemv_launch<MT, RPW>(xm, codes, qscalers, qfactor, mean, levels, bias, ym, m, (int)N, \
                                (int)K, st, tu.nf4_wk, tu.nf4_g)
    if (tile.mt == 1) {
      if (tu.nf4_rpw == 2) TAO_NF4(1, 2);
      else if (tu.nf4_rpw == 8) TAO_NF4(1, 8);
      else TAO_NF4(1, 4);
    } else if (tile.mt == 2) TAO_NF4(2, 4);
    else if (tile.mt == 4) TAO_NF4(4, 2);
    else TAO_NF4(8, 1);
#undef TAO_NF4
    if (rc != TAO_OK) return rc;
  }
  return TAO_OK;
}

extern "C" int tao_tune_nf4(int route, int max_gemv_m, int rows_per_wave, int waves_k,
                            int row_groups) {
  using namespace tao;
  TAO_CHECK_ARG(route >= kNf4RouteAuto && route <= kNf4RouteDequantMm,
                "tune: nf4 route must be 0 (auto), 1 (gemv) or 2 (dequant + mm)");
  TAO_CHECK_ARG(max_gemv_m >= 0, "tune: nf4 max_gemv_m must be >= 0");
  TAO_CHECK_ARG(rows_per_wave == 0 || rows_per_wave == 2 || rows_per_wave == 4 ||
                    rows_per_wave == 8,
                "tune: nf4 rows_per_wave must be 0, 2, 4 or 8");
  TAO_CHECK_ARG(waves_k >= 0 && waves_k <= 8, "tune: nf4 waves_k must be in [0, 8]");
  TAO_CHECK_ARG(row_groups >= 0 && row_groups <= 8, "tune: nf4 row_groups must be in [0, 8]");
  TAO_CHECK_ARG(waves_k * row_groups <= 8, "tune: nf4 waves_k * row_groups must be <= 8");
  Tuning& tu = tuning();
  tu.nf4_route = route;
  tu.nf4_max_m = max_gemv_m;
  tu.nf4_rpw = rows_per_wave;
  tu.nf4_wk = waves_k;
  tu.nf4_g = row_groups;
  return TAO_OK;
}
