// int8 per-channel weight-only linear, skinny-M (decode) path:
//   y[m][n] = bf16( bf16( sum_k x[m][k] * w[n][k] ) * scale[n] ) (+ bias[n])
// Replaces torch.mm(x, w.t().to(bf16)) * scale at torchao/dtypes/uintx/plain_layout.py:256-266,
// which materialises a bf16 copy of W (2x the bytes) before a library GEMM; here W is read once.
//
// The byte-weight decomposition of tao_gemv.h (a slice is 1024 k of one row), and the M == 1
// decode-step fusions. Per lane: bytes are biased to unsigned (xor 0x80), converted with
// v_cvt_f32_ubyte{0..3} and FMA'd against x in f32; the bias is removed once per chunk as
// 128 * sum(x).
#include <atomic>

#include "tao_gemv.h"

namespace tao {

TAO_DECODE_ERROR_WORD(int8gemv_decode_status)

namespace {

template <int MT, int RPW>
__global__ __launch_bounds__(512) void int8wo_gemv_kernel(
    const uint16_t* __restrict__ x, const uint4* __restrict__ w,
    const uint16_t* __restrict__ scale, const uint16_t* __restrict__ bias,
    uint16_t* __restrict__ y, int M, int N, int K, int Wk, int G, int S) {
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
    // x is streamed one row of M at a time: 16 live f32 values whatever M is.
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int mm = m < M ? m : M - 1;
      const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)mm * K + (size_t)cc * 16);
      const uint4 a = xp[0], b = xp[1];
      const uint32_t d8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      float xf[16];
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t di = cval ? d8[i] : 0u;
        xf[2 * i] = bf16lo_to_f32(di);
        xf[2 * i + 1] = bf16hi_to_f32(di);
        t = dot2_bf16(di, 0x3F803F80u, t);
      }
      const float sx128 = 128.f * t;
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const uint32_t wd[4] = {wv[r].x ^ 0x80808080u, wv[r].y ^ 0x80808080u,
                                wv[r].z ^ 0x80808080u, wv[r].w ^ 0x80808080u};
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          d = fmaf(xf[4 * j + 0], (float)(wd[j] & 0xFF), d);
          d = fmaf(xf[4 * j + 1], (float)((wd[j] >> 8) & 0xFF), d);
          d = fmaf(xf[4 * j + 2], (float)((wd[j] >> 16) & 0xFF), d);
          d = fmaf(xf[4 * j + 3], (float)(wd[j] >> 24), d);
        }
        acc[r][m] += d - sx128;
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
      // bf16 mm output, then bf16 * scale, then + bias: the reference's three roundings.
      float o = round_bf16(round_bf16(t.total) * bf16_to_f32(scale[n]));
      if (bias != nullptr) o = round_bf16(o + bf16_to_f32(bias[n]));
      y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

struct Int8Gemv {  // what wo8_gemv launches
  using scale_t = uint16_t;  // bf16
  static constexpr const char* name = "int8wo_gemv_kernel";
  template <int MT, int RPW>
  static auto kernel() {
    return int8wo_gemv_kernel<MT, RPW>;
  }
};

// ---- pieces of int8wo_decode_kernel: the slice loader and the chunk arithmetic of int8wo_gemv_kernel
// (written in place there: its M > 1 load schedule is sensitive to how the loop is written) ----
// Slice s of rows row0 .. row0 + RPW: lane's chunk s * 64 + lane, row and chunk clamped in bounds.
template <int RPW>
__device__ __forceinline__ void load_w_slice(uint4 (&wv)[RPW], const uint4* __restrict__ w,
                                             int row0, int N, int nchunk, int s, int lane) {
  const int c = s * 64 + lane;
  const int cc = c < nchunk ? c : nchunk - 1;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int n = row0 + r;
    wv[r] = ld_nt_u4(w + (size_t)(n < N ? n : N - 1) * nchunk + cc);
  }
}

// 16 bf16 of x (two 16-B pieces; zeroed when !cval) as f32, and 128 * their sum
struct I8ChunkX {
  float xf[16];
  float sx128;
};
__device__ __forceinline__ I8ChunkX i8_chunk_x(uint4 a, uint4 b, bool cval) {
  const uint32_t d8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  I8ChunkX x;
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t di = cval ? d8[i] : 0u;
    x.xf[2 * i] = bf16lo_to_f32(di);
    x.xf[2 * i + 1] = bf16hi_to_f32(di);
    t = dot2_bf16(di, 0x3F803F80u, t);
  }
  x.sx128 = 128.f * t;
  return x;
}
// sum_k x[k] * w[k] over one chunk of int8 weights: the bytes are biased to unsigned (xor 0x80),
// converted with v_cvt_f32_ubyte{0..3} and FMA'd against x in f32; the bias leaves as 128 * sum(x)
__device__ __forceinline__ float i8_chunk_dot(const I8ChunkX& x, uint4 wv) {
  const uint32_t wd[4] = {wv.x ^ 0x80808080u, wv.y ^ 0x80808080u, wv.z ^ 0x80808080u,
                          wv.w ^ 0x80808080u};
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    d = fmaf(x.xf[4 * j + 0], (float)(wd[j] & 0xFF), d);
    d = fmaf(x.xf[4 * j + 1], (float)((wd[j] >> 8) & 0xFF), d);
    d = fmaf(x.xf[4 * j + 2], (float)((wd[j] >> 16) & 0xFF), d);
    d = fmaf(x.xf[4 * j + 3], (float)(wd[j] >> 24), d);
  }
  return d - x.sx128;
}

// ---- decode-step fusions of the M == 1 int8 weight-only GEMV (tao_int8wo_decode_bf16) -------
// The fusions of tao_gemv.h on the int8 weight stream, so an int8wo Llama layer
// is 5 launches per token, as with int4 weights, instead of 9. NPT > 0: the RMSNorm prologue,
// x normalised once per workgroup into LDS while the first weight slice is in flight. The
// epilogues' a and b are the linear's own outputs bf16(bf16(sum) * scale[n]).

template <int RPW, int NPT, int EPI>
__global__ __launch_bounds__(512) void int8wo_decode_kernel(
    const uint16_t* __restrict__ x, const uint4* __restrict__ w,
    const uint16_t* __restrict__ scale, uint16_t* __restrict__ y, int N, int K, int Wk, int G,
    int S, DecodeFuse fu) {
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
  uint4 wv[RPW];
  load_w_slice<RPW>(wv, w, row0, N, nchunk, wk, lane);  // Wk <= S: every wave owns a slice
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
      // piece i of 16-k chunk c = i >> 1 lands at 2 c + ((i + (c >> 3)) & 1): consecutive lanes
      // read 32-B chunks, the rotation puts the two halves of a pass on distinct bank groups
      if (i < nx) xs[(i & ~1) | ((i + (i >> 4)) & 1)] = rmsnorm_piece(xv[u], gv[u], r);
    }
    __syncthreads();
  }

  float acc[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) acc[r] = 0.f;
  for (int s = wk; s < S; s += Wk) {
    if (s != wk) load_w_slice<RPW>(wv, w, row0, N, nchunk, s, lane);
    const int c = s * 64 + lane;
    const bool cval = c < nchunk;
    const int cc = cval ? c : nchunk - 1;
    uint4 a, b;
    if constexpr (PRO) {
      const int rot = (cc >> 3) & 1;
      a = xs[2 * cc + rot];
      b = xs[2 * cc + (rot ^ 1)];
    } else {
      const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)cc * 16);
      a = xp[0];
      b = xp[1];
    }
    const I8ChunkX xc = i8_chunk_x(a, b, cval);
#pragma unroll
    for (int r = 0; r < RPW; ++r) acc[r] += i8_chunk_dot(xc, wv[r]);
  }

  float v[V];
#pragma unroll
  for (int r = 0; r < RPW; ++r) v[r] = acc[r];
  wave_reduce_scatter<V>(v, lane);
  const WgTotal<float> t = wg_combine<V>(v[0], red, lane, wk, rg, Wk);
  // the linear's bf16 output of row t.widx (bf16 mm, then * scale, as int8wo_gemv_kernel)
  const int nrow = row0 + (t.widx < V ? t.widx : 0);
  const float o = round_bf16(round_bf16(t.total) * bf16_to_f32(scale[nrow < N ? nrow : N - 1]));
  if constexpr (EPI == kEpiNone) {
    if (t.writer && row0 + t.widx < N) y[row0 + t.widx] = f32_to_bf16(o);
  } else {
    pair_epilogue<EPI, RPW>(o, lane, wk, Wk, row0, N, y, fu,
                            [] { flag_decode_error(kDecodeErrKvPos); });
  }
}

template <int RPW, int NPT, int EPI>
int launch_i8_decode(const uint16_t* x, const int8_t* w, const uint16_t* scale, uint16_t* y, int N,
                     int K, GemvLaunchShape sh, hipStream_t stream, const DecodeFuse& fu) {
  const int grid = (N + sh.G * RPW - 1) / (sh.G * RPW);
  const size_t lds = (((size_t)sh.G * sh.Wk * RPW + 16 + 3) & ~(size_t)3) * sizeof(float) +
                     (NPT > 0 ? (size_t)K * 2 : 0);
  launch((int8wo_decode_kernel<RPW, NPT, EPI>), dim3(grid), dim3(64 * sh.Wk * sh.G), lds, stream,
         x, reinterpret_cast<const uint4*>(w), scale, y, N, K, sh.Wk, sh.G, sh.S, fu);
  return check_launch("int8wo_decode_kernel");
}

template <int EPI>
int i8_decode(const uint16_t* x, const int8_t* w, const uint16_t* scale, uint16_t* y, int N, int K,
              hipStream_t stream, const DecodeFuse& fu) {
  // launch shape: Wk = min(S, 4) waves along K, 2 row groups, RPW rows per wave (tao_tune_int8_gemv
  // overrides); the prologue needs K <= 8 x NPT x threads and has 16 slots for the waves' sums
  const int trpw = tuning().i8_rpw, twk = tuning().i8_wk, tg = tuning().i8_g;
  GemvLaunchShape sh = gemv_launch_shape(K / 16, twk > 0 ? twk : 4, tg > 0 ? tg : 2);
  while (sh.Wk * sh.G * 2 <= 8 && 64 * sh.Wk * sh.G * 8 * 4 < K) sh.G *= 2;
  const int threads = 64 * sh.Wk * sh.G;
  if (threads > 512)
    return set_error(TAO_ERR_INVALID_ARGUMENT, "int8 decode: %d waves along K exceed 8", sh.Wk);
  const bool pro = fu.norm_w != nullptr;
  if (pro && threads * 8 * 4 < K)
    return set_error(TAO_ERR_INVALID_ARGUMENT, "int8 decode: K (%d) too long for the RMSNorm prologue", K);
  const int npt = !pro ? 0 : (threads * 8 >= K ? 1 : threads * 8 * 2 >= K ? 2 : 4);
#define TAO_I8D(R, P) return launch_i8_decode<R, P, EPI>(x, w, scale, y, N, K, sh, stream, fu)
  if (trpw == 8) {
    if (npt == 0) TAO_I8D(8, 0);
    if (npt == 1) TAO_I8D(8, 1);
    if (npt == 2) TAO_I8D(8, 2);
    TAO_I8D(8, 4);
  }
  if (trpw == 2) {
    if (npt == 0) TAO_I8D(2, 0);
    if (npt == 1) TAO_I8D(2, 1);
    if (npt == 2) TAO_I8D(2, 2);
    TAO_I8D(2, 4);
  }
  if (npt == 0) TAO_I8D(4, 0);
  if (npt == 1) TAO_I8D(4, 1);
  if (npt == 2) TAO_I8D(4, 2);
  TAO_I8D(4, 4);
#undef TAO_I8D
}

}  // namespace

int int8wo_gemv(const uint16_t* x, const int8_t* w, const uint16_t* scale, const uint16_t* bias,
                uint16_t* y, int64_t M, int64_t N, int64_t K, hipStream_t stream) {
  return wo8_gemv<Int8Gemv>(x, w, scale, bias, y, (int)M, (int)N, (int)K, stream,
                             tuning().i8_rpw, tuning().i8_wk, tuning().i8_g);
}

}  // namespace tao

extern "C" int tao_int8wo_decode_bf16(const uint16_t* x, const int8_t* w, const uint16_t* scale,
                                      int64_t N, int64_t K, const uint16_t* norm_weight,
                                      float eps, int epilogue, uint16_t* y, const float* freqs,
                                      const int64_t* pos, uint16_t* k_cache, uint16_t* v_cache,
                                      int64_t n_head, int64_t n_kv_head, int64_t head_dim,
                                      int64_t max_seq, void* stream) {
  using namespace tao;
  TAO_CHECK_ARG(N >= 0 && K > 0 && K % 16 == 0 && N < (1LL << 31) && K < (1LL << 31),
                "int8 decode: K (%lld) must be a positive multiple of 16", (long long)K);
  int rc = check_decode_epilogue("int8 decode", epilogue, N);
  if (rc != TAO_OK) return rc;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(y, 2, "y");
  if (norm_weight != nullptr) TAO_CHECK_ALIGN(norm_weight, 16, "norm_weight");
  DecodeFuse fu{};
  rc = check_decode_fuse("int8 decode", epilogue, N, norm_weight, eps, y, freqs, pos, k_cache,
                         v_cache, n_head, n_kv_head, head_dim, max_seq, &fu);
  if (rc != TAO_OK) return rc;
  if (N == 0) return TAO_OK;
  const hipStream_t st = as_stream(stream);
  switch (epilogue) {
    case kEpiSwiGLU: return i8_decode<kEpiSwiGLU>(x, w, scale, y, (int)N, (int)K, st, fu);
    case kEpiRopeKV: return i8_decode<kEpiRopeKV>(x, w, scale, y, (int)N, (int)K, st, fu);
    default: return i8_decode<kEpiNone>(x, w, scale, y, (int)N, (int)K, st, fu);
  }
}
