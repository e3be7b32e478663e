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

#include "tao_gemm.h"
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

// ---- the int8 policy of wo8_decode_kernel (tao_gemv.h; tao_int8wo_decode_bf16): the chunk
// arithmetic of int8wo_gemv_kernel (written in place there: its M > 1 load schedule is sensitive
// to how the loop is written). The epilogues' a and b are the linear's own outputs
// bf16(bf16(sum) * scale[n]). ----
struct Int8Decode {
  using scale_t = uint16_t;  // bf16
  static constexpr const char* name = "int8wo_decode_kernel";
  static constexpr const char* what = "int8 decode";
  // a tail lane runs the math on a zeroed x: 0 * w adds nothing for every int8 w
  static constexpr bool kSkipTail = false;
  // 16 bf16 of x (two 16-B pieces; zeroed when !cval) as f32, and 128 * their sum
  struct X {
    float xf[16];
    float sx128;
  };
  static __device__ __forceinline__ X prep(uint4 a, uint4 b, bool cval) {
    const uint32_t d8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    X x;
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
  // the bytes are biased to unsigned (xor 0x80), converted with v_cvt_f32_ubyte{0..3} and FMA'd
  // against x in f32; the bias leaves as 128 * sum(x)
  static __device__ __forceinline__ float dot(const X& x, uint4 wv) {
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
  // bf16 mm, then * scale, as int8wo_gemv_kernel
  static __device__ __forceinline__ float out(float total, uint16_t scale) {
    return round_bf16(round_bf16(total) * bf16_to_f32(scale));
  }
  static __device__ __forceinline__ void flag_bad_kv_pos() { flag_decode_error(kDecodeErrKvPos); }
};

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
  const Wo8Want want = int8_decode_want(tuning().i8_rpw, tuning().i8_wk, tuning().i8_g);
  return dispatch_epilogue(epilogue, [&](auto epi) {
    return wo8_decode<Int8Decode, decltype(epi)::value>(x, w, scale, y, (int)N, (int)K, want, st,
                                                        fu);
  });
}
