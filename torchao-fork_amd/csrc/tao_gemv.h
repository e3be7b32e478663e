// The GEMV skeleton shared by the weight-only decode kernels (int4_gemv.hip, int8_gemv.hip,
// int8_dyn.hip, fp8_gemv.hip). Internal header.
//
// Work decomposition, common to all of them:
//   * a "slice" is one 1-KiB wave load of one weight row: 64 lanes x 16 B (1024 k of int8 / fp8
//     codes, 2048 k of int4 nibbles); lanes past the row's end load a clamped, in-bounds chunk
//     and add nothing;
//   * a wave owns RPW rows and one slice at a time; a workgroup is G row groups x Wk waves along
//     K, at most 8 waves (gemv_launch_shape); slices beyond Wk are looped;
//   * cross-lane: wave_reduce_scatter (tao_reduce.h) over the wave's RPW * MT partials;
//     cross-wave: LDS, wave wk == 0 of each row group finishes and writes (wg_combine);
//   * the M == 1 decode entries fuse the RMSNorm of x as a prologue (staged once per workgroup
//     in LDS under the first slice's load latency) and SwiGLU or RoPE + KV-cache write as a
//     row-pair epilogue (DecodeFuse, pair_epilogue).
// Each file keeps what is its own: the per-slice arithmetic, the prologue's LDS layout and the
// launch-shape defaults. The byte-weight (int8 / fp8) weight-only GEMVs share launcher and M
// dispatcher (wo8_gemv).
#pragma once

#include "tao_common.h"
#include "tao_reduce.h"

namespace tao {

// ---- decode-step fusions: arguments ------------------------------------------------------------
//   prologue    x -> bf16(bf16(x * rsqrt(mean(x^2) + eps)) * norm_w) (RMSNorm, norm_w != null);
//   kEpiSwiGLU  rows (2i, 2i+1) hold (w1_i, w3_i): y[i] = bf16(bf16(silu(a)) * b);
//   kEpiRopeKV  rows = [q | k | v] heads of wqkv: q rotated into y, k rotated and v stored into
//               the caches at pos[0] (a position outside [0, T) is reported, no cache row written).
// a and b are the linear's own bf16 outputs, so every result equals the unfused chain
// (decode_ops.hip: rmsnorm_kernel -> the linear -> silu_mul_kernel / rope_kv_kernel) bit for bit,
// up to the norm's fp32 sum order.
enum { kEpiNone = 0, kEpiSwiGLU = 1, kEpiRopeKV = 2 };
struct DecodeFuse {
  const uint16_t* norm_w;  // [K] RMSNorm weight, or null
  float eps;
  const float* freqs;      // [T][D/2] (cos, sin) pairs (kEpiRopeKV)
  const int64_t* pos;
  uint16_t* k_cache;       // [Hkv][T][D]
  uint16_t* v_cache;
  int H, Hkv, D, T;
};

// Host validation of the fusion arguments of a tao_*_decode_bf16 entry, in the two steps the
// entries make it in: check_decode_epilogue, then the entry's own checks (operand alignment, the
// norm weight's alignment, K limits: each format's, in its old place, so that a call with
// several bad arguments still reports the same one), then check_decode_fuse, which checks the
// rope_kv arguments and fills *fu. `what` prefixes the messages ("int4 decode", ...).
static inline int check_decode_epilogue(const char* what, int epilogue, int64_t N) {
  TAO_CHECK_ARG(epilogue >= kEpiNone && epilogue <= kEpiRopeKV,
                "%s: epilogue must be 0 (none), 1 (swiglu) or 2 (rope_kv)", what);
  TAO_CHECK_ARG(epilogue == kEpiNone || N % 2 == 0, "%s: N (%lld) must be even", what,
                (long long)N);
  return TAO_OK;
}
static inline int check_decode_fuse(const char* what, int epilogue, int64_t N,
                                    const uint16_t* norm_weight, float eps, const uint16_t* y,
                                    const float* freqs, const int64_t* pos, uint16_t* k_cache,
                                    uint16_t* v_cache, int64_t n_head, int64_t n_kv_head,
                                    int64_t head_dim, int64_t max_seq, DecodeFuse* fu) {
  fu->norm_w = norm_weight;
  fu->eps = eps;
  if (epilogue != kEpiRopeKV) return TAO_OK;
  TAO_CHECK_ARG(n_head > 0 && n_kv_head > 0 && head_dim > 0 && head_dim % 2 == 0 &&
                    max_seq > 0 && N == (n_head + 2 * n_kv_head) * head_dim,
                "%s rope_kv: N (%lld) must be (n_head + 2 n_kv_head) * head_dim", what,
                (long long)N);
  TAO_CHECK_ARG(freqs != nullptr && pos != nullptr && k_cache != nullptr && v_cache != nullptr,
                "%s rope_kv: freqs, pos and caches are required", what);
  TAO_CHECK_ALIGN(k_cache, 4, "k_cache");
  TAO_CHECK_ALIGN(v_cache, 4, "v_cache");
  TAO_CHECK_ALIGN(y, 4, "y");
  fu->freqs = freqs;
  fu->pos = pos;
  fu->k_cache = k_cache;
  fu->v_cache = v_cache;
  fu->H = (int)n_head;
  fu->Hkv = (int)n_kv_head;
  fu->D = (int)head_dim;
  fu->T = (int)max_seq;
  return TAO_OK;
}

// ---- launch shape --------------------------------------------------------------------------------
// S slices per row, Wk = min(wk, S) waves along K (every wave owns a slice), G row groups halved
// until the workgroup fits __launch_bounds__(512): Wk * G <= 8. Callers bring their own defaults
// for wk and g and grow G afterwards where a prologue needs more threads.
struct GemvLaunchShape {
  int S, Wk, G;
};
static inline GemvLaunchShape gemv_launch_shape(int nchunk, int wk, int g) {
  const int S = (nchunk + 63) / 64;
  const int Wk = wk < S ? wk : S;
  while (g > 1 && Wk * g > 8) g >>= 1;
  return {S, Wk, g};
}

// ---- cross-wave combine ----------------------------------------------------------------------------
// v0 is this lane's v[0] after wave_reduce_scatter<V>: the wave's total of value lane >> (6 - T)
// in the owner lanes (T = log2 V). Wk == 1: the owners write. Wk > 1: the owners park their
// totals in red[G][Wk][V], and lanes < V of wave wk == 0 sum the row group's Wk partials in wave
// order. Returns the total, the value index it belongs to and whether this lane writes it.
template <typename T>
struct WgTotal {
  T total;
  int widx;
  bool writer;
};
template <int V, typename T>
__device__ __forceinline__ WgTotal<T> wg_combine(T v0, T* red, int lane, int wk, int rg, int Wk) {
  constexpr int L = Log2<V>::value;
  const bool owner = (lane & ((64 >> L) - 1)) == 0;
  const int idx = lane >> (6 - L);
  WgTotal<T> t{v0, idx, owner};
  if (Wk > 1) {
    if (owner) red[(rg * Wk + wk) * V + idx] = v0;
    __syncthreads();
    t.writer = (wk == 0) && (lane < V);
    t.widx = lane;
    if (t.writer) {
      t.total = 0;
      for (int kk = 0; kk < Wk; ++kk) t.total += red[(rg * Wk + kk) * V + lane];
    }
  }
  return t;
}

// ---- row-pair epilogues (M == 1) -------------------------------------------------------------------
// Agent-scope (sc1) store: COH stores are read by other workgroups of the same launch
// (tao_int4wo_qkv_attn_bf16) after their ticket wait.
__device__ __forceinline__ void st_coh(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// o is the linear's bf16 output (as float) of the row wg_combine<RPW> gave this lane: row r's sits
// in lane r (Wk > 1) or in owner lane r << (6 - T) (Wk == 1). Row pair (2p, 2p+1) meets in lane p
// of the writing wave; every lane takes part in the shuffles. on_bad_pos() reports a KV position
// outside [0, T) (each translation unit has its own error word: TAO_DECODE_ERROR_WORD).
template <int EPI, int RPW, bool COH = false, typename F>
__device__ __forceinline__ void pair_epilogue(float o, int lane, int wk, int Wk, int row0, int N,
                                              uint16_t* __restrict__ y, const DecodeFuse& fu,
                                              F on_bad_pos) {
  static_assert(EPI == kEpiSwiGLU || EPI == kEpiRopeKV, "a row-pair epilogue");
  static_assert(RPW % 2 == 0, "row pairs stay inside one wave");
  const int sh = Wk > 1 ? 0 : 6 - Log2<RPW>::value;
  const int pl = lane < RPW / 2 ? lane : 0;
  const float a = __shfl(o, (2 * pl) << sh);
  const float b = __shfl(o, (2 * pl + 1) << sh);
  const int n = row0 + 2 * pl;
  if (!((Wk == 1 || wk == 0) && lane < RPW / 2 && n < N)) return;
  if constexpr (EPI == kEpiSwiGLU) {
    y[n >> 1] = f32_to_bf16(round_bf16(a / (1.f + __expf(-a))) * b);
  } else {
    const int D = fu.D, HD = fu.H * fu.D, KD = fu.Hkv * fu.D;
    int64_t p = fu.pos[0];
    const bool pok = p >= 0 && p < fu.T;  // KV cache row inside [0, T)
    if (!pok) {  // report (tao_decode_status) and write no cache row
      on_bad_pos();
      p = p < 0 ? 0 : fu.T - 1;
    }
    uint32_t ov = (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
    if (n < HD + KD) {
      const float2 cs = reinterpret_cast<const float2*>(fu.freqs)[p * (D >> 1) + ((n % D) >> 1)];
      const float o0 = a * cs.x - b * cs.y, o1 = b * cs.x + a * cs.y;
      ov = (uint32_t)f32_to_bf16(o0) | ((uint32_t)f32_to_bf16(o1) << 16);
    }
    if (n < HD) {
      if constexpr (COH) st_coh(reinterpret_cast<uint32_t*>(y) + (n >> 1), ov);
      else reinterpret_cast<uint32_t*>(y)[n >> 1] = ov;
    } else if (pok) {
      const int nk = n < HD + KD ? n - HD : n - HD - KD;
      uint16_t* cache = n < HD + KD ? fu.k_cache : fu.v_cache;
      const size_t off = ((size_t)(nk / D) * fu.T + p) * D + nk % D;
      if constexpr (COH) st_coh(reinterpret_cast<uint32_t*>(cache) + (off >> 1), ov);
      else reinterpret_cast<uint32_t*>(cache)[off >> 1] = ov;
    }
  }
}

// ---- RMSNorm prologue pieces -------------------------------------------------------------------
// bf16(bf16(x * r) * w) on a bf16 pair: rmsnorm_kernel's two roundings
__device__ __forceinline__ uint32_t rmsnorm_pair(uint32_t xv, uint32_t wv, float r) {
  const float lo = round_bf16(bf16lo_to_f32(xv) * r) * bf16lo_to_f32(wv);
  const float hi = round_bf16(bf16hi_to_f32(xv) * r) * bf16hi_to_f32(wv);
  return (uint32_t)f32_to_bf16(lo) | ((uint32_t)f32_to_bf16(hi) << 16);
}
__device__ __forceinline__ uint4 rmsnorm_piece(uint4 xv, uint4 wv, float r) {
  return make_uint4(rmsnorm_pair(xv.x, wv.x, r), rmsnorm_pair(xv.y, wv.y, r),
                    rmsnorm_pair(xv.z, wv.z, r), rmsnorm_pair(xv.w, wv.w, r));
}

// ss + the sum of squares of one 16-B piece of x (8 bf16), in element order; a piece past the
// end of x (!ok) was loaded clamped and counts as 0. The callers walk their pieces
// threadIdx.x + u * blockDim.x in order of u. (Taking the thread's whole xv[] array here costs
// int8wo_decode_kernel<2, 4, *> 9 VGPRs and one wave of occupancy.)
__device__ __forceinline__ float sumsq_piece(uint4 v, bool ok, float ss) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = ok ? bf16lo_to_f32(d[j]) : 0.f, b = ok ? bf16hi_to_f32(d[j]) : 0.f;
    ss = fmaf(a, a, fmaf(b, b, ss));
  }
  return ss;
}

// ---- byte-weight weight-only GEMV: host side ----------------------------------------------------
// int8wo_gemv_kernel and fp8wo_gemv_kernel are each written out as one __global__ function (their
// loops differ in the arithmetic and in fp8's skipped tail lanes) and share launcher and M
// dispatcher. A common __device__ body behind thin wrappers compiled to other load schedules at
// M > 1 (int8 <4, 2>: 7 of the slice's 12 loads issued before the first wait instead of 10) and
// measured 3-19% slower at M = 4, so it was not kept.
// A Kernel describes what to launch: scale_t, kernel<MT, RPW>() and the name check_launch records.
// wk, g: 0 = the default shape, Wk = min(S, 8) and as many row groups as fit 8 waves
template <typename Kernel, int MT, int RPW>
static int wo8_launch(const uint16_t* x, const void* w, const typename Kernel::scale_t* scale,
                      const uint16_t* bias, uint16_t* y, int M, int N, int K, hipStream_t stream,
                      int wk = 0, int g = 0) {
  const GemvLaunchShape sh = gemv_launch_shape(K / 16, wk > 0 ? wk : 8, g > 0 ? g : 8);
  const int rows_per_wg = sh.G * RPW;
  const int grid = (N + rows_per_wg - 1) / rows_per_wg;
  const size_t lds = (size_t)sh.G * sh.Wk * RPW * MT * sizeof(float);
  launch(Kernel::template kernel<MT, RPW>(), dim3(grid), dim3(64 * sh.Wk * sh.G), lds, stream, x,
         reinterpret_cast<const uint4*>(w), scale, bias, y, M, N, K, sh.Wk, sh.G, sh.S);
  return check_launch(Kernel::name);
}

// M == 1: rpw rows per wave (0 = 4), wk waves along K (0 = min(S, 8)), g row groups (0 = 1):
// experiments/sweep_int8.py, profiles/r1_sweep_int8.jsonl: 4 rows per wave, Wk = min(S, 8), G = 1
// is within 1% of the per-shape best on every Llama-3-8B linear (the head 77.8 -> 72.7 us).
// M > 1 keeps V = RPW * MT = 8 partials per lane on the default shape.
template <typename Kernel>
static int wo8_gemv(const uint16_t* x, const void* w, const typename Kernel::scale_t* scale,
                    const uint16_t* bias, uint16_t* y, int M, int N, int K, hipStream_t stream,
                    int rpw, int wk, int g) {
  if (M <= 1) {
    if (g <= 0) g = 1;
    if (rpw == 2) return wo8_launch<Kernel, 1, 2>(x, w, scale, bias, y, M, N, K, stream, wk, g);
    if (rpw == 8) return wo8_launch<Kernel, 1, 8>(x, w, scale, bias, y, M, N, K, stream, wk, g);
    return wo8_launch<Kernel, 1, 4>(x, w, scale, bias, y, M, N, K, stream, wk, g);
  }
  if (M <= 2) return wo8_launch<Kernel, 2, 4>(x, w, scale, bias, y, M, N, K, stream);
  if (M <= 4) return wo8_launch<Kernel, 4, 2>(x, w, scale, bias, y, M, N, K, stream);
  return wo8_launch<Kernel, 8, 1>(x, w, scale, bias, y, M, N, K, stream);
}

}  // namespace tao
