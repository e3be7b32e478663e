// The GEMV skeleton shared by the decode kernels (int4_gemv.hip, int8_gemv.hip, int8_dyn.hip,
// fp8_gemv.hip, scaled_gemv.h). Internal header.
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
//     row-pair epilogue (DecodeFuse, pair_epilogue); all five entries pick the
//     epilogue's instantiation through dispatch_epilogue.
// Each file keeps what is its own: the per-slice arithmetic, the prologue's LDS layout and its
// entries' argument checks. The byte-weight (int8 / fp8) weight-only kernels share
//   * at M >= 1 the launcher and M dispatcher of the plain GEMVs (wo8_gemv; one __global__
//     function per format, see there);
//   * at M == 1 with the decode fusions one kernel and one host path: wo8_decode_kernel over a
//     format policy (Int8Decode in int8_gemv.hip, Fp8Decode in fp8_gemv.hip: the chunk arithmetic,
//     whether tail lanes skip it, the scale type and the final rounding), wo8_decode_shape (the
//     launch shape as a plain function of N, K, the format's wanted shape and the norm; the two
//     formats' rules are int8_decode_want / fp8_decode_want) and wo8_decode (checks, dispatch).
// The float8-activation linears (fp8_dyn.hip, mx_fp8.hip, mx_fp4.hip, block_fp8.hip) share one
// kernel and one host path at every M, in scaled_gemv.h: scaled_gemv_kernel over a format policy
// (Fp8DynFmt, MxFmt, Mx4Fmt, BlockFp8Fmt, each in its format's file). A policy supplies where the
// scales live (per row, or per block with the weight's scale row), how a token piece finds its
// block's scale and codes in the fused one-token launch, how a chunk's partial sum enters the
// accumulator (or the total meets the row scales), and for e2m1 weights the block arithmetic;
// launcher, token-piece ladder and M dispatcher are scaled_gemv_launch / scaled_gemv, the launch
// shape fp8dyn_launch_shape (fp8_dyn_host.h).
#pragma once

#include <type_traits>

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

// The one switch over the epilogue: f is called with the epilogue as a compile-time constant,
//   dispatch_epilogue(epilogue, [&](auto epi) { return launch<decltype(epi)::value>(...); });
template <typename F>
static inline int dispatch_epilogue(int epilogue, F&& f) {
  switch (epilogue) {
    case kEpiSwiGLU: return f(std::integral_constant<int, kEpiSwiGLU>{});
    case kEpiRopeKV: return f(std::integral_constant<int, kEpiRopeKV>{});
    default: return f(std::integral_constant<int, kEpiNone>{});
  }
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

// ---- byte-weight weight-only decode (M == 1 with the fusions): one kernel, one host path -------
// The fusions above on a 1-B-per-weight stream, so an int8wo / float8wo Llama layer is 5 launches
// per token, as with int4 weights, instead of 9. A format policy F brings
//   scale_t                 the per-row scale's type;
//   X, prep(a, b, cval)     one 16-k chunk of x (two 16-B pieces) as the arithmetic wants it;
//   dot(x, wv)              sum_k x[k] * w[k] over the chunk;
//   kSkipTail               a lane past the row's last chunk skips the math (true) or runs it on
//                           an x that prep zeroed (false);
//   out(total, scale)       the linear's bf16 output, as float;
//   flag_bad_kv_pos()       flag_decode_error(kDecodeErrKvPos) on its file's error word;
//   name, what              what check_launch records; the prefix of error messages.
// Unlike the M > 1 GEMVs (above), the shared body costs nothing here: against the two kernels
// written out, every int8 instantiation compiles to the same VGPRs, scratch and occupancy, and
// the fp8 ones differ by a few VGPRs at unchanged occupancy (DESIGN.md §4.11 lists them).

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

// NPT > 0: the RMSNorm prologue, x normalised once per workgroup into LDS while the first weight
// slice is in flight (NPT 16-B pieces of x and of the norm weight per thread: K <= 8 NPT threads).
template <typename F, int RPW, int NPT, int EPI>
__global__ __launch_bounds__(512) void wo8_decode_kernel(
    const uint16_t* __restrict__ x, const uint4* __restrict__ w,
    const typename F::scale_t* __restrict__ scale, uint16_t* __restrict__ y, int N, int K, int Wk,
    int G, int S, DecodeFuse fu) {
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
    const typename F::X xc = F::prep(a, b, cval);
    if (!F::kSkipTail || cval) {
#pragma unroll
      for (int r = 0; r < RPW; ++r) acc[r] += F::dot(xc, wv[r]);
    }
  }

  float v[V];
#pragma unroll
  for (int r = 0; r < RPW; ++r) v[r] = acc[r];
  wave_reduce_scatter<V>(v, lane);
  const WgTotal<float> t = wg_combine<V>(v[0], red, lane, wk, rg, Wk);
  // the linear's bf16 output of row t.widx
  const int nrow = row0 + (t.widx < V ? t.widx : 0);
  const float o = F::out(t.total, scale[nrow < N ? nrow : N - 1]);
  if constexpr (EPI == kEpiNone) {
    if (t.writer && row0 + t.widx < N) y[row0 + t.widx] = f32_to_bf16(o);
  } else {
    pair_epilogue<EPI, RPW>(o, lane, wk, Wk, row0, N, y, fu, [] { F::flag_bad_kv_pos(); });
  }
}

// The launch shape a format wants: rows per wave (2, 4 or 8), waves along K, row groups, and
// whether row groups are added for a long K without the norm too (with it they always are).
struct Wo8Want {
  int rpw, wk, g;
  bool grow_plain;
};
// int8 (tao_tune_int8_gemv overrides each of the three): 4 rows per wave, Wk = min(S, 4), G = 2.
static inline Wo8Want int8_decode_want(int trpw, int twk, int tg) {
  return {trpw == 2 || trpw == 8 ? trpw : 4, twk > 0 ? twk : 4, tg > 0 ? tg : 2, true};
}
// fp8 (tao_tune_fp8_gemv overrides): without the norm, fp8wo_gemv_kernel's M == 1 shape: 4 rows
// per wave, Wk = min(S, 8) waves along K, one row group. With it every workgroup re-normalises
// the token, so fewer, larger workgroups pay: 8 rows per wave, 4 waves along K (fused, 4 x 8 x 1
// vs 8 x 4 x 1, us: 6144 x 4096 7.9 vs 7.5, 28672 x 4096 25.3 vs 20.8, the 128256 x 4096 head
// 93.2 vs 75.4, 10240 x 8192 20.2 vs 17.1, 57344 x 8192 93.2 vs 72.5;
// profiles/fp8_decode_shape_ab.jsonl).
static inline Wo8Want fp8_decode_want(int trpw, int twk, int tg, bool pro) {
  const int rpw = trpw > 0 ? trpw : (pro ? 8 : 4);
  return {rpw == 2 || rpw == 8 ? rpw : 4, twk > 0 ? twk : (pro ? 4 : 8), tg > 0 ? tg : 1, false};
}

// The prologue needs K <= 8 x NPT x threads, NPT <= 4, and has 16 slots for the waves' sums: row
// groups are added while they fit 8 waves. npt: 0 without the norm, -1 where K is too long.
struct Wo8DecodeLaunch {
  int rpw, S, Wk, G, threads, npt, grid;
  size_t lds;
};
static inline Wo8DecodeLaunch wo8_decode_shape(int N, int K, Wo8Want want, bool pro) {
  GemvLaunchShape sh = gemv_launch_shape(K / 16, want.wk, want.g);
  while ((pro || want.grow_plain) && sh.Wk * sh.G * 2 <= 8 && 64 * sh.Wk * sh.G * 8 * 4 < K)
    sh.G *= 2;
  Wo8DecodeLaunch L{want.rpw, sh.S, sh.Wk, sh.G, 64 * sh.Wk * sh.G, 0, 0, 0};
  const int64_t t8 = (int64_t)L.threads * 8;
  if (pro) L.npt = t8 >= K ? 1 : t8 * 2 >= K ? 2 : t8 * 4 >= K ? 4 : -1;
  const int rows_per_wg = L.G * L.rpw;
  L.grid = (int)(((int64_t)N + rows_per_wg - 1) / rows_per_wg);
  L.lds = (((size_t)L.G * L.Wk * L.rpw + 16 + 3) & ~(size_t)3) * sizeof(float) +
          (pro ? (size_t)K * 2 : 0);
  return L;
}

template <typename F, int RPW, int NPT, int EPI>
static int launch_wo8_decode(const uint16_t* x, const void* w, const typename F::scale_t* scale,
                             uint16_t* y, int N, int K, const Wo8DecodeLaunch& L,
                             hipStream_t stream, const DecodeFuse& fu) {
  launch((wo8_decode_kernel<F, RPW, NPT, EPI>), dim3(L.grid), dim3(L.threads), L.lds, stream, x,
         reinterpret_cast<const uint4*>(w), scale, y, N, K, L.Wk, L.G, L.S, fu);
  return check_launch(F::name);
}

template <typename F, int EPI>
static int wo8_decode(const uint16_t* x, const void* w, const typename F::scale_t* scale,
                      uint16_t* y, int N, int K, Wo8Want want, hipStream_t stream,
                      const DecodeFuse& fu) {
  const Wo8DecodeLaunch L = wo8_decode_shape(N, K, want, fu.norm_w != nullptr);
  if (L.threads > 512)
    return set_error(TAO_ERR_INVALID_ARGUMENT, "%s: %d waves along K exceed 8", F::what, L.Wk);
  if (L.npt < 0)
    return set_error(TAO_ERR_INVALID_ARGUMENT,
                     "%s: K (%d) too long for the RMSNorm prologue of %d threads", F::what, K,
                     L.threads);
#define TAO_WO8D(R, P) \
  return launch_wo8_decode<F, R, P, EPI>(x, w, scale, y, N, K, L, stream, fu)
#define TAO_WO8D_NPT(R)         \
  switch (L.npt) {              \
    case 0: TAO_WO8D(R, 0);     \
    case 1: TAO_WO8D(R, 1);     \
    case 2: TAO_WO8D(R, 2);     \
    default: TAO_WO8D(R, 4);    \
  }
  switch (L.rpw) {
    case 8: TAO_WO8D_NPT(8)
    case 2: TAO_WO8D_NPT(2)
    default: TAO_WO8D_NPT(4)
  }
#undef TAO_WO8D_NPT
#undef TAO_WO8D
}

}  // namespace tao
