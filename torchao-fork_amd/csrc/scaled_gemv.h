// The decode GEMV of the float8 (e4m3fn) activation linears: one kernel and one host path over a
// format policy, Fp8DynFmt (fp8_dyn.hip), MxFmt (mx_fp8.hip), Mx4Fmt (mx_fp4.hip) or BlockFp8Fmt
// (block_fp8.hip). Internal header.
//
// Common to the formats: the byte-weight decomposition of tao_gemv.h (a wave owns RPW rows and one
// slice of 64 16-B weight chunks at a time), both code streams decoded in hardware
// (v_cvt_scalef32_pk_bf16_fp8 with scale 1.0 is exact: every finite e4m3fn value is a bf16 number),
// one v_dot2c_f32_bf16 per code pair into an fp32 partial sum per chunk, tao_gemv.h's tail
// (wave_reduce_scatter -> wg_combine), the bias added in fp32 and one rounding to bf16. A lane past
// the row's last chunk loaded clamped, in-bounds addresses and skips the math: either side's codes
// may be NaN, which 0 * w would not cancel. NPT > 0 is the fused one-token launch (M == 1): x is
// the bf16 token, NPT 16-B pieces of it per thread (K <= 8 NPT threads); every workgroup quantises
// it into LDS under its first weight slice's latency and runs the GEMV on the codes.
//
// A policy F supplies
//   Args, name, what       ScaledGemvArgs of its stored scale type; what check_launch records; the
//                          prefix of error messages;
//   kChunkShift            log2 of the k in one 16-B weight chunk (4: e4m3fn, 5: e2m1);
//   kRowScales             one fp32 scale per token and per weight row, applied to the total:
//                          row_scaled(total, xs, ws). The fused launch finds the token's scale by a
//                          row-wide amax through LDS (two barriers). Otherwise a scale per block:
//   kBlockShift, Scale     log2 of the k in a block; a scale in a register;
//   scale_row(nn)          the row of the weight's scale array that weight row nn reads;
//   token_scale(xv)        the scale of the block that a token piece lies in, met across the lanes
//                          that share the block (no barrier); token_codes(xv, s): its 8 codes;
//   add(d, xb, wb, acc)    acc plus a chunk's partial sum d under the two block scales;
//   kFp4Weights            the weight chunk is a whole 32-k block of e2m1 codes against 32 B of x:
//                          x16_bf16<SWAP>, swap_nibbles, block_dot (mx_fp4.hip).
// The hooks take and return scalars, or one 16-B piece by value. The kernel's arrays (wv, xv, wp,
// xp, acc) stay in its own scope, and the formats' differences inside the loop are `if constexpr`
// branches on the policy's constants, each spelt as the format's own kernel spelt it: a hook that
// takes those arrays by reference, or a shared __device__ body behind one thin __global__ wrapper
// per format, compiled to other schedules and register counts.
#pragma once

#include "fp8_dyn_host.h"
#include "fp8_quant_row.h"
#include "tao_gemv.h"

namespace tao {

// codes (2 sel, 2 sel + 1) of a dword -> bf16 pair, exact; NaN codes (0x7F, 0xFF) stay NaN
template <bool HI>
__device__ __forceinline__ uint32_t e4m3_pair_bf16(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
}
// the 16 codes of a 16-B chunk -> 8 bf16 pairs (k, k + 1) in k order
__device__ __forceinline__ void e4m3_chunk_bf16(const uint4 v, uint32_t (&p)[8]) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[2 * j] = e4m3_pair_bf16<false>(d[j]);
    p[2 * j + 1] = e4m3_pair_bf16<true>(d[j]);
  }
}

// T: the stored type of a scale (fp32, or an E8M0 byte)
template <typename T>
struct ScaledGemvArgs {
  using scale_t = T;
  const void* x;         // e4m3fn codes [M][K] (fused: the bf16 token [K])
  const T* xs;           // token scales: [M], or [M][K / block] (unused when fused)
  const uint4* w;        // [N] rows of 16-B chunks of codes
  const T* ws;           // weight scales: [N], or [scale rows][K / block]
  const uint16_t* bias;  // [N] bf16 or null
  uint16_t* y;           // [M][N]
  int M, N, K, Wk, G, S;
};

template <typename F, int MT, int RPW, int NPT>
__global__ __launch_bounds__(512) void scaled_gemv_kernel(typename F::Args a) {
  constexpr bool FQ = NPT > 0;
  static_assert(!FQ || MT == 1, "the fused quantisation is one token, M == 1");
  constexpr bool kRow = F::kRowScales;
  constexpr int V = RPW * MT;
  // [G][Wk][V] fp32 partials | (FQ, row scales) [8] wave maxima | (FQ) the token's codes [K] |
  // (FQ, block scales) its scales [K / block]
  extern __shared__ float lds_f[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % a.Wk;
  const int rg = wave / a.Wk;
  const int row0 = (blockIdx.x * a.G + rg) * RPW;
  const int K = a.K, N = a.N, S = a.S, Wk = a.Wk;
  // Block scales: chunk cc lies in block cc >> kCB, and 2^kPB token pieces (8 bf16, one per
  // thread) make a block; nblk blocks per row. (Unused with row scales, as wmax is without them.
  // All of these are computed here, ahead of the first loads: computing wmax or nblk where it is
  // used moves the scalar instructions of the kernel's entry.)
  using Scale = typename F::Scale;
  constexpr int kCB = F::kBlockShift - F::kChunkShift, kPB = F::kBlockShift - 3;
  const int nchunk = K >> F::kChunkShift;  // 16-B weight chunks per row
  const int nblk = K >> F::kBlockShift;
  const int nw = a.G * a.Wk;
  float* wmax = lds_f + nw * V;
  uint4* xl = reinterpret_cast<uint4*>(lds_f + ((nw * V + 8 + 3) & ~3));
  auto* xsl = reinterpret_cast<typename F::Args::scale_t*>(reinterpret_cast<uint8_t*>(xl) + K);

  float acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

  // a slice's codes and the scale of the lane's block; rows, scale rows and chunks clamped in
  // bounds
  uint4 wv[RPW];
  Scale wsc[RPW];
  auto load_w = [&](int s) __attribute__((always_inline)) {
    const int c = s * 64 + lane;
    const int cc = c < nchunk ? c : nchunk - 1;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const size_t nn = (size_t)(n < N ? n : N - 1);
      wv[r] = ld_nt_u4(a.w + nn * nchunk + cc);
      if constexpr (!kRow) wsc[r] = a.ws[F::scale_row(nn) * nblk + (cc >> kCB)];
    }
  };

  float sx[MT];  // row scales: the tokens'
  if constexpr (FQ) {
    // The token's pieces are loaded BEFORE the first slice's weights: vector loads retire in
    // issue order, so the wait for x does not wait for the weights, and the quantisation into LDS
    // runs under the weight loads' latency.
    const uint4* xr = reinterpret_cast<const uint4*>(a.x);
    const int nvec = K >> 3;
    uint4 xv[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      xv[u] = xr[i < nvec ? i : nvec - 1];  // clamped duplicates do not change a max
    }
    load_w(wk);  // Wk <= S: every wave owns a slice
    uint2* xq = reinterpret_cast<uint2*>(xl);
    if constexpr (kRow) {
      float m = 0.f;
#pragma unroll
      for (int u = 0; u < NPT; ++u) m = fp8_amax8(xv[u], m);
      m = wave_max(m);
      if (lane == 0) wmax[wave] = m;
      __syncthreads();
      float amax = wmax[0];
      for (int w = 1; w < nw; ++w) amax = fmaxf(amax, wmax[w]);
      const float st = fp8_row_scale(amax);
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const int i = threadIdx.x + u * (int)blockDim.x;
        if (i < nvec) xq[i] = fp8_quant8(xv[u], st);
      }
      sx[0] = st;
    } else {
      // 2^kPB consecutive threads hold one block (K / 8 is a multiple of that, so a group is
      // whole or clamped as a whole); a block's scale depends on that block alone
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const int i = threadIdx.x + u * (int)blockDim.x;
        const Scale s = F::token_scale(xv[u]);
        if (i < nvec) {
          xq[i] = F::token_codes(xv[u], s);
          if ((i & ((1 << kPB) - 1)) == 0) xsl[i >> kPB] = (typename F::Args::scale_t)s;
        }
      }
    }
    __syncthreads();
  } else {
    load_w(wk);
    if constexpr (kRow) {
#pragma unroll
      for (int m = 0; m < MT; ++m) sx[m] = a.xs[m < a.M ? m : a.M - 1];
    }
  }

  for (int s = wk; s < S; s += Wk) {
    if (s != wk) load_w(s);
    const int c = s * 64 + lane;
    const bool cval = c < nchunk;
    const int cc = cval ? c : nchunk - 1;
    if (cval) {  // a lane past the row's last chunk skips the math
      if constexpr (F::kFp4Weights) {
        // The pairs of one side are put in the other's order where that takes fewer instructions
        // per block: the x side (2 v_perm_b32 per 16-B piece and token) or the weight side (3 per
        // dword and row, before the conversion).
        constexpr bool SWAPW = 12 * RPW < 8 * MT;
        if constexpr (SWAPW) {
#pragma unroll
          for (int r = 0; r < RPW; ++r) wv[r] = F::swap_nibbles(wv[r]);
        }
        // x is streamed one row of M at a time; its pairs serve the wave's RPW rows
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          uint4 x0, x1;
          Scale xb;
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
          F::template x16_bf16<!SWAPW>(x0, xp);
          F::template x16_bf16<!SWAPW>(x1, xp + 8);
#pragma unroll
          for (int r = 0; r < RPW; ++r)
            acc[r][m] = F::add(F::block_dot(xp, wv[r]), xb, wsc[r], acc[r][m]);
        }
      } else {
        uint32_t wp[RPW][8];
#pragma unroll
        for (int r = 0; r < RPW; ++r) e4m3_chunk_bf16(wv[r], wp[r]);
        // x is streamed one row of M at a time
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          uint4 xc;
          Scale xb;
          if constexpr (FQ) {
            xc = xl[cc];
            if constexpr (!kRow) xb = xsl[cc >> kCB];
          } else if constexpr (kRow) {
            const int mm = m < a.M ? m : a.M - 1;
            xc = reinterpret_cast<const uint4*>(a.x)[(size_t)mm * nchunk + cc];
          } else {
            const size_t mm = (size_t)(m < a.M ? m : a.M - 1);
            xc = reinterpret_cast<const uint4*>(a.x)[mm * nchunk + cc];
            xb = a.xs[mm * nblk + (cc >> kCB)];
          }
          uint32_t xp[8];
          e4m3_chunk_bf16(xc, xp);
#pragma unroll
          for (int r = 0; r < RPW; ++r) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) d = dot2_bf16(xp[i], wp[r][i], d);
            if constexpr (kRow)
              acc[r][m] += d;
            else
              acc[r][m] = F::add(d, xb, wsc[r], acc[r][m]);
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

  const WgTotal<float> t = wg_combine<V>(v[0], lds_f, lane, wk, rg, Wk);
  if (t.writer) {
    const int r = t.widx / MT, m = t.widx % MT;
    const int n = row0 + r;
    if (n < N && m < a.M) {
      // fp32: the total (row scales: times the token's scale, times the row's), plus the bias; one
      // rounding
      float o = t.total;
      if constexpr (kRow) {
        float xsm = sx[0];
#pragma unroll
        for (int i = 1; i < MT; ++i) xsm = (m == i) ? sx[i] : xsm;
        o = F::row_scaled(t.total, xsm, a.ws[n]);
      }
      if (a.bias != nullptr) o = o + bf16_to_f32(a.bias[n]);
      a.y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------
template <typename F, int MT, int RPW, int NPT>
int scaled_gemv_launch_npt(typename F::Args a, const Fp8DynLaunch& L, hipStream_t stream) {
  launch((scaled_gemv_kernel<F, MT, RPW, NPT>), dim3(L.grid), dim3(L.threads), L.lds, stream, a);
  return check_launch(F::name);
}

// One launch at rpw = RPW rows per wave and the wanted (wk, g) (fp8dyn_launch_shape). FQ: the
// fused one-token launch, instantiated for the token pieces a thread holds.
template <typename F, int MT, int RPW, bool FQ>
int scaled_gemv_launch(typename F::Args a, int wk, int g, hipStream_t stream) {
  const int scale_bytes =
      F::kRowScales ? 0 : (a.K >> F::kBlockShift) * (int)sizeof(typename F::Args::scale_t);
  const Fp8DynLaunch L =
      fp8dyn_launch_shape(a.N, a.K, RPW, MT, wk, g, FQ, 16, 1 << F::kChunkShift, scale_bytes);
  a.S = L.S;
  a.Wk = L.Wk;
  a.G = L.G;
  if constexpr (!FQ) {
    return scaled_gemv_launch_npt<F, MT, RPW, 0>(a, L, stream);
  } else {
    if (L.per <= 1) return scaled_gemv_launch_npt<F, MT, RPW, 1>(a, L, stream);
    if (L.per <= 2) return scaled_gemv_launch_npt<F, MT, RPW, 2>(a, L, stream);
    if (L.per <= 4) return scaled_gemv_launch_npt<F, MT, RPW, 4>(a, L, stream);
    if (L.per <= 8) return scaled_gemv_launch_npt<F, MT, RPW, 8>(a, L, stream);
    if (L.per <= 16) return scaled_gemv_launch_npt<F, MT, RPW, 16>(a, L, stream);
    TAO_CHECK_ARG(false, "%s dyn linear: K (%d) too long for the token prologue", F::what, a.K);
  }
  return TAO_OK;
}

// Ready-made codes, M tokens. M == 1: 4 rows per wave, Wk = min(S, 8), one row group
// (fp8wo_gemv_kernel's default shape); M > 1 keeps V = RPW * MT = 8 partials per lane, 8 waves per
// workgroup.
template <typename F>
int scaled_gemv(const typename F::Args& a, hipStream_t stream) {
  if (a.M <= 1) return scaled_gemv_launch<F, 1, 4, false>(a, 8, 1, stream);
  if (a.M <= 2) return scaled_gemv_launch<F, 2, 4, false>(a, 8, 8, stream);
  if (a.M <= 4) return scaled_gemv_launch<F, 4, 2, false>(a, 8, 8, stream);
  return scaled_gemv_launch<F, 8, 1, false>(a, 8, 8, stream);
}

// The fused one-token launch on the bf16 token: 8 rows per wave, 4 waves along K, 2 row groups.
// Every workgroup quantises the whole token (true fp32 divisions, for the byte-exact codes), so
// fewer, larger workgroups pay: 9.1 -> 7.1 us at 4096^2, 20.4 -> 14.2 us at 14336 x 4096 with row
// scales, best or within 4% of the best of ten shapes on the four README shapes
// (profiles/fp8dyn_fused_shape_ab.jsonl).
template <typename F>
int scaled_gemv_fused(const typename F::Args& a, hipStream_t stream) {
  return scaled_gemv_launch<F, 1, 8, true>(a, 4, 2, stream);
}

}  // namespace tao
