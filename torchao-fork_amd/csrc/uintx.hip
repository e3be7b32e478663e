// uintx (torch.uint1 .. torch.uint7) weight-only linear (UIntXWeightOnlyConfig): the decode GEMV
// and the dequantizer behind tao_uintx_linear_bf16 and tao_uintx_dequant_bf16
// (torchao/dtypes/uintx/uintx_layout.py). The measured boundary of the route rule, the GEMV's lane
// unit and where it reads x are in uintx_host.h; the rule, the GEMV's tile, launch and tail are the
// weight-only front end's (wo_host.h, tao_gemv.h). A third route, the UintxWO policy of gemm_mfma_kernel (gemm_mfma_policy.h), reads the
// same shards; tao_uintx_linear_bf16 reaches it through tao_tune_uintx_mfma until the route rule
// names it.
//
// Storage, read in place (the reference's UintxLayout shards, pack_dim = -1): a code of BITS bits
// is cut into its 4-, 2- and 1-bit parts (the set bits of BITS), each part a uint8 stream per row:
//   s4 [N][K/2], s2 [N][K/4], s1 [N][K/8].
// With K8 = K / 8 and element k = j K8 + i (segment j in 0..7, i in [0, K8)):
//   4-bit part: nibble j >> 2 of s4 byte (j & 3) K8 + i
//   2-bit part: field  j >> 1 of s2 byte (j & 1) K8 + i
//   1-bit part: bit    j      of s1 byte i
// so the U bytes at i .. i + U - 1 of each of the (up to) seven K8-long pieces hold the 8 U codes
// (j, i .. i + U - 1): one lane unit. The element order inside a unit is segment-strided, which a
// dot product does not mind as long as x is read in the same order.
//
//   dequantize:  w^[n][k] = bf16( bf16(q - zp) * s )          s bf16, zp int32, per (row, group)
//   linear:      y[m][n]  = bf16( sum_k x[m][k] (q - zp) s )  fp32 sums (+ bias -> bf16)
#include <type_traits>

#include "tao_gemm.h"
#include "tao_gemv.h"
#include "uintx_host.h"

namespace tao {

namespace {

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

template <int BITS>
struct UintxFmt {
  static_assert(BITS >= 1 && BITS <= 7, "1 to 7 bits");
  static constexpr bool kS4 = (BITS & 4) != 0, kS2 = (BITS & 2) != 0, kS1 = (BITS & 1) != 0;
  // bit position of the 2- and the 1-bit part inside a code
  static constexpr int kPos2 = kS4 ? 4 : 0, kPos1 = kPos2 + (kS2 ? 2 : 0);
};

// D dwords (4 D bytes, 4 D-byte aligned) of a streamed-once shard
template <int D>
__device__ __forceinline__ void uintx_ld(const uint8_t* __restrict__ p, uint32_t (&v)[D]) {
  if constexpr (D == 4) {
    const u32x4_t a = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
    v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3];
  } else if constexpr (D == 2) {
    const u32x2_t a = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
    v[0] = a[0], v[1] = a[1];
  } else {
    v[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
  }
}

// One lane unit of one row: D dwords of each piece of each shard the width has.
template <int BITS, int D>
struct UintxUnit {
  using F = UintxFmt<BITS>;
  uint32_t s4[F::kS4 ? 4 : 1][D], s2[F::kS2 ? 2 : 1][D], s1[D];

  // i0: the unit's first byte position (a multiple of 4 D, i0 + 4 D <= K8)
  __device__ __forceinline__ void load(const uint8_t* __restrict__ p4,
                                       const uint8_t* __restrict__ p2,
                                       const uint8_t* __restrict__ p1, size_t n, int K8, int i0) {
    if constexpr (F::kS4) {
#pragma unroll
      for (int h = 0; h < 4; ++h) uintx_ld<D>(p4 + (n * 4 + h) * (size_t)K8 + i0, s4[h]);
    }
    if constexpr (F::kS2) {
#pragma unroll
      for (int h = 0; h < 2; ++h) uintx_ld<D>(p2 + (n * 2 + h) * (size_t)K8 + i0, s2[h]);
    }
    if constexpr (F::kS1) uintx_ld<D>(p1 + n * (size_t)K8 + i0, s1);
  }

  // The codes of elements (j, i0 + 4 d .. + 3) as the four bytes of a dword: whole-dword shifts
  // and masks, no per-element work.
  __device__ __forceinline__ uint32_t codes4(int j, int d) const {
    uint32_t c = 0;
    if constexpr (F::kS4) c = (s4[j & 3][d] >> (4 * (j >> 2))) & 0x0F0F0F0Fu;
    if constexpr (F::kS2) c |= ((s2[j & 1][d] >> (2 * (j >> 1))) & 0x03030303u) << F::kPos2;
    if constexpr (F::kS1) c |= ((s1[d] >> j) & 0x01010101u) << F::kPos1;
    return c;
  }
};

// k / group without a division (and without the branches a select of two forms grows):
// gmul = ceil(2^32 / group), exact for k < K under uintx_shape_ok (uintx_host.h)
__device__ __forceinline__ int uintx_group_of(int k, uint32_t gmul) {
  return (int)__umulhi((uint32_t)k, gmul);
}

// ---- dequantizer ------------------------------------------------------------------------------
// Streaming: one thread per 8-byte unit (64 codes): up to seven 8-B loads in, eight 16-B stores
// out, one per segment, at column j K8 + i0 (consecutive threads write consecutive 16 B).
template <int BITS>
__global__ __launch_bounds__(256) void uintx_dequant_kernel(
    const uint8_t* __restrict__ s4, const uint8_t* __restrict__ s2, const uint8_t* __restrict__ s1,
    const uint16_t* __restrict__ scale, const int32_t* __restrict__ zp, uint16_t* __restrict__ w,
    int64_t nunits, int K8, int group, uint32_t gmul) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nunits) return;
  const int upr = K8 >> 3;
  const size_t n = (size_t)(idx / upr);
  const int i0 = (int)(idx % upr) << 3;
  const int ngrp = (K8 << 3) / group;
  UintxUnit<BITS, 2> u;
  u.load(s4, s2, s1, n, K8, i0);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = j * K8 + i0;
    const size_t gi = n * ngrp + uintx_group_of(k, gmul);
    const float s = bf16_to_f32(scale[gi]);
    const int z = zp[gi];
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const uint32_t c = u.codes4(j, d);
      uint16_t h[4];
#pragma unroll
      for (int b = 0; b < 4; ++b)
        h[b] = f32_to_bf16(round_bf16((float)((int)((c >> (8 * b)) & 0xFFu) - z)) * s);
      o[2 * d] = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
      o[2 * d + 1] = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
    }
    st_nt_u4(reinterpret_cast<uint4*>(w + n * ((size_t)K8 << 3) + k),
             make_uint4(o[0], o[1], o[2], o[3]));
  }
}

// ---- decode GEMV ------------------------------------------------------------------------------
// The decomposition of tao_gemv.h over the row's K / (8 U) units. Per segment j of a unit: the
// code dwords become bf16 pairs (128 + q) by one byte permute each (0x43 above a code <= 127 is the
// bf16 number 128 + q, exactly), then v_dot2_f32_bf16 against x as loaded gives
// dot = sum x (128 + q); sx = sum x is formed once per token (a dot2 against (1, 1)) and shared by
// the wave's rows; the unit adds s (dot - (zp + 128) sx) in fp32. A unit's U elements of one
// segment lie in one group (U divides the group size and K8). x: XL = false reads it through L1 (each
// of a token's 8 pieces is a coalesced 2 U-byte load per lane); XL = true (MT >= 4 only) stages the
// MT tokens once per workgroup in LDS behind the partials, [MT][K] bf16 (rows past M repeat the
// last token), and reads the same 2 U bytes from there. uintx_x_lds (uintx_host.h) picks, by
// measurement.
template <int BITS, int MT, int RPW, int U, bool XL>
__global__ __launch_bounds__(512) void uintx_gemv_kernel(
    const uint16_t* __restrict__ x, const uint8_t* __restrict__ s4, const uint8_t* __restrict__ s2,
    const uint8_t* __restrict__ s1, const uint16_t* __restrict__ scale,
    const int32_t* __restrict__ zp, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    int M, int N, int K, int group, uint32_t gmul, int Wk, int G, int S) {
  constexpr int V = RPW * MT;
  constexpr int D = U / 4;        // dwords of a shard piece per unit
  extern __shared__ __attribute__((aligned(16))) float red[];  // [G][Wk][V] | (XL) x [MT][K] bf16
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
  const int wk = wave % Wk;
  const int rg = wave / Wk;
  const int row0 = (blockIdx.x * G + rg) * RPW;
  const int K8 = K >> 3;
  const int nunit = K8 / U;
  const int ngrp = K / group;

  const uint16_t* xs = reinterpret_cast<const uint16_t*>(red + ((G * Wk * V + 3) & ~3));
  if constexpr (XL) {
    uint4* dst = reinterpret_cast<uint4*>(red + ((G * Wk * V + 3) & ~3));
    for (int i = threadIdx.x; i < MT * K8; i += (int)blockDim.x) {  // 16-B pieces, K8 per token
      const int m = i / K8, p = i - m * K8;
      dst[i] = reinterpret_cast<const uint4*>(x + (size_t)(m < M ? m : M - 1) * K)[p];
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
    const bool cval = c < nunit;
    const int i0 = (cval ? c : nunit - 1) * U;

    UintxUnit<BITS, D> wv[RPW];
    size_t qrow[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const size_t nn = (size_t)(n < N ? n : N - 1);
      wv[r].load(s4, s2, s1, nn, K8, i0);
      qrow[r] = nn * ngrp;
    }
    // A lane past the row's last unit loaded a clamped (valid) unit and adds nothing.
    if (cval) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = j * K8 + i0;
        const int gi = uintx_group_of(k, gmul);
        float sc[RPW], zf[RPW];
        uint32_t wp[RPW][2 * D];  // bf16 pairs (128 + q) of elements k .. k + U - 1, in x's order
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          sc[r] = bf16_to_f32(scale[qrow[r] + gi]);
          zf[r] = (float)zp[qrow[r] + gi] + 128.f;
#pragma unroll
          for (int d = 0; d < D; ++d) {
            const uint32_t q = wv[r].codes4(j, d);
            wp[r][2 * d] = __builtin_amdgcn_perm(0x43434343u, q, 0x04010400u);
            wp[r][2 * d + 1] = __builtin_amdgcn_perm(0x43434343u, q, 0x04030402u);
          }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int mm = m < M ? m : M - 1;
          const uint16_t* xp = XL ? xs + m * K + k : x + (size_t)mm * K + k;
          uint32_t xd[2 * D];
          if constexpr (D == 1) {
            const u32x2_t a = *reinterpret_cast<const u32x2_t*>(xp);
            xd[0] = a[0], xd[1] = a[1];
          } else {
#pragma unroll
            for (int q = 0; q < D / 2; ++q) {
              const uint4 a = reinterpret_cast<const uint4*>(xp)[q];
              xd[4 * q] = a.x, xd[4 * q + 1] = a.y, xd[4 * q + 2] = a.z, xd[4 * q + 3] = a.w;
            }
          }
          float sx = 0.f;
#pragma unroll
          for (int i = 0; i < 2 * D; ++i) sx = dot2_bf16(xd[i], 0x3F803F80u, sx);
#pragma unroll
          for (int r = 0; r < RPW; ++r) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 2 * D; ++i) d = dot2_bf16(xd[i], wp[r][i], d);
            acc[r][m] = fmaf(sc[r], fmaf(-zf[r], sx, d), acc[r][m]);
          }
        }
        // One segment's x and qparam loads in flight at a time: without the fence the scheduler
        // hoists all 8 MT of them above the first dot product and the V = 8 instances spill.
        __builtin_amdgcn_sched_barrier(0);
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
      float o = round_bf16(t.total);
      if (bias != nullptr) o = round_bf16(o + bf16_to_f32(bias[n]));
      y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

struct UintxArgs {
  const uint16_t* x;
  const uint8_t *s4, *s2, *s1;
  const uint16_t* scale;
  const int32_t* zp;
  const uint16_t* bias;
  uint16_t* y;
  int M, N, K, group;
  hipStream_t stream;
};

// wk, g: tao_tune_uintx's, 0 = the default shape (tao_gemv.h wo_gemv_launch)
template <int BITS, int MT, int RPW, int U, bool XL = false>
int uintx_gemv_launch(const UintxArgs& a, int wk, int g) {
  const WoGemvLaunch L = wo_gemv_launch(a.K / (8 * U), a.N, MT, RPW, wk, g);
  size_t lds = L.lds;
  if constexpr (XL) {
    lds = ((lds + 15) & ~(size_t)15) + uintx_x_lds_bytes(a.K, MT);
    // beyond 64 KiB a kernel's dynamic LDS has to be allowed first
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&uintx_gemv_kernel<BITS, MT, RPW, U, XL>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return set_error(TAO_ERR_HIP, "uintx linear: %zu bytes of LDS for the staged x refused", lds);
  }
  launch(uintx_gemv_kernel<BITS, MT, RPW, U, XL>, dim3(L.grid), dim3(L.threads), lds, a.stream, a.x,
         a.s4, a.s2, a.s1, a.scale, a.zp, a.bias, a.y, a.M, a.N, a.K, a.group,
         uintx_group_mul(a.group), L.Wk, L.G, L.S);
  return check_launch("uintx_gemv_kernel");
}

// The format's own two cases on top of the shared tile switch: 8 rows per wave never meet a
// 16-byte unit (uintx_unit caps it, so the <1, 8, 16> instances do not exist; the built-in 4 rows
// stand in), and the 4 x 2 and 8 x 1 tiles have an instance with x staged in LDS (uintx_x_lds).
template <int BITS, int U>
int uintx_gemv(const UintxArgs& a, const Tuning& tu) {
  return dispatch_gemv_tile(a.M, tu.uintx.rpw, [&](auto mt, auto rpw) {
    constexpr int MT = decltype(mt)::value, RPW = decltype(rpw)::value;
    if constexpr (MT == 1 && RPW == 8 && U == 16) {
      return uintx_gemv_launch<BITS, 1, 4, U>(a, tu.uintx.wk, tu.uintx.g);
    } else {
      if constexpr (MT >= 4) {
        if (uintx_x_lds(a.K, BITS, a.M, tu.uintx_xlds))
          return uintx_gemv_launch<BITS, MT, RPW, U, true>(a, tu.uintx.wk, tu.uintx.g);
      }
      return uintx_gemv_launch<BITS, MT, RPW, U>(a, tu.uintx.wk, tu.uintx.g);
    }
  });
}

// The one switch over the width: f is called with it as a compile-time constant.
template <typename F>
int dispatch_uintx_bits(int bits, F&& f) {
  switch (bits) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 7>{});
  }
}

int check_uintx_weight(const char* what, const uint8_t* s4, const uint8_t* s2, const uint8_t* s1,
                       const uint16_t* scale, const int32_t* zp, int64_t N, int64_t K, int bits,
                       int group) {
  TAO_CHECK_ARG(uintx_bits_ok(bits), "%s: bit width %d is not served; served: 1 to 7", what, bits);
  TAO_CHECK_ARG(N >= 0 && N < (1LL << 31) && K < (1LL << 31) && uintx_shape_ok(K, group),
                "%s: K (%lld) must be a positive multiple of 128 and the group size (%d) a "
                "multiple of 16 that divides K",
                what, (long long)K, group);
  TAO_CHECK_ARG((s4 != nullptr) == uintx_has_s4(bits) && (s2 != nullptr) == uintx_has_s2(bits) &&
                    (s1 != nullptr) == uintx_has_s1(bits),
                "%s: uint%d takes exactly the shards of its set bits (4-bit: %d, 2-bit: %d, "
                "1-bit: %d)",
                what, bits, (int)uintx_has_s4(bits), (int)uintx_has_s2(bits),
                (int)uintx_has_s1(bits));
  if (s4 != nullptr) TAO_CHECK_ALIGN(s4, 16, "int4_shard");
  if (s2 != nullptr) TAO_CHECK_ALIGN(s2, 16, "int2_shard");
  if (s1 != nullptr) TAO_CHECK_ALIGN(s1, 16, "int1_shard");
  TAO_CHECK_ALIGN(scale, 2, "scale");
  TAO_CHECK_ALIGN(zp, 4, "zero_point");
  return TAO_OK;
}

}  // namespace

}  // namespace tao

extern "C" int tao_uintx_dequant_bf16(const uint8_t* s4, const uint8_t* s2, const uint8_t* s1,
                                      const uint16_t* scale, const int32_t* zero_point,
                                      uint16_t* w, int64_t N, int64_t K, int bits, int group_size,
                                      void* stream) {
  using namespace tao;
  if (int rc = check_uintx_weight("uintx dequant", s4, s2, s1, scale, zero_point, N, K, bits,
                                  group_size))
    return rc;
  if (N == 0) return TAO_OK;
  TAO_CHECK_ALIGN(w, 16, "w");
  const int64_t nunits = N * (K / 64);
  TAO_CHECK_ARG(nunits / 256 < (1LL << 31), "uintx dequant: tensor too large");
  const dim3 grid((unsigned)((nunits + 255) / 256));
  const hipStream_t st = as_stream(stream);
  return dispatch_uintx_bits(bits, [&](auto b) {
    launch(uintx_dequant_kernel<decltype(b)::value>, grid, dim3(256), 0, st, s4, s2, s1, scale,
           zero_point, w, nunits, (int)(K / 8), group_size, uintx_group_mul(group_size));
    return check_launch("uintx_dequant_kernel");
  });
}

extern "C" int tao_uintx_linear_route_g(int64_t M, int64_t N, int64_t K, int bits,
                                        int group_size) {
  const tao::Tuning& tu = tao::tuning();
  (void)N;
  return tao::uintx_route(M, K, bits, group_size, tu.uintx.route, tu.uintx.max_m, tu.uintx_mfma);
}

extern "C" int tao_uintx_linear_route(int64_t M, int64_t N, int64_t K, int bits) {
  return tao_uintx_linear_route_g(M, N, K, bits, 0);
}

extern "C" int tao_uintx_gemv_unit(int64_t M, int64_t K, int bits) {
  const tao::Tuning& tu = tao::tuning();
  const int64_t m = M < tao::kWoGemvMaxM ? M : tao::kWoGemvMaxM;
  return tao::uintx_unit(K, bits, m, tu.uintx_unit, tu.uintx.rpw);
}

extern "C" int tao_uintx_gemv_x_lds(int64_t M, int64_t K, int bits) {
  const int64_t m = M < tao::kWoGemvMaxM ? M : tao::kWoGemvMaxM;
  return tao::uintx_x_lds(K, bits, m, tao::tuning().uintx_xlds) ? 1 : 0;
}

extern "C" int tao_uintx_linear_bf16(const uint16_t* x, const uint8_t* s4, const uint8_t* s2,
                                     const uint8_t* s1, const uint16_t* scale,
                                     const int32_t* zero_point, const uint16_t* bias, uint16_t* y,
                                     int64_t M, int64_t N, int64_t K, int bits, int group_size,
                                     void* stream) {
  using namespace tao;
  if (int rc = check_uintx_weight("uintx linear", s4, s2, s1, scale, zero_point, N, K, bits,
                                  group_size))
    return rc;
  TAO_CHECK_ARG(M >= 0 && M < (1LL << 31), "uintx linear: M (%lld) must be in [0, 2^31)",
                (long long)M);
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(y, 2, "y");
  if (bias != nullptr) TAO_CHECK_ALIGN(bias, 2, "bias");
  const Tuning& tu = tuning();
  // the UintxWO policy of gemm_mfma_kernel where the rule names it (tao_tune_uintx_mfma)
  if (uintx_route(M, K, bits, group_size, tu.uintx.route, tu.uintx.max_m, tu.uintx_mfma) ==
      kWoRouteMfma)
    return dispatch_uintx_bits(bits, [&](auto b) {
      return uintx_mm_launch<decltype(b)::value>(x, s4, s2, s1, scale, zero_point, bias, y, (int)M,
                                                 (int)N, (int)K, group_size, as_stream(stream));
    });
  return for_gemv_pieces(x, y, M, N, K, [&](const uint16_t* xm, uint16_t* ym, int m) {
    const UintxArgs a{xm,   s4, s2, s1,     scale,  zero_point,
                      bias, ym, m,  (int)N, (int)K, group_size, as_stream(stream)};
    const int unit = uintx_unit(K, bits, m, tu.uintx_unit, tu.uintx.rpw);
    return dispatch_uintx_bits(bits, [&](auto b) {
      constexpr int B = decltype(b)::value;
      if (unit == 4) return uintx_gemv<B, 4>(a, tu);
      if (unit == 8) return uintx_gemv<B, 8>(a, tu);
      return uintx_gemv<B, 16>(a, tu);
    });
  });
}

extern "C" int tao_tune_uintx_mfma(int on) {
  TAO_CHECK_ARG(on == 0 || on == 1, "tune: uintx mfma must be 0 (built-in route) or 1");
  tao::tuning().uintx_mfma = on;
  return TAO_OK;
}

extern "C" int tao_tune_uintx(int route, int max_gemv_m, int rows_per_wave, int waves_k,
                              int row_groups, int unit, int x_lds) {
  using namespace tao;
  if (int rc = check_wo_tune("uintx", route, max_gemv_m, rows_per_wave, waves_k, row_groups))
    return rc;
  TAO_CHECK_ARG(unit == 0 || unit == 4 || unit == 8 || unit == 16,
                "tune: uintx unit must be 0 (built-in), 4, 8 or 16 bytes");
  TAO_CHECK_ARG(x_lds >= 0 && x_lds <= 2,
                "tune: uintx x_lds must be 0 (built-in), 1 (through L1) or 2 (staged in LDS)");
  Tuning& tu = tuning();
  tu.uintx = {route, max_gemv_m, rows_per_wave, waves_k, row_groups};
  tu.uintx_unit = unit;
  tu.uintx_xlds = x_lds;
  return TAO_OK;
}
