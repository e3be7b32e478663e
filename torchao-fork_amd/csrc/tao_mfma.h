// What the MFMA skinny GEMMs (gemm_mfma.hip, gemm_i8_lds.hip, gemm32_int4.hip) and the format
// policies (gemm_mfma_policy.h) all use: the operand vector types, the bf16 packers, the two LDS
// swizzles, the workgroup order and static_for. Internal header; everything is file-local
// (anonymous namespace), so each kernel file keeps its own copy of the device helpers.
#pragma once

#include <type_traits>

#include "tao_common.h"

namespace tao {
namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// one v_cvt_pk_bf16_f32 (RNE, NaN-preserving)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

__device__ __forceinline__ bf16x8_t as_bf16x8(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  u32x4_t v = {a, b, c, d};
  return __builtin_bit_cast(bf16x8_t, v);
}

// The 8 int4 codes of one row-stream dword as the bf16 B fragment bf16(fma(q, s, z - 8 s)), given
// sc = s and zc = z - 8 s (q*s + zc == (q-8)*s + z). Row-stream nibble order (bits 4i: q[2i], bits
// 16+4i: q[2i+1]) puts q0,q4,q1,q5 in the bytes of w & 0x0F0F0F0F and q2,q6,q3,q7 in those of
// (w >> 4) & 0x0F0F0F0F. A byte b < 16 read as OCP e4m3 is exactly b / 512 (subnormals for b < 8,
// exponent 1 above), so one v_cvt_scalef32_pk_f32_fp8 with scale 512 turns two of them into exact
// fp32 integers; then one v_pk_fma_f32 and one v_cvt_pk_bf16_f32 per pair: ~1.9 VALU per weight.
__device__ __forceinline__ bf16x8_t int4x8_bf16(uint32_t w, float sc, float zc) {
  const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;
  const f32x2_t q04 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(lo, 512.f, false);
  const f32x2_t q15 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(lo, 512.f, true);
  const f32x2_t q26 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(hi, 512.f, false);
  const f32x2_t q37 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(hi, 512.f, true);
  const f32x2_t sv = {sc, sc}, zv = {zc, zc};
  const f32x2_t w04 = q04 * sv + zv, w15 = q15 * sv + zv;  // v_pk_fma_f32 (contracted)
  const f32x2_t w26 = q26 * sv + zv, w37 = q37 * sv + zv;
  return as_bf16x8(pack_bf16x2(w04[0], w15[0]), pack_bf16x2(w26[0], w37[0]),
                   pack_bf16x2(w04[1], w15[1]), pack_bf16x2(w26[1], w37[1]));
}

// 16 B under one AND mask (~0 / 0): a tail is zeroed by masks, never by a select on loaded data
__device__ __forceinline__ uint4 and16(const uint4& v, uint32_t k) {
  return make_uint4(v.x & k, v.y & k, v.z & k, v.w & k);
}

// Per-wave weight stage of 16 rows x 8 16-B slots (Int4WO, Int8WO). A ds_*_b128 pass is 16
// lanes of 16 B: conflict-free iff the 16 slots land in 16 distinct 16-B bank groups (slot index
// mod 16). The write passes cover rows {2i, 2i+1} x 8 slots; the read passes cover rows 0..15 at
// one slot. Swizzling the slot by (row >> 1) & 7 serves both (the row's parity supplies bit 3);
// the previous row & 7 gave rows n and n + 8 the same bank group on every read pass
// (SQ_LDS_BANK_CONFLICT 1.24-1.33 extra cycles per LDS cycle, profiles/r2_pmc_prefill.jsonl).
__device__ __forceinline__ int stage_slot(int row, int slot) {
  return row * 8 + (slot ^ ((row >> 1) & 7));
}

// LDS image of one x tile: [BM rows][16 slots of 16 B], slot XOR-swizzled with row & 15 so the
// 16 rows of an A fragment read spread over all banks (cdna guide §5.5 T2).
template <int SLOTS>
__device__ __forceinline__ int lds_slot(int row, int slot) {
  return row * SLOTS + (slot ^ (row & 15));
}

// Optional XCD-grouped workgroup order (tao_tune_gemm_order 1). Workgroups are dealt
// round-robin over the 8 XCDs (blocks b, b + 8, ... share one L2; which XCD is not fixed:
// MI355X_MICROARCH.md "Workgroup dispatch"). The M tiles of one (column tile, K slice) read the
// same weight bytes; grouped, those ny workgroups run back to back on one XCD and its L2 serves
// the re-reads. Measured (profiles/r2_pmc_prefill*.jsonl, r2_prefill_order_ab.txt): at M = 128,
// N = 28672 it cuts FETCH_SIZE from 2.2x to 1.26x the algorithmic bytes but runs 76 -> 80 us,
// and ties elsewhere: these GEMMs are bound by per-CU ingest, not HBM. So the plain grid order
// is the default. Speed only: any order is correct. Identity unless the grid divides into whole
// groups of 8 x ny.
struct TileId {
  int n, m, z;
};
__device__ __forceinline__ TileId xcd_tile(int order) {
  const int nx = gridDim.x, ny = gridDim.y, nz = gridDim.z;
  const int L = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
  const int T = nx * ny * nz;
  if (order != 1 || ny == 1 || T % (8 * ny) != 0)
    return TileId{(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
  const int xcd = L & 7, slot = L >> 3;
  const int gi = (slot / ny) * 8 + xcd;
  return TileId{gi % nx, slot % ny, gi / nx};
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

}  // namespace
}  // namespace tao
