// The format policies of gemm_mfma_kernel (gemm_mfma.hip) and the parts they are built from.
//
// A policy is one struct: the kernel's operand pointers (it is the kernel argument), compile-time
// tile constants, and the per-lane weight path.
//   setup(): per-lane state for lane (n, kq) — descriptors and voffsets (once per launch).
//   load(): the raw bytes of the lane's weight piece for step `st` (wave-uniform, clamped to the
//   slice), never predicated: a select on a freshly loaded value makes hipcc wait for the load on
//   the spot, or branch around it, which collapses the prefetch pipeline. No weight is masked:
//   columns past N (clamped to row N - 1) are computed and dropped, and a K tail reads the next
//   row's finite weights against x that the LDS store zeroes (formats whose codes can be NaN zero
//   them instead: kMaskTail / mask_tail()). prep()/frag(): B fragments. slot(), xswz(): where
//   the matching A fragment lies in the x image. mfma() / mfma2() / mfma2s(): the instruction.
//   kRowF / kColF, row_factor() / col_factor(), epi(): the epilogue.
// Composition: PolicyDefaults holds what most formats share; LineLoader<STEP> is the full-line
// weight load and its per-wave stage regroup; ByteWeights<STEP> is the weight path of the
// one-byte formats on top of it; E8M0Scales<AL> is the scale-byte path of the MX formats. The
// parts hold the expressions the policies had when each was written out in full: sharing here
// must leave every kernel's instructions unchanged (experiments/asm_same.py), so an
// "equivalent" spelling is not a substitute for the one that is there.
#pragma once

#include "tao_mfma.h"

namespace tao {
namespace {

typedef int i32x8_t __attribute__((ext_vector_type(8)));

// the 32-B operand of the f8f6f4 MFMA from two 16-B pieces
__device__ __forceinline__ i32x8_t pair(const uint4& a, const uint4& b) {
  return i32x8_t{(int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y, (int)b.z, (int)b.w};
}

struct PolicyDefaults {
  static constexpr bool kMaskTail = false;     // weights past a K tail need no zeroing
  static constexpr int kASlots = 1;            // 16-B x slots one MFMA reads per lane
  static constexpr int kMaxKG = 4;             // k-groups per workgroup the policy is built for
  static constexpr bool kBlockScaled = false;  // the MFMAs take per-block scale bytes
  static constexpr bool kScaleAligned = false;  // ... a row's 8 per step are one aligned 8-B word
  static constexpr bool kBlockF32 = false;     // fp32 scales per 128-k block, applied per MFMA
  static constexpr bool kXPerm = false;        // x pieces pass through xperm() on their way to LDS
  typedef f32x4_t Acc;
  // x image mask (x_slot, gemm_mfma.hip)
  static __device__ __forceinline__ int xswz(int row) { return row & 15; }
  static __device__ __forceinline__ Acc mfma(const uint4& a, const bf16x8_t& b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), b, c, 0, 0, 0);
  }
  static constexpr bool kRowF = false, kColF = false;  // no per-row / per-column factor
  __device__ __forceinline__ const uint16_t* row_factor() const { return nullptr; }
  __device__ __forceinline__ const uint16_t* col_factor() const { return nullptr; }
};

// Weights in full 128-B lines: 8 rows x 128 B per wave instruction, lane l reads row 8 g + l / 8,
// bytes 128 h + 16 (l % 8) of the row's STEP bytes of the step (STEP 128: one line, two loads;
// 256: two lines, four loads), rows past N clamped. Measured ~1.4x over 16 rows x 64 B per
// instruction on the streaming-bound shapes. regroup() takes them to the MFMA layout through a
// per-wave LDS stage of [16 rows][STEP / 16 slots], the slot XOR-swizzled by row:
//   STEP 128 (2 KiB): stage_slot(); lane (n, kq) reads back slots kq and 4 + kq of row n;
//   STEP 256 (4 KiB): slot ^ row; lane (n, kq) reads back slots 4 s + kq: 15.1 -> ~11 us at
//   M=128, 4096^2 (experiments/gemm_debug.sh, 5/6).
template <int STEP>
struct LineLoader {
  struct Lane {
    Rsrc w;
    uint32_t wv0, wv1;
  };
  struct Chunk {
    uint4 v[STEP / 64];  // (g, h) = (0,0), (1,0), (0,1), (1,1); after regroup(): slot 4 s + kq
  };
  // rb: bytes per weight row. (Two steps because Int4WO makes its second descriptor between
  // them: in another order its kernels come out scheduled differently.)
  static __device__ __forceinline__ void offsets(Lane& L, uint32_t rb, int bn, int lane, int N) {
    const int base = bn - (lane & 15);  // the wave's first row
    const int r0 = base + (lane >> 3), r1 = r0 + 8;
    L.wv0 = (uint32_t)(r0 < N ? r0 : N - 1) * rb + 16 * (lane & 7);
    L.wv1 = (uint32_t)(r1 < N ? r1 : N - 1) * rb + 16 * (lane & 7);
  }
  static __device__ __forceinline__ Lane setup(const uint4* w, uint32_t rb, int bn, int lane,
                                               int N) {
    Lane L;
    L.w = make_rsrc(w, (uint32_t)N * rb);
    offsets(L, rb, bn, lane, N);
    return L;
  }
  static __device__ __forceinline__ Chunk load(const Lane& L, int st) {
    Chunk ch;
    ch.v[0] = bload16<kNT>(L.w, L.wv0, st * STEP);
    ch.v[1] = bload16<kNT>(L.w, L.wv1, st * STEP);
    if constexpr (STEP == 256) {
      ch.v[2] = bload16<kNT>(L.w, L.wv0 + 128, st * STEP);
      ch.v[3] = bload16<kNT>(L.w, L.wv1 + 128, st * STEP);
    }
    return ch;
  }
  static __device__ __forceinline__ Chunk regroup(const Chunk& ch, uint4* stage, int lane) {
    const int r = lane >> 3, c = lane & 7;
    const int n = lane & 15, kq = lane >> 4;
    Chunk p;
    if constexpr (STEP == 128) {
      stage[stage_slot(r, c)] = ch.v[0];
      stage[stage_slot(r + 8, c)] = ch.v[1];
      p.v[0] = stage[stage_slot(n, kq)];
      p.v[1] = stage[stage_slot(n, 4 + kq)];
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int row = r + 8 * (x & 1), slot = c + 8 * (x >> 1);
        stage[row * 16 + (slot ^ row)] = ch.v[x];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) p.v[s] = stage[n * 16 + ((4 * s + kq) ^ n)];
    }
    return p;
  }
  static constexpr int kStage = STEP;  // uint4 per wave
};

// The weight path of the one-byte formats (int8, e4m3fn), [N][K/16] 16-B pieces: STEP k per
// step, the lines regrouped and nothing else. After prep() lane (n, kq) holds, in v[s], bytes
// 64 s + 16 kq .. + 16 of row n's step.
template <int STEP>
struct ByteWeights : PolicyDefaults {
  const uint4* w;  // [N][K/16]
  static constexpr int kKStep = STEP;
  static constexpr int kStage = LineLoader<STEP>::kStage;
  typedef typename LineLoader<STEP>::Lane Lane;
  typedef typename LineLoader<STEP>::Chunk Chunk;
  typedef Chunk Prep;
  __device__ __forceinline__ Lane setup(int bn, int lane, int N, int K) const {
    return LineLoader<STEP>::setup(w, (uint32_t)K, bn, lane, N);
  }
  __device__ __forceinline__ Chunk load(const Lane& L, int st) const {
    return LineLoader<STEP>::load(L, st);
  }
  __device__ __forceinline__ Prep prep(const Chunk& ch, uint4* stage, int lane) const {
    return LineLoader<STEP>::regroup(ch, stage, lane);
  }
  // (kMaskTail formats) the codes past K zeroed. K % 16 == 0, so each 16-B piece is wholly inside
  // or wholly past the row (AND masks, no select)
  static __device__ __forceinline__ void mask_tail(Prep& p, int st, int kq, int K) {
    const int k0 = st * kKStep + 16 * kq;
#pragma unroll
    for (int s = 0; s < STEP / 64; ++s) {
      const uint32_t k = k0 + 64 * s < K ? ~0u : 0u;
      p.v[s] = and16(p.v[s], k);
    }
  }
  // STEP 128, two-byte x: lane (n, kq) holds k 16 kq .. +16 (v[0]) and 64 + 16 kq .. +16 (v[1]):
  // 8-k slots 2 kq, 2 kq + 1, 8 + 2 kq, 9 + 2 kq for MFMA s = 0..3.
  // STEP 256, one-byte x: load s covers 64 contiguous bytes of each row, i.e. MFMA s is the
  // contiguous k block 64 s .. +64 (16-B x slot 4 s + kq)
  static __device__ __forceinline__ int slot(int s, int kq) {
    if constexpr (STEP == 128)
      return (s >> 1) * 8 + kq * 2 + (s & 1);
    else
      return s * 4 + kq;
  }
};

struct Int4WO : PolicyDefaults {
  static constexpr int kPathId = 0;   // gemm_table.inc
  static constexpr int kABytes = 2;   // bf16 x
  static constexpr int kKStep = 256;  // 128 B of nibbles per row per step: one full line
  static constexpr int kMfma = 8;
  static constexpr int kMaxBM = 64;  // 512-B x rows: BM 128 would need 64 x VGPRs per stage
  static constexpr int kPrefKG = 2;
  static constexpr int kMinSlice = 4;  // steps per split-K slice (1024 k)
  // Weights in full lines (LineLoader<128>: 16-B chunk l % 8 of the step) regrouped through the
  // 2-KiB per-wave stage; lane (n, kq) then holds chunks kq and 4 + kq (32 k each, one
  // (scale, zero) dword each).
  typedef LineLoader<128> Lines;
  static constexpr int kStage = Lines::kStage;
  const uint4* wq;     // [N][K/32] 16-B chunks
  const uint32_t* sz;  // [N][K/g] (scale, zero)
  int gshift;          // log2(g / 32)
  struct Lane {
    Lines::Lane c;
    Rsrc z;
    uint32_t zv0, zv1;
  };
  struct Chunk {
    Lines::Chunk c;
    uint32_t sz0, sz1;
  };
  struct Prep {
    uint32_t w[8];  // dwords of chunks kq (0..3) and 4 + kq (4..7)
    float s0, zc0, s1, zc1;
  };
  __device__ __forceinline__ Lane setup(int bn, int lane, int N, int K) const {
    const int n = bn < N ? bn : N - 1, kq = lane >> 4;
    Lane L;
    const uint32_t zrow = (uint32_t)(K >> 5 >> gshift);  // (scale, zero) dwords per row
    L.c.w = make_rsrc(wq, (uint32_t)N * (uint32_t)(K >> 1));
    L.z = make_rsrc(sz, (uint32_t)N * zrow * 4u);
    Lines::offsets(L.c, (uint32_t)(K >> 1), bn, lane, N);
    // chunk 8 st + c -> group ((8 st) >> gshift) + (c >> gshift) (c < 8, gshift <= 3)
    L.zv0 = ((uint32_t)n * zrow + (kq >> gshift)) * 4;
    L.zv1 = ((uint32_t)n * zrow + ((4 + kq) >> gshift)) * 4;
    return L;
  }
  __device__ __forceinline__ Chunk load(const Lane& L, int st) const {
    Chunk ch;
    ch.c = Lines::load(L.c, st);
    const uint32_t zo = ((8 * st) >> gshift) * 4;
    ch.sz0 = bload4<kNT>(L.z, L.zv0, zo);
    ch.sz1 = bload4<kNT>(L.z, L.zv1, zo);
    return ch;
  }
  __device__ __forceinline__ Prep prep(const Chunk& ch, uint4* stage, int lane) const {
    const Lines::Chunk q = Lines::regroup(ch.c, stage, lane);
    const uint4 p0 = q.v[0], p1 = q.v[1];
    Prep p;
    p.w[0] = p0.x;
    p.w[1] = p0.y;
    p.w[2] = p0.z;
    p.w[3] = p0.w;
    p.w[4] = p1.x;
    p.w[5] = p1.y;
    p.w[6] = p1.z;
    p.w[7] = p1.w;
    p.s0 = bf16lo_to_f32(ch.sz0);
    p.zc0 = bf16hi_to_f32(ch.sz0) - 8.f * p.s0;  // q*s + zc == (q-8)*s + z
    p.s1 = bf16lo_to_f32(ch.sz1);
    p.zc1 = bf16hi_to_f32(ch.sz1) - 8.f * p.s1;
    return p;
  }
  // B fragment of MFMA s (chunk s >> 2, dword s & 3): int4x8_bf16 (tao_mfma.h) of its 8 nibbles
  __device__ __forceinline__ bf16x8_t frag(const Prep& p, int s) const {
    return int4x8_bf16(p.w[s], s < 4 ? p.s0 : p.s1, s < 4 ? p.zc0 : p.zc1);
  }
  // MFMA s = 4 h + t takes dword t of chunk 4 h + kq: x slot 4 (4 h + kq) + t
  static __device__ __forceinline__ int slot(int s, int kq) {
    return 16 * (s >> 2) + 4 * kq + (s & 3);
  }
  // x image mask (x_slot): m, with bit 2 flipped on rows m & 15 in 4..11 (bits 2 and 3 differ)
  static __device__ __forceinline__ int xswz(int row) {
    const int m = row & 15;
    return m ^ ((m ^ (m >> 1)) & 4);
  }
  // int4 output: bf16(acc) (+ bias added by the caller, tensor_core_tiled_layout.py:104-114)
  __device__ __forceinline__ float epi(float acc, float, float) const { return round_bf16(acc); }
};

struct Int8WO : ByteWeights<128> {
  static constexpr int kPathId = 1;
  static constexpr int kABytes = 2;
  static constexpr int kMfma = 4;
  static constexpr int kMaxBM = 128;
  static constexpr int kPrefKG = 2;
  static constexpr int kMinSlice = 8;
  const uint16_t* scale;  // [N]
  // int8 -> bf16 is exact: (q ^ 0x80) is q + 128 as an unsigned byte (one v_cvt_f32_ubyteN),
  // minus 128 in fp32 (exact), packed.
  __device__ __forceinline__ bf16x8_t frag(const Prep& p, int s) const {
    const uint4 &a = p.v[0], &b = p.v[1];
    const uint32_t d0 = ((s == 0) ? a.x : (s == 1) ? a.z : (s == 2) ? b.x : b.z) ^ 0x80808080u;
    const uint32_t d1 = ((s == 0) ? a.y : (s == 1) ? a.w : (s == 2) ? b.y : b.w) ^ 0x80808080u;
    auto cv = [](uint32_t d, int b) { return (float)((d >> (8 * b)) & 0xFF) - 128.f; };
    return as_bf16x8(pack_bf16x2(cv(d0, 0), cv(d0, 1)), pack_bf16x2(cv(d0, 2), cv(d0, 3)),
                     pack_bf16x2(cv(d1, 0), cv(d1, 1)), pack_bf16x2(cv(d1, 2), cv(d1, 3)));
  }
  // bf16 mm output, then * scale (plain_layout.py:258-262)
  static constexpr bool kColF = true;
  __device__ __forceinline__ const uint16_t* col_factor() const { return scale; }
  __device__ __forceinline__ float epi(float acc, float, float sc) const {
    return round_bf16(round_bf16(acc) * sc);
  }
};

// e4m3fn weights, one byte each like Int8WO: the same full-line loads, per-wave stage, k order
// and x image. The dequant step is the hardware decode: one v_cvt_scalef32_pk_bf16_fp8 (scale 1.0)
// per two codes, exact because every finite e4m3fn value is a bf16 number; x stays bf16 (the
// non-scaled fp8 MFMA runs at the bf16 rate, so quantising x would buy nothing).
struct Fp8WO : ByteWeights<128> {
  static constexpr int kPathId = 3;  // no measured table entries: the heuristic shapes
  // A K tail reads the next row's codes against zeroed x; unlike the integer formats a code can
  // be NaN (an all-zero row quantises to NaN codes) and 0 * NaN would reach the sum, so the
  // codes past K are zeroed after the stage read (mask_tail; K % 32 == 0).
  static constexpr bool kMaskTail = true;
  static constexpr int kABytes = 2;
  static constexpr int kMfma = 4;
  static constexpr int kMaxBM = 128;
  static constexpr int kPrefKG = 2;
  static constexpr int kMinSlice = 8;
  const float* scale;  // [N] fp32
  // (both masks before both ANDs: ByteWeights' loop compiles to another schedule here)
  static __device__ __forceinline__ void mask_tail(Prep& p, int st, int kq, int K) {
    const int k0 = st * kKStep + 16 * kq;
    const uint32_t ka = k0 < K ? ~0u : 0u, kb = k0 + 64 < K ? ~0u : 0u;
    p.v[0] = and16(p.v[0], ka);
    p.v[1] = and16(p.v[1], kb);
  }
  __device__ __forceinline__ bf16x8_t frag(const Prep& p, int s) const {
    const uint4 &a = p.v[0], &b = p.v[1];
    const uint32_t d0 = (s == 0) ? a.x : (s == 1) ? a.z : (s == 2) ? b.x : b.z;
    const uint32_t d1 = (s == 0) ? a.y : (s == 1) ? a.w : (s == 2) ? b.y : b.w;
    auto cv = [](uint32_t d, bool hi) {
      return hi ? __builtin_bit_cast(uint32_t,
                                     __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, true))
                : __builtin_bit_cast(uint32_t,
                                     __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, false));
    };
    return as_bf16x8(cv(d0, false), cv(d0, true), cv(d1, false), cv(d1, true));
  }
  // the fp32 sum times the fp32 scale, rounded once (include/torchao_mi355x.h)
  static constexpr bool kColF = true;
  __device__ __forceinline__ const float* col_factor() const { return scale; }
  __device__ __forceinline__ float epi(float acc, float, float sc) const {
    return round_bf16(acc * sc);
  }
};

struct Int8Dyn : ByteWeights<256> {
  static constexpr int kPathId = 2;
  static constexpr int kABytes = 1;  // int8 x
  static constexpr int kMfma = 4;
  static constexpr int kMaxBM = 128;
  static constexpr int kPrefKG = 1;
  static constexpr int kMinSlice = 4;
  typedef i32x4_t Acc;
  const uint16_t* wscale;   // [N]
  const uint16_t* xscale;   // [M]
  __device__ __forceinline__ i32x4_t frag(const Prep& p, int s) const {
    return __builtin_bit_cast(i32x4_t, p.v[s]);
  }
  static __device__ __forceinline__ Acc mfma(const uint4& a, const i32x4_t& b, Acc c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4_t, a), b, c, 0, 0, 0);
  }
  // bf16(c) * x_scale, * w_scale, each rounded (intmm.py:133-137, plain_layout.py:301-315)
  static constexpr bool kRowF = true, kColF = true;
  __device__ __forceinline__ const uint16_t* row_factor() const { return xscale; }
  __device__ __forceinline__ const uint16_t* col_factor() const { return wscale; }
  __device__ __forceinline__ float epi(int acc, float xs, float ws) const {
    const float v = round_bf16(round_bf16((float)acc) * xs);
    return round_bf16(v * ws);
  }
};

// Int8DynW4: int8 x (per-token fp32 scale), int4 W packed two per byte (per-row fp32 scale; W4A8,
// w4a8.hip) on Int8Dyn's MFMA, x image size (16 slots of 16 int8 per row and step) and 256-k step.
// W is 128 B per row and step, one full line: MxFp8Fp4's two loads per wave (LineLoader<128>),
// regrouped through the 2-KiB stage so that lane (n, kq) holds the 16-B pieces kq and 4 + kq of
// row n: k 32 kq .. + 32 and 128 + 32 kq .. + 32 of the step. MFMA s takes dwords (2 (s & 1),
// 2 (s & 1) + 1) of piece s >> 1, i.e. the 16 k of x slot 8 (s >> 1) + 2 kq + (s & 1): Int8WO's
// slot map on a 16-slot row, conflict-free under the plain row mask (x_slot, gemm_mfma.hip).
// Expansion: for a dword w of eight nibbles (storage: element 2 j in the low nibble of byte j),
// (w << 4) & 0xF0F0F0F0 and w & 0xF0F0F0F0 are its even and its odd elements times 16 as int8 lanes,
// so the B fragment of 16 k holds them in the order 0 2 4 6 | 1 3 5 7 | 8 10 12 14 | 9 11 13 15.
// A must agree per lane group: every 16-B x piece is permuted to that order once, on its way into
// the LDS image (kXPerm / xperm(), four v_perm_b32 per piece per workgroup), not per MFMA. The
// factor 16 leaves the exact int32 sum by an arithmetic shift in the epilogue; with it
// |acc| <= 16384 K < 2^31 for K < 131072 (checked by the entry). A K tail reads the next row's
// nibbles (or 0 past the buffer) against x zeroed at the LDS store: integers, adding exactly 0.
struct Int8DynW4 : PolicyDefaults {
  static constexpr int kPathId = 8;  // no measured table entries: the heuristic shapes
  static constexpr int kABytes = 1;  // int8 x
  static constexpr int kKStep = 256;
  static constexpr int kMfma = 4;
  static constexpr int kMaxBM = 128;
  static constexpr int kPrefKG = 1;
  static constexpr int kMinSlice = 4;
  static constexpr bool kXPerm = true;
  typedef i32x4_t Acc;
  typedef LineLoader<128> Lines;  // rows l / 8 and 8 + l / 8, bytes 16 (l % 8) of the step's 128
  static constexpr int kStage = Lines::kStage;
  typedef Lines::Lane Lane;
  typedef Lines::Chunk Chunk;
  typedef Lines::Chunk Prep;  // v[h]: nibbles of k 128 h + 32 kq .. + 32 of row n
  const uint4* w;        // [N][K/32] 16-B pieces of nibbles
  const float* wscale;   // [N] fp32
  const float* xscale;   // [M] fp32
  __device__ __forceinline__ Lane setup(int bn, int lane, int N, int K) const {
    return Lines::setup(w, (uint32_t)K >> 1, bn, lane, N);
  }
  __device__ __forceinline__ Chunk load(const Lane& L, int st) const { return Lines::load(L, st); }
  __device__ __forceinline__ Prep prep(const Chunk& ch, uint4* stage, int lane) const {
    return Lines::regroup(ch, stage, lane);
  }
  static __device__ __forceinline__ int slot(int s, int kq) {
    return (s >> 1) * 8 + kq * 2 + (s & 1);
  }
  // a 16-B x piece (16 int8 in element order) in the B fragment's order
  static __device__ __forceinline__ uint4 xperm(const uint4& v) {
    return make_uint4(__builtin_amdgcn_perm(v.y, v.x, 0x06040200u),
                      __builtin_amdgcn_perm(v.y, v.x, 0x07050301u),
                      __builtin_amdgcn_perm(v.w, v.z, 0x06040200u),
                      __builtin_amdgcn_perm(v.w, v.z, 0x07050301u));
  }
  __device__ __forceinline__ i32x4_t frag(const Prep& p, int s) const {
    const uint4& q = s < 2 ? p.v[0] : p.v[1];
    const uint32_t d0 = (s & 1) ? q.z : q.x, d1 = (s & 1) ? q.w : q.y;
    return i32x4_t{(int)((d0 << 4) & 0xF0F0F0F0u), (int)(d0 & 0xF0F0F0F0u),
                   (int)((d1 << 4) & 0xF0F0F0F0u), (int)(d1 & 0xF0F0F0F0u)};
  }
  static __device__ __forceinline__ Acc mfma(const uint4& a, const i32x4_t& b, Acc c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4_t, a), b, c, 0, 0, 0);
  }
  // fp32(fp32(fp32(acc) * xs) * ws), acc the sum without the expansion's 16; the bias add and
  // the one bf16 rounding follow in the kernel. No contraction, as Fp8Dyn::epi.
  static constexpr bool kRowF = true, kColF = true;
  __device__ __forceinline__ const float* row_factor() const { return xscale; }
  __device__ __forceinline__ const float* col_factor() const { return wscale; }
  __device__ __forceinline__ float epi(int acc, float xs, float ws) const {
#pragma clang fp contract(off)
    return ((float)(acc >> 4) * xs) * ws;
  }
};

// Fp8Dyn: e4m3fn x (per-token fp32 scale), e4m3fn W (per-row fp32 scale) on the block-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4 with E8M0 scale bytes 127 (2^0): a plain fp8 x fp8 MFMA with
// K = 128, at twice the bf16 rate. Int8Dyn's tile structure (1-byte x, 256-k steps, full-line
// weight loads through the per-wave stage, the same x image); an MFMA takes 32 B per lane of each
// operand, two of the template's 16-B slots (kASlots = 2): MFMA u of a step reads slots 2u and
// 2u + 1, i.e. lane (n, kq) holds k 128 u + 16 kq .. +16 and 128 u + 64 + 16 kq .. +16 on both
// sides. Any such assignment is correct as long as A and B agree per lane group kq, because the
// instruction pairs byte b of lane group kq of A with byte b of lane group kq of B
// (tests/test_gpu_exact_fp8dyn.py settles it with asymmetric exact data). Either operand can hold
// NaN codes (an all-zero token or weight row), so the weights past a K tail are zeroed as Fp8WO
// does; x past the tail is zeroed at the LDS store.
struct Fp8Dyn : ByteWeights<256> {
  static constexpr int kPathId = 4;  // no measured table entries: the heuristic shapes
  static constexpr bool kMaskTail = true;
  static constexpr int kABytes = 1;  // e4m3fn x
  static constexpr int kMfma = 2;
  static constexpr int kASlots = 2;  // 16-B x slots per MFMA
  static constexpr int kMaxBM = 128;
  static constexpr int kPrefKG = 1;
  static constexpr int kMaxKG = 2;  // 8 fragment registers per operand spill under the 1024-thread cap
  static constexpr int kMinSlice = 4;
  const float* wscale;   // [N] fp32
  const float* xscale;   // [M] fp32
  __device__ __forceinline__ i32x8_t frag(const Prep& p, int u) const {
    return u == 0 ? pair(p.v[0], p.v[1]) : pair(p.v[2], p.v[3]);
  }
  static __device__ __forceinline__ Acc mfma2(const uint4& a0, const uint4& a1, const i32x8_t& b,
                                              Acc c) {
    // cbsz 0 / blgp 0: both operands e4m3; scale bytes 127 = 2^0
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(pair(a0, a1), b, c, 0, 0, 0,
                                                            0x7F7F7F7F, 0, 0x7F7F7F7F);
  }
  // fp32(fp32(acc * xs) * ws); the bias add and the one bf16 rounding follow in the kernel. No
  // contraction: the product must be rounded to fp32 before the bias is added (fp8_dyn.hip).
  static constexpr bool kRowF = true, kColF = true;
  __device__ __forceinline__ const float* row_factor() const { return xscale; }
  __device__ __forceinline__ const float* col_factor() const { return wscale; }
  __device__ __forceinline__ float epi(float acc, float xs, float ws) const {
#pragma clang fp contract(off)
    return (acc * xs) * ws;
  }
};

// BlockFp8: e4m3fn x with one fp32 scale per 1 x 128 block ([M][K/128]) and e4m3fn W with one per
// 128 x 128 block ([ceil(N/128)][K/128]) (block_fp8.hip). Fp8Dyn's tile, x image, weight path, k
// order and unit E8M0 bytes; K = 128 of the instruction is one scale block, MFMA u of a step is
// block 2 st + u, and the k order inside an MFMA is immaterial under one scale. Each MFMA runs into
// a zero accumulator and the kernel then does acc = fma(P, xs * ws, acc) per element (kBlockF32):
//  * W: a wave's 16 columns start at a multiple of 16, so they lie in one 128-row scale block: the
//    scale is wave-uniform (every lane loads the same two floats per step, riding in the weight
//    ring); the scale row of a column past N is that of row N - 1, which is ceil(N/128) - 1.
//  * x: the step's BM x 2 floats are loaded by the k-group's threads (thread t: row t >> 1, block
//    t & 1), ride in the x ring and are stored beside the x image, double-buffered like it, as
//    [block][row]; a lane reads the four factors of its four C rows with one ds_read_b128.
// K % 256 == 128 is the only tail: the codes of the missing block are zeroed on both sides (mask_tail
// here, the LDS store for x) and both its scales are replaced by 0 (never a clamped neighbour's,
// which may be inf or NaN), so it adds exactly fma(0, 0, acc). A block index is clamped to
// K / 128 - 1 before any load. No row or column factor: the epilogue is the bias add and the one
// rounding.
struct BlockFp8 : ByteWeights<256> {
  static constexpr int kPathId = 7;  // no measured table entries: the heuristic shapes
  static constexpr bool kMaskTail = true;
  static constexpr bool kBlockF32 = true;
  static constexpr int kABytes = 1;  // e4m3fn x
  static constexpr int kMfma = 2;
  static constexpr int kASlots = 2;  // 16-B x slots per MFMA
  // 128-row tiles never won (M = 512: 31.7 vs 31.8 us on 4096^2, 61.1 vs 46.9 on 6144 x 4096,
  // 123.1 vs 119.9 on 14336 x 4096): at one wave per SIMD the products land in AGPRs and are
  // copied out one v_accvgpr_read each (gemm_mfma.hip, TAO_GEMM_WPE_ATTR)
  static constexpr int kMaxBM = 64;
  static constexpr int kPrefKG = 1;
  static constexpr int kMaxKG = 2;
  static constexpr int kMinSlice = 4;
  const float* wscale;   // [ceil(N/128)][K/128] fp32
  const float* xscale;   // [M][K/128] fp32
  typedef ByteWeights<256> Codes;  // w: [N][K/16] e4m3fn codes
  struct Lane {
    Codes::Lane c;
    const float* s;  // the wave's row of weight scales
    int nblk;
  };
  struct Chunk {
    Codes::Chunk c;
    float s0, s1;  // scales of blocks 2 st and 2 st + 1 (clamped to the row)
  };
  struct Prep {
    Codes::Prep c;  // v[s]: bytes 64 s + 16 kq .. + 16 of row n
    float s0, s1;   // mask_tail: a block past K / 128 -> 0
  };
  __device__ __forceinline__ Lane setup(int bn, int lane, int N, int K) const {
    Lane L;
    L.c = Codes::setup(bn, lane, N, K);
    L.nblk = K >> 7;
    L.s = wscale + (size_t)((bn < N ? bn : N - 1) >> 7) * L.nblk;
    return L;
  }
  __device__ __forceinline__ Chunk load(const Lane& L, int st) const {
    Chunk ch;
    ch.c = Codes::load(L.c, st);
    const int b0 = 2 * st, b1 = b0 + 1;
    ch.s0 = L.s[b0 < L.nblk ? b0 : L.nblk - 1];
    ch.s1 = L.s[b1 < L.nblk ? b1 : L.nblk - 1];
    return ch;
  }
  __device__ __forceinline__ Prep prep(const Chunk& ch, uint4* stage, int lane) const {
    Prep p;
    p.c = Codes::prep(ch.c, stage, lane);
    p.s0 = ch.s0;
    p.s1 = ch.s1;
    return p;
  }
  // the codes as Fp8Dyn masks them (16-B pieces); the scale of a block at or past K / 128 -> 0
  static __device__ __forceinline__ void mask_tail(Prep& p, int st, int kq, int K) {
    Codes::mask_tail(p.c, st, kq, K);
    p.s0 = st * kKStep < K ? p.s0 : 0.f;
    p.s1 = st * kKStep + 128 < K ? p.s1 : 0.f;
  }
  __device__ __forceinline__ i32x8_t frag(const Prep& p, int u) const {
    return u == 0 ? pair(p.c.v[0], p.c.v[1]) : pair(p.c.v[2], p.c.v[3]);
  }
  // cbsz 0 / blgp 0: both operands e4m3; scale bytes 127 = 2^0
  static __device__ __forceinline__ Acc mfma2(const uint4& a0, const uint4& a1, const i32x8_t& b,
                                              Acc c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(pair(a0, a1), b, c, 0, 0, 0,
                                                            0x7F7F7F7F, 0, 0x7F7F7F7F);
  }
  // the scaled accumulate of MFMA u's product: xf the lane's four C rows' activation scales
  static __device__ __forceinline__ Acc scaled_acc(const Acc& pr, const float4& xf, const Prep& p,
                                                   int u, Acc c) {
    const float w = u == 0 ? p.s0 : p.s1;
    c[0] = __builtin_fmaf(pr[0], xf.x * w, c[0]);
    c[1] = __builtin_fmaf(pr[1], xf.y * w, c[1]);
    c[2] = __builtin_fmaf(pr[2], xf.z * w, c[2]);
    c[3] = __builtin_fmaf(pr[3], xf.w * w, c[3]);
    return c;
  }
  __device__ __forceinline__ float epi(float acc, float, float) const { return acc; }
};

// The weight side of the E8M0 scale bytes of the MX formats ([N][K/32], one per 32-k block);
// the lane map is above MxFp8. Lane (i, kq) supplies the bytes of blocks kq and 4 + kq of the
// step, byte u of one VGPR for MFMA u.
template <bool AL>
struct E8M0Scales {
  struct Lane {
    const uint8_t* s;  // the lane's row of scale bytes
    int nblk, kq;
  };
  struct Bytes {
    // scale bytes of blocks kq and 4 + kq of the step (clamped to the row); AL: the step's 8
    // bytes of the row, blocks 0-3 and 4-7
    uint32_t s0, s1;
  };
  static __device__ __forceinline__ Lane setup(const uint8_t* wscale, int bn, int lane, int N,
                                               int K) {
    Lane L;
    L.nblk = K >> 5;
    L.kq = lane >> 4;
    L.s = wscale + (size_t)(bn < N ? bn : N - 1) * L.nblk;
    return L;
  }
  static __device__ __forceinline__ Bytes load(const Lane& L, int st) {
    Bytes ch;
    if constexpr (AL) {
      const uint2 v = *reinterpret_cast<const uint2*>(L.s + st * 8);
      ch.s0 = v.x;
      ch.s1 = v.y;
    } else {
      const int b0 = st * 8 + L.kq, b1 = b0 + 4;
      ch.s0 = L.s[b0 < L.nblk ? b0 : L.nblk - 1];
      ch.s1 = L.s[b1 < L.nblk ? b1 : L.nblk - 1];
    }
    return ch;
  }
  // byte u: the scale of block 4 u + kq. sh = 8 kq, passed in because the two callers' spellings
  // of it (8 * (lane >> 4), 8 * kq) do not compile alike
  static __device__ __forceinline__ uint32_t pack(const Bytes& ch, int sh) {
    if constexpr (AL) {
      return ((ch.s0 >> sh) & 0xFFu) | (((ch.s1 >> sh) & 0xFFu) << 8);
    } else {
      return ch.s0 | (ch.s1 << 8);
    }
  }
  // the bytes of blocks 4 u + kq at or past K / 32 replaced by 127 (2^0) against the zeroed codes
  static __device__ __forceinline__ uint32_t mask_tail(uint32_t sc, int st, int kq, int K) {
    const int b0 = st * 256 + 32 * kq;
    return (b0 < K ? sc & 0xFFu : 127u) | (b0 + 128 < K ? sc & 0xFF00u : 127u << 8);
  }
  // cbsz 0: A e4m3; BLGP 0: B e4m3, 4: B e2m1. MFMA u takes byte u of both scale VGPRs
  template <int BLGP>
  static __device__ __forceinline__ f32x4_t mfma2s(const uint4& a0, const uint4& a1,
                                                   const i32x8_t& b, f32x4_t c, int u,
                                                   uint32_t asc, uint32_t bsc) {
    const i32x8_t a = pair(a0, a1);
    return u == 0 ? __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, BLGP, 0,
                                                                      (int)asc, 0, (int)bsc)
                  : __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, BLGP, 1,
                                                                      (int)asc, 1, (int)bsc);
  }
};

// MxFp8: e4m3fn x and W with one E8M0 scale byte per 32-k block on both operands (MXFP8,
// mx_fp8.hip), the scales applied inside v_mfma_scale_f32_16x16x128_f8f6f4. Fp8Dyn's tile
// structure unchanged (1-byte x image, 256-k steps, full-line weight loads through the per-wave
// stage, the same k order, weights past a K tail zeroed) plus the scales.
// Layout of the instruction, as the exact-input test (tests/test_gpu_mx.py,
// test_scale_mapping_exact) establishes it:
//  * data: lane l = (i = l & 15, g = l >> 4) holds, in its first four operand VGPRs, k
//    16 g .. + 16 of the MFMA's 128 and, in its last four, k 64 + 16 g .. + 16: Fp8Dyn's order
//    (slots 2 u and 2 u + 1 of Int8Dyn::slot). A lane does NOT hold one whole 32-k block: its two
//    halves lie in blocks g >> 1 and 2 + (g >> 1).
//  * scales: the 32-k block j (k 32 j .. + 32) of row i (A: output row, B: output column) is
//    scaled by the byte that lane i + 16 j supplies, in the byte of its scale VGPR that opsel
//    names. (Giving lane group g the contiguous k 32 g .. + 32 instead scaled half of blocks 0
//    and 3 and nothing of blocks 1 and 2.)
// So lane (i, kq) supplies the scale of block 4 u + kq of the step for MFMA u, whatever k it
// holds itself. It packs the bytes of its two MFMAs of a step into one VGPR (byte u) and MFMA u
// selects byte u by opsel. W: two byte loads per lane and step, riding in the weight ring. x: the
// step's BM x 8 bytes are loaded by the k-group's threads (thread t: row t >> 3 (+ 32 i), block
// t & 7), ride in the x ring and are stored beside the x image, double-buffered like it, as
// [row][kq][u]; an A fragment read takes its two bytes with one ds_read_u16. A block at or past
// K / 32 is never read (the index is clamped) and its byte is replaced by 127 (2^0) against the
// zeroed codes: a stray 0xFF would make 0 * w NaN.
// AL (K % 256 == 0; tao_mx_scaled_mm_bf16 then wants both scale arrays 8-B aligned, so every
// step's 8 bytes of a row are one aligned 8-B word, and there is no K tail): one 8-B load per lane
// replaces the two byte loads of W, and thread t < BM loads the 8 bytes of x row t, permutes them
// to [kq][u] with two v_perm_b32 and stores them with one ds_write_b64.
// No row or column factor: the epilogue is the bias add and the one rounding.
template <bool AL>
struct MxFp8 : ByteWeights<256> {
  static constexpr int kPathId = 5;  // no measured table entries: the heuristic shapes
  static constexpr bool kMaskTail = !AL;
  static constexpr bool kBlockScaled = true;
  static constexpr bool kScaleAligned = AL;
  static constexpr int kABytes = 1;  // e4m3fn x
  static constexpr int kMfma = 2;
  static constexpr int kASlots = 2;  // 16-B x slots per MFMA
  static constexpr int kMaxBM = 128;
  static constexpr int kPrefKG = 1;
  static constexpr int kMaxKG = 2;
  static constexpr int kMinSlice = 4;
  const uint8_t* wscale;   // [N][K/32] E8M0 bytes
  const uint8_t* xscale;   // [M][K/32] E8M0 bytes
  typedef ByteWeights<256> Codes;  // w: [N][K/16] e4m3fn codes
  typedef E8M0Scales<AL> Scales;
  struct Lane {
    Codes::Lane c;
    typename Scales::Lane s;
  };
  struct Chunk {
    Codes::Chunk c;
    typename Scales::Bytes s;
  };
  struct Prep {
    Codes::Prep c;  // v[s]: bytes 64 s + 16 kq .. + 16 of row n
    uint32_t sc;    // byte u: the scale of block 4 u + kq (mask_tail: tails -> 127)
  };
  __device__ __forceinline__ Lane setup(int bn, int lane, int N, int K) const {
    Lane L;
    L.c = Codes::setup(bn, lane, N, K);
    L.s = Scales::setup(wscale, bn, lane, N, K);
    return L;
  }
  __device__ __forceinline__ Chunk load(const Lane& L, int st) const {
    Chunk ch;
    ch.c = Codes::load(L.c, st);
    ch.s = Scales::load(L.s, st);
    return ch;
  }
  __device__ __forceinline__ Prep prep(const Chunk& ch, uint4* stage, int lane) const {
    Prep p;
    p.c = Codes::prep(ch.c, stage, lane);
    p.sc = Scales::pack(ch.s, 8 * (lane >> 4));
    return p;
  }
  // the codes as Fp8Dyn masks them (16-B pieces); the scale bytes of blocks 4 u + kq past K / 32
  static __device__ __forceinline__ void mask_tail(Prep& p, int st, int kq, int K) {
    Codes::mask_tail(p.c, st, kq, K);
    p.sc = Scales::mask_tail(p.sc, st, kq, K);
  }
  __device__ __forceinline__ i32x8_t frag(const Prep& p, int u) const {
    return u == 0 ? pair(p.c.v[0], p.c.v[1]) : pair(p.c.v[2], p.c.v[3]);
  }
  // blgp 0: both operands e4m3
  static __device__ __forceinline__ Acc mfma2s(const uint4& a0, const uint4& a1, const i32x8_t& b,
                                               Acc c, int u, uint32_t asc, uint32_t bsc) {
    return Scales::template mfma2s<0>(a0, a1, b, c, u, asc, bsc);
  }
  __device__ __forceinline__ float epi(float acc, float, float) const { return acc; }
};

// MxFp8Fp4: MxFp8 with an e2m1 W (MXFP4 weights, mx_fp4.hip): cbsz 0 (A e4m3), blgp 4 (B e2m1,
// four operand VGPRs). MxFp8's tile, x image, x scale array, 256-k step, two MFMAs per step and
// scale bytes unchanged; W is 128 B per row and step, one full line, so a wave loads its 16 rows
// with two instructions (lane l: row 8 h + l / 8, bytes 16 (l % 8)) instead of four.
// Layout of the B operand, as the one-MFMA probe with one-hot data measured it
// (experiments/probe_fp4_layout.hip; the exact k map of tests/test_gpu_mxfp4.py holds it):
//  * lane (i, g) holds, in its four VGPRs, the 32 contiguous k 32 g .. + 32 of the MFMA's 128,
//    in A's numbering (where lane (i, g) holds k 16 g .. + 16 and 64 + 16 g .. + 16, see MxFp8):
//    VGPR d, nibble p (p = 0 the lowest four bits) is k 32 g + 8 d + p. So, unlike A, a lane holds
//    one whole block: block g, the one whose scale byte it supplies.
//  * the even element is the LOW nibble. Storage has it in the high nibble (the reference's
//    packing), so the nibbles of every byte are swapped after the stage read (a shift each way
//    and one bit-field insert per dword); the stored bytes are never changed.
// So for MFMA u of a step lane (n, kq) takes the 16 B of block 4 u + kq of row n: slot 4 u + kq
// of the row's eight 16-B slots in the per-wave stage ([16 rows][8 slots], XOR-swizzled by
// row >> 1: the 16 lanes of each ds_read_b128 pass, rows {0-3, 12-15} of one kq and {4-11} of the
// next, hit 16 distinct 16-B granules). A 16-B piece is a whole block, inside the row or past
// it: mask_tail zeroes it and replaces its scale byte by 127, as MxFp8 does.
template <bool AL>
struct MxFp8Fp4 : PolicyDefaults {
  static constexpr int kPathId = 6;  // no measured table entries: the heuristic shapes
  static constexpr bool kMaskTail = !AL;
  static constexpr bool kBlockScaled = true;
  static constexpr bool kScaleAligned = AL;
  static constexpr int kABytes = 1;  // e4m3fn x
  static constexpr int kKStep = 256;
  static constexpr int kMfma = 2;
  static constexpr int kASlots = 2;  // 16-B x slots per MFMA
  static constexpr int kMaxBM = 128;
  static constexpr int kPrefKG = 1;
  static constexpr int kMaxKG = 2;
  static constexpr int kMinSlice = 4;
  const uint4* w;          // [N][K/32] 16-B blocks of e2m1 codes, element 2 j in the high nibble
  const uint8_t* wscale;   // [N][K/32] E8M0 bytes
  const uint8_t* xscale;   // [M][K/32] E8M0 bytes
  typedef LineLoader<128> Lines;  // rows l / 8 and 8 + l / 8, bytes 16 (l % 8) of the step's 128
  typedef E8M0Scales<AL> Scales;
  static constexpr int kStage = Lines::kStage;  // uint4 per wave: [16 rows][8 slots]
  struct Lane {
    Lines::Lane c;
    typename Scales::Lane s;
  };
  struct Chunk {
    Lines::Chunk c;
    typename Scales::Bytes s;
  };
  struct Prep {
    uint4 v[2];   // v[u]: block 4 u + kq of row n, nibbles in the instruction's order
    uint32_t sc;  // byte u: the scale of block 4 u + kq
  };
  static __device__ __forceinline__ int slot(int s, int kq) { return Int8Dyn::slot(s, kq); }
  __device__ __forceinline__ Lane setup(int bn, int lane, int N, int K) const {
    Lane L;
    L.c = Lines::setup(w, (uint32_t)K >> 1, bn, lane, N);
    L.s = Scales::setup(wscale, bn, lane, N, K);
    return L;
  }
  __device__ __forceinline__ Chunk load(const Lane& L, int st) const {
    Chunk ch;
    ch.c = Lines::load(L.c, st);
    ch.s = Scales::load(L.s, st);
    return ch;
  }
  static __device__ __forceinline__ uint32_t swap_nibbles(uint32_t v) {
    return ((v << 4) & 0xF0F0F0F0u) | ((v >> 4) & 0x0F0F0F0Fu);
  }
  // (its own stage index: stage_slot()'s `& 7`, a no-op on rows below 16, compiles differently)
  __device__ __forceinline__ Prep prep(const Chunk& ch, uint4* stage, int lane) const {
    const int r = lane >> 3, c = lane & 7;
    stage[r * 8 + (c ^ (r >> 1))] = ch.c.v[0];
    stage[(r + 8) * 8 + (c ^ ((r + 8) >> 1))] = ch.c.v[1];
    const int n = lane & 15, kq = lane >> 4;
    Prep p;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint4 q = stage[n * 8 + ((4 * u + kq) ^ (n >> 1))];
      p.v[u] = make_uint4(swap_nibbles(q.x), swap_nibbles(q.y), swap_nibbles(q.z),
                          swap_nibbles(q.w));
    }
    p.sc = Scales::pack(ch.s, 8 * kq);
    return p;
  }
  // blocks 4 u + kq at or past K / 32: codes zeroed, scale byte 127
  static __device__ __forceinline__ void mask_tail(Prep& p, int st, int kq, int K) {
    const int b0 = st * kKStep + 32 * kq;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t k = b0 + 128 * u < K ? ~0u : 0u;
      p.v[u] = and16(p.v[u], k);
    }
    p.sc = Scales::mask_tail(p.sc, st, kq, K);
  }
  __device__ __forceinline__ i32x8_t frag(const Prep& p, int u) const {
    const uint4 v = u == 0 ? p.v[0] : p.v[1];
    return i32x8_t{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};  // blgp 4 reads four
  }
  // blgp 4: B e2m1
  static __device__ __forceinline__ Acc mfma2s(const uint4& a0, const uint4& a1, const i32x8_t& b,
                                               Acc c, int u, uint32_t asc, uint32_t bsc) {
    return Scales::template mfma2s<4>(a0, a1, b, c, u, asc, bsc);
  }
  __device__ __forceinline__ float epi(float acc, float, float) const { return acc; }
};

}  // namespace
}  // namespace tao
