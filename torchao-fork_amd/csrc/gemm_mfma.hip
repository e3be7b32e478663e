// Skinny GEMM on MFMA for the quantized linears at M > 4 (prefill / batched decode):
//   y[M][N] = epilogue( x[M][K] . W[N][K]^T )
// nine weight/activation formats share one kernel template (the policies: gemm_mfma_policy.h):
//   Int4WO  : bf16 x, int4 group-quant W (gfx950 row-stream layout), v_mfma_f32_16x16x32_bf16
//   Int8WO  : bf16 x, int8 per-channel W,                            v_mfma_f32_16x16x32_bf16
//   Fp8WO   : bf16 x, e4m3fn per-channel W (fp32 scales),            v_mfma_f32_16x16x32_bf16
//   Int8Dyn : int8 x (per-token scale), int8 W (per-channel scale),   v_mfma_i32_16x16x64_i8
//   Int8DynW4: int8 x (per-token fp32 scale), int4 W two per byte (per-channel fp32 scale),
//             expanded to int8 x 16 in registers,                    v_mfma_i32_16x16x64_i8
//   Fp8Dyn  : e4m3fn x (per-token scale), e4m3fn W (per-row scale),   v_mfma_scale_f32_16x16x128_f8f6f4
//   MxFp8   : e4m3fn x and W, one E8M0 scale byte per 32-k block,    v_mfma_scale_f32_16x16x128_f8f6f4
//   MxFp8Fp4: e4m3fn x, e2m1 W (two codes per byte), the same scales, the same MFMA (cbsz 0, blgp 4)
//   BlockFp8: e4m3fn x (1 x 128 fp32 scales), e4m3fn W (128 x 128 fp32 scales), the same MFMA with
//             unit scale bytes into a zero accumulator, then a scaled fp32 accumulate
// Replaces aten._weight_int4pack_mm (tensor_core_tiled_layout.py:104), mm(x, w.to(bf16)) * s
// (plain_layout.py:256-266), int_scaled_matmul + scales (plain_layout.py:294-315,
// kernel/intmm.py:108-143), F.linear(x, w.dequantize()) (floatx/float8_layout.py:391-396) and the
// row-wise torch._scaled_mm of the float8 dynamic path (floatx/float8_layout.py:329-367) and the
// block-scaled torch._scaled_mm of the MX path (prototype/mx_formats/mx_ops.py _addmm_mx_dispatch).
//
// Tile: 4 waves x 16 output columns (BN = 64) x BM rows per k-group; each wave owns 16 columns
// and all BM rows. K advances in macro-steps (256 bf16 k for int4, 128 bf16 k for int8-WO,
// 256 int8 k for int8-dyn) in which every weight load instruction reads full 128-B lines
// (8 rows x 128 B); a per-wave LDS stage regroups them into the MFMA B layout. The k order
// inside a step is permuted identically for A and B (policy slot(s, kq): the 16-B x slot
// MFMA s of lane l = (n = l & 15, kq = l >> 4) reads).
// x goes global -> registers (D-deep prefetch ring, T14) -> double-buffered, XOR-swizzled LDS
// image -> A fragments; one barrier per step. W goes straight to registers (read once per
// tile, dequantised in registers, reused for BM/16 MFMAs). K is split across k-groups inside
// the workgroup and across workgroups (split-K) so every SIMD holds several waves; the launch
// shape (BM, k-groups, slices) comes from measured sweeps (experiments/sweep_gemm.py).
// This file: gemm_mfma_kernel and its launch shape, the routing of the linear entries between
// the GEMVs, this kernel and the other GEMMs (tao_gemm.h), and the three weight-only entries.
#include <tuple>
#include <type_traits>

#include "fp8_dyn_host.h"
#include "gemm_mfma_policy.h"
#include "tao_gemm.h"

// Experiment switch: ring depth override (experiments/gemm_depth.sh; 0 = launch_one's rule).
#ifndef TAO_GEMM_DEPTH
#define TAO_GEMM_DEPTH 0
#endif

namespace tao {

namespace {

constexpr int kBN = 64;

// gemm_mfma_kernel's x image: the policy picks the row's XOR mask (P::xswz). ds_read_b128
// serves a wave in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59},
// {36-43,48-51,60-63} (MI355X_MICROARCH.md §LDS); an A-fragment read is conflict-free iff the 16
// lanes of each group hit 16 distinct 16-B granules (slot mod 16). Lane (m = l & 15, kq = l >> 4)
// reads slot(s, kq) of row m, so a group holds kq = 2i at rows A = {0-3, 12-15} and kq = 2i + 1
// at rows B = {4-11} (or the reverse). Int8Dyn's slot 4 s + kq and Int8WO's 8 (s >> 1) + 2 kq +
// (s & 1) are conflict-free with mask m; Int4WO's 16 (s >> 2) + 4 kq + (s & 3) is not (A ^ t and
// B ^ 4 ^ t are the same 8 granules: every read 2-way), so it flips bit 2 of the mask on rows B.
// The ds_write_b128 fill (8 lanes = 8 consecutive slots of one row) is conflict-free either way.
template <int SLOTS, class P>
__device__ __forceinline__ int x_slot(int row, int slot) {
  return row * SLOTS + (slot ^ P::xswz(row));
}

// One k-step ring of depth D holds both operands' loads: vector-memory loads retire in issue
// order (one vmcnt), so an x ring shallower than the weight ring would drain the weight loads
// issued before each x load anyway. The k loop is unrolled by D so every ring index is a
// compile-time constant (no scratch), and the steady-state body is straight-line code: loads
// past the last step re-read it (clamped), so hipcc counts outstanding loads (vmcnt(N))
// instead of draining them every step.
//
// Latency hiding comes from waves per SIMD, so K is split twice:
//  * inside the workgroup: KG k-groups of 4 waves (256 x KG threads) take interleaved steps
//    (k-group g: steps s0 + g, s0 + g + KG, ...), each with its own double-buffered x tile;
//    their accumulators are summed through LDS in k-group order at the end;
//  * across workgroups (gridDim.z = S slices of `sps` steps): each slice stores its raw
//    accumulator tile to a slab with sc1 (write-through) stores, and the tile's last arriver
//    (agent-scope ticket, told by the value its add returned) reads the S slabs with sc1 loads,
//    sums them in slice order and runs the epilogue. Both sums have a fixed order, so results
//    do not depend on arrival order. Protocol and its hardware assumption: last_arriver()
//    (tao_common.h); `fenced` adds the agent release/acquire fences (tao_tune_splitk_fenced).
// Experiment switch (timing A/B only): minimum waves per SIMD the register allocation must
// allow (amdgpu_waves_per_eu); 0 = the compiler's choice (the product).
#ifndef TAO_GEMM_WPE
#define TAO_GEMM_WPE 0
#endif
#if TAO_GEMM_WPE > 0
#define TAO_GEMM_WPE_ATTR __attribute__((amdgpu_waves_per_eu(TAO_GEMM_WPE)))
#else
// kBlockF32 policies read every MFMA's product back for the scaled accumulate. With up to 512
// registers per lane (256 threads) hipcc puts MFMA results into AGPRs and copies each one out with
// a v_accvgpr_read; asked to leave room for two waves per SIMD (256 registers, which these
// instances fit without scratch) it writes them to VGPRs. 0: no attribute (every other policy).
#define TAO_GEMM_WPE_ATTR __attribute__((amdgpu_waves_per_eu(P::kBlockF32 ? 2 : 0)))
#endif
template <int BM, int D, int KG, int NW, class P>
__global__ __launch_bounds__(256 * KG) TAO_GEMM_WPE_ATTR void gemm_mfma_kernel(
    const uint8_t* __restrict__ x, P pol, const uint16_t* __restrict__ bias,
    uint16_t* __restrict__ y, int M, int N, int K, int sps, typename P::Acc* __restrict__ slab,
    unsigned* __restrict__ cnt, int fenced, int order, int cs) {
  typedef typename P::Acc Acc;
  constexpr int MT = BM / 16;
  constexpr int XSB = P::kABytes * P::kKStep;  // x bytes per row per step (256 or 512)
  constexpr int SLOTS = XSB / 16;               // 16-B x slots per row per step
  constexpr int RPP = 256 / SLOTS;              // x rows loaded per 256-thread pass
  constexpr int XLOADS = BM * SLOTS / 256;      // 16-B x pieces per thread per step
  constexpr int TILE = BM * SLOTS;              // uint4 per x tile
  constexpr int NA = MT * NW;                   // accumulator tiles per wave
  static_assert((KG - 1) * 4 * NA * 64 <= KG * 2 * TILE, "k-group reduction must fit in LDS");
  // one LDS array (a second __shared__ object can de-pipeline the loop, cdna guide §5 item 4a):
  // [KG][2][x tile] then the per-wave weight stages (NW per wave), then (block-scaled policies)
  // [KG][2][BM rows][8 scale bytes] of the x tiles ([KG][2][2 blocks][BM rows] floats: kBlockF32)
  constexpr bool kBS = P::kBlockScaled;
  constexpr bool kBSA = P::kScaleAligned;  // whole 8-B words of scale bytes per row and step
  constexpr int XSL = kBSA ? 2 : kBS ? (BM + 31) / 32 : 1;  // x scale registers per thread per step
  constexpr bool kBF = P::kBlockF32;  // fp32 x scales per 128-k block: BM x 2 floats per step
  constexpr int XSC = (kBS || kBF) ? BM / 2 : 0;  // uint4 per tile of x scale bytes / floats
  __shared__ uint4 lds[KG * 2 * TILE + KG * 4 * NW * P::kStage + (P::kStage == 0) + KG * 2 * XSC];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int kg = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int wave = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int ktid = tid & 255;
  const TileId tid3 = xcd_tile(order);
  const int n_blk = tid3.n * kBN * NW;
  const int m_blk = tid3.m * BM;
  const int nsteps = (K + P::kKStep - 1) / P::kKStep;
  const int s0 = tid3.z * sps;
  const int s1 = s0 + sps < nsteps ? s0 + sps : nsteps;  // launcher: no empty slice
  const int J = (s1 - s0 + KG - 1) / KG;                 // steps per k-group (all k-groups)
  const int row_bytes = K * P::kABytes;
  uint4* xs = lds + kg * 2 * TILE;

  // the wave's NW 16-column blocks: columns n_blk + 16 (NW wave + c) + (lane & 15)
  int bn[NW];
  typename P::Lane wl[NW];
#pragma unroll
  for (int c = 0; c < NW; ++c) {
    bn[c] = n_blk + (wave * NW + c) * 16 + (lane & 15);
    wl[c] = pol.setup(bn[c], lane, N, K);
  }
  const int kq = lane >> 4;
  uint4* wstage = lds + KG * 2 * TILE + (kg * 4 + wave) * NW * P::kStage;

  // this thread's x pieces: rows row0 + RPP i (i < XLOADS), 16-B slot xslot of each; rows
  // past M are clamped to M - 1 (computed and dropped). A k tail past the row end reads the
  // next row (or 0 past the buffer) and is masked at the LDS store.
  const int row0 = ktid / SLOTS, xslot = ktid % SLOTS;
  const int xslot_b = xslot * 16;
  const Rsrc xrs = make_rsrc(x, (uint32_t)M * (uint32_t)row_bytes);
  uint32_t xv[XLOADS];
  int xlds[XLOADS];
#pragma unroll
  for (int i = 0; i < XLOADS; ++i) {
    const int gm = m_blk + row0 + RPP * i;
    xv[i] = (uint32_t)(gm < M ? gm : M - 1) * (uint32_t)row_bytes + xslot_b;
    xlds[i] = x_slot<SLOTS, P>(row0 + RPP * i, xslot);
  }
  const bool ragged = (row_bytes % XSB) != 0;
  // block-scaled: this thread's x scale bytes, block ktid & 7 of rows (ktid >> 3) + 32 i
  const int nblk = K >> 5;
  const int xsblk = ktid & 7;
  const uint8_t* xsrow[XSL];
  uint8_t* xscl = reinterpret_cast<uint8_t*>(lds + KG * 2 * TILE + KG * 4 * NW * P::kStage +
                                             (P::kStage == 0) + kg * 2 * XSC);
  if constexpr (kBSA) {  // thread t: the step's 8 bytes of row t (t >= BM: row BM - 1, not stored)
    const int gm = m_blk + (ktid < BM ? ktid : BM - 1);
    xsrow[0] = pol.xscale + (size_t)(gm < M ? gm : M - 1) * nblk;
  } else if constexpr (kBS) {
#pragma unroll
    for (int i = 0; i < XSL; ++i) {
      const int gm = m_blk + (ktid >> 3) + 32 * i;
      xsrow[i] = pol.xscale + (size_t)(gm < M ? gm : M - 1) * nblk;
    }
  }

  // kBlockF32: this thread's x scale, block ktid & 1 of row ktid >> 1 (rows past BM: row BM - 1,
  // not stored)
  const int nblk128 = K >> 7;
  const float* xfrow = nullptr;
  if constexpr (kBF) {
    const int r = ktid >> 1;
    const int gm = m_blk + (r < BM ? r : BM - 1);
    xfrow = pol.xscale + (size_t)(gm < M ? gm : M - 1) * nblk128;
  }

  Acc acc[NA];  // [t][c]
#pragma unroll
  for (int t = 0; t < NA; ++t) acc[t] = Acc{0, 0, 0, 0};

  uint4 xr[D][XLOADS];
  typename P::Chunk wr[D][NW];
  uint32_t xsr[D][XSL];

  // local step j of this k-group -> absolute step (may be >= s1: then inactive)
  auto abs_step = [&](int j) __attribute__((always_inline)) { return s0 + kg + j * KG; };
  auto load_step = [&](int j, uint4 (&xdst)[XLOADS], typename P::Chunk (&wdst)[NW],
                       uint32_t (&sdst)[XSL]) __attribute__((always_inline)) {
    const int st0 = abs_step(j);
    const int st = st0 < s1 ? st0 : s1 - 1;
#pragma unroll
    for (int i = 0; i < XLOADS; ++i) xdst[i] = bload16(xrs, xv[i], st * XSB);
    if constexpr (kBSA) {
      const uint2 v = *reinterpret_cast<const uint2*>(xsrow[0] + st * 8);
      sdst[0] = v.x;
      sdst[1] = v.y;
    } else if constexpr (kBS) {
      const int b = st * 8 + xsblk;
      const int bc = b < nblk ? b : nblk - 1;  // never past the row's K / 32 bytes
#pragma unroll
      for (int i = 0; i < XSL; ++i) sdst[i] = xsrow[i][bc];
    } else if constexpr (kBF) {
      const int b = st * 2 + (ktid & 1);
      sdst[0] = __float_as_uint(xfrow[b < nblk128 ? b : nblk128 - 1]);  // never past K / 128
    }
#pragma unroll
    for (int c = 0; c < NW; ++c) wdst[c] = pol.load(wl[c], st);
  };
  auto store_x = [&](const uint4 (&src)[XLOADS], int j) __attribute__((always_inline)) {
    const int st = abs_step(j);
    uint4* dst = xs + (j & 1) * TILE;
    if constexpr (P::kXPerm) {
      // (Int8DynW4) each piece's bytes in the B fragment's k order; the tail mask as below
      const uint32_t keep = st < s1 && st * XSB + xslot_b < row_bytes ? ~0u : 0u;
#pragma unroll
      for (int i = 0; i < XLOADS; ++i) dst[xlds[i]] = and16(P::xperm(src[i]), keep);
    } else if (!ragged && st < s1) {
#pragma unroll
      for (int i = 0; i < XLOADS; ++i) dst[xlds[i]] = src[i];
    } else {
      // k tail / inactive step -> 0 (an AND mask: a select here compiles to a branch)
      const uint32_t keep = st < s1 && st * XSB + xslot_b < row_bytes ? ~0u : 0u;
#pragma unroll
      for (int i = 0; i < XLOADS; ++i) dst[xlds[i]] = and16(src[i], keep);
    }
  };
  // block-scaled: the step's x scale bytes beside the image, [row][kq][u] for block 4 u + kq; a
  // block past K / 32 (or an inactive step) gets 127 = 2^0 against its zeroed codes
  auto store_xs = [&](const uint32_t (&src)[XSL], int j) __attribute__((always_inline)) {
    if constexpr (kBSA) {
      // bytes b0 .. b7 -> (b0 b4 b1 b5) (b2 b6 b3 b7); no K tail here, and an inactive step's
      // bytes are never read
      if (ktid < BM) {
        uint8_t* dst = xscl + (j & 1) * (BM * 8);
        *reinterpret_cast<uint2*>(dst + ktid * 8) =
            make_uint2(__builtin_amdgcn_perm(src[1], src[0], 0x05010400u),
                       __builtin_amdgcn_perm(src[1], src[0], 0x07030602u));
      }
    } else if constexpr (kBS) {
      const int st = abs_step(j);
      const bool in = st < s1 && st * 8 + xsblk < nblk;
      uint8_t* dst = xscl + (j & 1) * (BM * 8);
#pragma unroll
      for (int i = 0; i < XSL; ++i) {
        const int row = (ktid >> 3) + 32 * i;
        if (row < BM)
          dst[row * 8 + (xsblk & 3) * 2 + (xsblk >> 2)] = (uint8_t)(in ? src[i] : 127u);
      }
    } else if constexpr (kBF) {
      // [block][row]; a block past K / 128 (or an inactive step) gets 0 against its zeroed codes
      const int st = abs_step(j);
      const bool in = st < s1 && st * 2 + (ktid & 1) < nblk128;
      uint32_t* dst = reinterpret_cast<uint32_t*>(xscl + (j & 1) * (BM * 8));
      if ((ktid >> 1) < BM) dst[(ktid & 1) * BM + (ktid >> 1)] = in ? src[0] : 0u;
    }
  };
  // local step j; u = j % D at compile time
  auto body = [&](auto uc, int j) __attribute__((always_inline)) {
    constexpr int u = decltype(uc)::value;
    load_step(j + D - 1, xr[(u + D - 1) % D], wr[(u + D - 1) % D], xsr[(u + D - 1) % D]);
    if (abs_step(j) < s1) {  // uniform: a k-group's idle tail iterations skip the math
      typename P::Prep pw[NW];
#pragma unroll
      for (int c = 0; c < NW; ++c) {
        pw[c] = pol.prep(wr[u][c], wstage + c * P::kStage, lane);
        if constexpr (P::kMaskTail) P::mask_tail(pw[c], abs_step(j), kq, K);
      }
      const uint4* xb = xs + (j & 1) * TILE;
      // block-scaled: the step's two scale bytes of this lane's row of each M tile (byte u: MFMA u)
      uint32_t asc[kBS ? MT : 1];
      if constexpr (kBS) {
#pragma unroll
        for (int t = 0; t < MT; ++t)
          asc[t] = reinterpret_cast<const uint16_t*>(
              xscl + (j & 1) * (BM * 8))[(t * 16 + (lane & 15)) * 4 + kq];
      }
#pragma unroll
      for (int s = 0; s < P::kMfma; ++s) {
        decltype(pol.frag(pw[0], s)) bfrag[NW];
#pragma unroll
        for (int c = 0; c < NW; ++c) bfrag[c] = pol.frag(pw[c], s);
        if constexpr (P::kASlots == 2) {
          // a 32-B A fragment: the two 16-B slots that hold the k of B fragment s
          const int slot0 = P::slot(2 * s, kq), slot1 = P::slot(2 * s + 1, kq);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            const int row = t * 16 + (lane & 15);
            const uint4 a0 = xb[x_slot<SLOTS, P>(row, slot0)];
            const uint4 a1 = xb[x_slot<SLOTS, P>(row, slot1)];
            if constexpr (kBS) {
#pragma unroll
              for (int c = 0; c < NW; ++c)
                acc[t * NW + c] =
                    P::mfma2s(a0, a1, bfrag[c], acc[t * NW + c], s, asc[t], pw[c].sc);
            } else if constexpr (kBF) {
              // block s of the step: the scales of this lane's C rows 4 kq .. 4 kq + 3 of tile t
              const float4 xf = reinterpret_cast<const float4*>(
                  xscl + (j & 1) * (BM * 8))[(s * BM + t * 16) / 4 + kq];
#pragma unroll
              for (int c = 0; c < NW; ++c)
                acc[t * NW + c] =
                    P::scaled_acc(P::mfma2(a0, a1, bfrag[c], Acc{0, 0, 0, 0}), xf, pw[c], s,
                                  acc[t * NW + c]);
            } else {
#pragma unroll
              for (int c = 0; c < NW; ++c)
                acc[t * NW + c] = P::mfma2(a0, a1, bfrag[c], acc[t * NW + c]);
            }
          }
        } else {
          const int slot = P::slot(s, kq);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            const int row = t * 16 + (lane & 15);
            // one A fragment read from LDS feeds the wave's NW column blocks
            const uint4 a = xb[x_slot<SLOTS, P>(row, slot)];
#pragma unroll
            for (int c = 0; c < NW; ++c) acc[t * NW + c] = P::mfma(a, bfrag[c], acc[t * NW + c]);
          }
        }
      }
    }
    if (j + 1 < J) {
      store_x(xr[(u + 1) % D], j + 1);
      store_xs(xsr[(u + 1) % D], j + 1);
    }
    __syncthreads();
  };

  // Epilogue operands loaded now, ahead of the weights: loaded in the epilogue, their round
  // trip sat in every workgroup's tail (~1 µs of the int8-dyn M = 128 4096² kernel;
  // experiments/gemm_stamps.py). Per lane: the row factor of its 4 rows per M tile (rows
  // clamped to M - 1, kept as bf16 pairs), the column factor and bias of its NW columns.
  // (the int4 policy has neither factor; its bias stays an epilogue load: prefetching that too
  // measured 1.3 µs slower at M = 128, 4096², profiles/r2_ab_epi.txt)
  constexpr bool kPre = P::kRowF || P::kColF;
  // (an fp32 row factor, Fp8Dyn's, is kept as floats)
  constexpr bool kRowF32 =
      P::kRowF && std::is_same_v<decltype(pol.row_factor()), const float*>;
  uint2 rowf[P::kRowF ? MT : 1];
  float rowff[kRowF32 ? MT * 4 : 1];
  float colf[NW], biasf[NW];
  if constexpr (kRowF32) {
    const float* rp = pol.row_factor();
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m_blk + t * 16 + 4 * (lane >> 4) + i;
        rowff[t * 4 + i] = rp[m < M ? m : M - 1];
      }
    }
  } else if constexpr (P::kRowF) {
    const uint16_t* rp = pol.row_factor();
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      uint32_t h[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m_blk + t * 16 + 4 * (lane >> 4) + i;
        h[i] = rp[m < M ? m : M - 1];
      }
      rowf[t] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    }
  }
#pragma unroll
  for (int c = 0; c < NW; ++c) {
    const int nn = bn[c] < N ? bn[c] : N - 1;
    if constexpr (!P::kColF)
      colf[c] = 1.f;
    else if constexpr (std::is_same_v<decltype(pol.col_factor()), const float*>)
      colf[c] = pol.col_factor()[nn];  // fp32 factors (Fp8WO)
    else
      colf[c] = bf16_to_f32(pol.col_factor()[nn]);
    biasf[c] = (kPre && bias != nullptr) ? bf16_to_f32(bias[nn]) : 0.f;
  }
  static_for<0, D - 1>([&](auto i) __attribute__((always_inline)) {
    load_step(decltype(i)::value, xr[decltype(i)::value], wr[decltype(i)::value],
              xsr[decltype(i)::value]);
  });
  store_x(xr[0], 0);
  store_xs(xsr[0], 0);
  __syncthreads();

  int j = 0;
  for (; j + D <= J; j += D)
    static_for<0, D>([&](auto uc) __attribute__((always_inline)) {
      body(uc, j + decltype(uc)::value);
    });
  static_for<0, D - 1>([&](auto uc) __attribute__((always_inline)) {
    if (j + decltype(uc)::value < J) body(uc, j + decltype(uc)::value);
  });

  // k-groups 1..KG-1 hand their accumulators to k-group 0 through LDS (summed in order)
  if constexpr (KG > 1) {
    Acc* red = reinterpret_cast<Acc*>(lds);
    if (kg > 0) {
#pragma unroll
      for (int t = 0; t < NA; ++t) red[(((kg - 1) * 4 + wave) * NA + t) * 64 + lane] = acc[t];
    }
    __syncthreads();
    if (kg == 0) {
      for (int g = 1; g < KG; ++g) {
#pragma unroll
        for (int t = 0; t < NA; ++t) acc[t] += red[(((g - 1) * 4 + wave) * NA + t) * 64 + lane];
      }
    }
    __syncthreads();  // LDS free again (the split-K flag below reuses it)
  }

  const int S = gridDim.z;
  if (S > 1) {
    // Slab hand-off (last_arriver, tao_common.h: MI355X_MICROARCH.md "Hand-offs measured with
    // sc1 loads in place of the acquire", first row): every slab byte is stored sc1 (write-through
    // past the XCD's L2) and read sc1 (L1 bypassed), each storing wave waits for its stores
    // before the workgroup barrier, one lane adds the tile's ticket, and the last arriver is told
    // by the value its add returned. The fences this leaves out by default (buffer_wbl2 +
    // buffer_inv, 1.7-6.5 µs each and serialised per CU) made every split slower than no split;
    // `fenced` puts them back (tao_tune_splitk_fenced).
    const unsigned tile = tid3.m * gridDim.x + tid3.n;
    const size_t tile_bytes = (size_t)S * 4 * NA * 64 * sizeof(Acc);
    const Rsrc srs = make_rsrc(reinterpret_cast<const uint8_t*>(slab) + tile * tile_bytes,
                               (uint32_t)tile_bytes);
    const uint32_t lane_off = (uint32_t)((wave * NA * 64 + lane) * sizeof(Acc));
    constexpr uint32_t kZ = 4 * NA * 64 * sizeof(Acc);  // one slice's slab
    if (kg == 0) {
#pragma unroll
      for (int t = 0; t < NA; ++t)
        bstore16<kSC1>(srs, lane_off + t * 64 * sizeof(Acc), tid3.z * kZ,
                       __builtin_bit_cast(uint4, acc[t]));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool last =
        last_arriver(&cnt[tile * cs], (unsigned)S, reinterpret_cast<unsigned*>(lds), fenced);
    if (!last || kg != 0) {
      return;
    }
#pragma unroll
    for (int t = 0; t < NA; ++t) acc[t] = Acc{0, 0, 0, 0};
    // 4 slabs per round, all loads issued before the first add (clamped, then masked); slices
    // summed in slice order whatever the arrival order
    for (int z0 = 0; z0 < S; z0 += 4) {
      Acc part[4][NA];
#pragma unroll
      for (int zz = 0; zz < 4; ++zz) {
        const int z = z0 + zz < S ? z0 + zz : S - 1;
#pragma unroll
        for (int t = 0; t < NA; ++t)
          part[zz][t] = __builtin_bit_cast(
              Acc, bload16<kSC1>(srs, lane_off + t * 64 * sizeof(Acc), z * kZ));
      }
#pragma unroll
      for (int zz = 0; zz < 4; ++zz) {
        if (z0 + zz < S) {
#pragma unroll
          for (int t = 0; t < NA; ++t) acc[t] += part[zz][t];
        }
      }
    }
  } else if (kg != 0) {
    return;
  }

  // C/D map: col = lane & 15 (n), row = 4*(lane >> 4) + i (m).
#pragma unroll
  for (int c = 0; c < NW; ++c) {
    if (bn[c] < N) {
      if constexpr (!kPre) biasf[c] = bias != nullptr ? bf16_to_f32(bias[bn[c]]) : 0.f;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = m_blk + t * 16 + 4 * (lane >> 4) + i;
          if (m < M) {
            float rf = 1.f;
            if constexpr (kRowF32) {
              rf = rowff[t * 4 + i];
            } else if constexpr (P::kRowF) {
              const uint32_t w = (i < 2) ? rowf[t].x : rowf[t].y;
              rf = (i & 1) ? bf16hi_to_f32(w) : bf16lo_to_f32(w);
            }
            float v = pol.epi(acc[t * NW + c][i], rf, colf[c]);
            if (bias != nullptr) v = round_bf16(v + biasf[c]);
            y[(size_t)m * N + bn[c]] = f32_to_bf16(v);
          }
        }
      }
    }
  }
}

// Launch shape: M tile, k-groups per workgroup and K slices. Per-workgroup time is set by its
// load latency chain, so the grid should put several waves on every SIMD.
struct GemmShape {
  int bm, kg, splits, nw;
};

GemmShape choose_shape(int M, int N, int nsteps, int max_bm, int xsb, int pref_kg,
                       int min_slice, int nw) {
  // From the sweeps with the fence-free split-K hand-off (experiments/sweep_gemm.py,
  // profiles/r1_sweep_gemm_sc1*.jsonl; the fenced hand-off made every split lose):
  //  * short K (<= 16 steps): the largest M tile (no 2x padding of M) that gives ~one round of
  //    workgroups (>= 224 tiles of 256 CUs) unsplit; 128 gives way to 64 while that still fits
  //    in two rounds (<= 512 tiles);
  //  * otherwise the M tile that covers M up to 64 rows, and K split until the distinct weight
  //    slices (N tiles x K slices) reach one round, <= 512 workgroups, slices >= min_slice
  //    steps (1024 k);
  //  * the policy's preferred k-groups (int4 / int8-WO 2, int8-dyn 1).
  const long nb = (N + kBN * nw - 1) / (kBN * nw);
  auto tiles_of = [&](int bm) { return nb * ((M + bm - 1) / bm); };
  GemmShape sh{16, pref_kg, 1, nw};
  const int cands[4] = {128, 64, 32, 16};
  bool found = false;
  if (nsteps <= 16) {
    for (int bm : cands)
      if (bm <= max_bm && (bm < 2 * M || bm == 16) && tiles_of(bm) >= 224) {
        sh.bm = bm;
        found = true;
        break;
      }
    if (found && sh.bm == 128 && tiles_of(64) <= 512) sh.bm = 64;
  }
  if (!found) {
    const int cap = max_bm < 64 ? max_bm : 64;
    while (sh.bm < cap && sh.bm < M) sh.bm *= 2;
    const long tiles = tiles_of(sh.bm);
    while (nb * sh.splits < 224 && tiles * sh.splits * 2 <= 512 && sh.splits * 2 <= 8 &&
           nsteps >= min_slice * sh.splits * 2)
      sh.splits *= 2;
  }
  // int8-dyn (one k-group by default): two when the launch is unsplit and >= 4 M tiles re-read
  // each weight tile (M = 128, 4096^2: 11.4 vs 11.9 µs; profiles/r1_sweep_gemm_sc1*.jsonl)
  if (pref_kg == 1 && sh.splits == 1 && (M + sh.bm - 1) / sh.bm >= 4) sh.kg = 2;
  const int tb = tao::tuning().bm;
  const int tk = tao::tuning().kg;
  const int ts = tao::tuning().splits;
  if (tb) sh.bm = tb < max_bm ? tb : max_bm;
  if (tk) sh.kg = tk;
  if (ts) sh.splits = ts < nsteps ? ts : nsteps;
  // LDS: KG x 2 x BM x xsb (double-buffered x tiles) <= 64 KiB
  while (sh.kg > 1 && sh.kg * sh.bm * xsb > 32768) sh.kg >>= 1;
  return sh;
}

// Measured launch shapes for the Llama-3 8B / 70B linears (experiments/sweep_nw.py ->
// experiments/gen_gemm_table.py; profiles/r2_sweep_nw_wide*.jsonl): where a swept shape beat
// choose_shape (and, for int8-dyn, the LDS-kernel choice) by >= 7% on the box. M is bucketed up
// to 16 / 32 / ... / 512; other shapes and M > 512 keep the heuristic. Any shape is correct and
// deterministic; a table shape only changes speed (and, through kg / splits, the fixed fp32
// summation order). nw 32 (int4 only) names gemm32_int4_kernel with that (bm, splits).
struct TunedShape {
  int path, m, n, k, bm, kg, splits, nw;
};
constexpr TunedShape kTuned[] = {
#include "gemm_table.inc"
};

const TunedShape* tuned_shape(int path, int M, int N, int K) {
  if (tuning().gemm_table == 1 || tuning().bm || tuning().kg || tuning().splits ||
      tuning().gemm_nw || M > 512)
    return nullptr;
  int mb = 16;
  while (mb < M) mb *= 2;
  for (const TunedShape& t : kTuned)
    if (t.path == path && t.m == mb && t.n == N && t.k == K) return &t;
  return nullptr;
}

template <int BM, int KG, int NW, class P>
void launch_one(dim3 grid, hipStream_t stream, const uint8_t* xb, const P& pol,
                const uint16_t* bias, uint16_t* y, int M, int N, int K, int sps,
                typename P::Acc* slab, unsigned* cnt) {
  if constexpr (BM <= P::kMaxBM && KG <= P::kMaxKG) {
    // ring depth: 4 steps, 3 where the per-stage registers grow (int8-dyn's 64-B pieces,
    // int4's 512-B x rows), 2 at BM >= 64
    constexpr bool big = sizeof(typename P::Chunk) > 32 || P::kABytes * P::kKStep > 256;
    constexpr int D = TAO_GEMM_DEPTH > 0 ? TAO_GEMM_DEPTH
                                         : (BM <= 16 ? 4 : (BM <= 32 ? (big ? 3 : 4) : 2));
    launch((gemm_mfma_kernel<BM, D, KG, NW, P>), grid, dim3(256 * KG), 0, stream, xb, pol, bias, y,
           M, N, K, sps, slab, cnt, tuning().splitk_fenced, tuning().gemm_order,
           tuning().cnt_stride);
  }
}

template <class P>
int launch_gemm(const void* x, const P& pol, const uint16_t* bias, uint16_t* y, int M, int N,
                int K, hipStream_t stream) {
  const int nsteps = (K + P::kKStep - 1) / P::kKStep;
  const int nw = tuning().gemm_nw == 2 ? 2 : 1;
  GemmShape sh;
  if (const TunedShape* t = tuned_shape(P::kPathId, M, N, K)) {
    sh = GemmShape{t->bm < P::kMaxBM ? t->bm : P::kMaxBM, t->kg,
                   t->splits < nsteps ? t->splits : nsteps, t->nw};
    // as choose_shape's overrides were applied when the table was measured
    while (sh.kg > 1 && sh.kg * sh.bm * P::kABytes * P::kKStep > 32768) sh.kg >>= 1;
  } else {
    sh = choose_shape(M, N, nsteps, P::kMaxBM, P::kABytes * P::kKStep, P::kPrefKG, P::kMinSlice,
                      nw);
  }
  if (sh.nw == 32) sh.nw = 1;  // (the 32x32x16 kernel's entries are dispatched before this)
  if (sh.kg > P::kMaxKG) sh.kg = P::kMaxKG;
  if (sh.nw == 2) {  // instantiated: BM <= 64, KG <= 2 (registers)
    if (sh.bm > 64) sh.bm = 64;
    if (sh.kg > 2) sh.kg = 2;
  }
  const int sps = (nsteps + sh.splits - 1) / sh.splits;
  const int S = (nsteps + sps - 1) / sps;  // no empty slice
  const int bnw = kBN * sh.nw;
  dim3 grid((N + bnw - 1) / bnw, (M + sh.bm - 1) / sh.bm, S);
  typename P::Acc* slab = nullptr;
  unsigned* cnt = nullptr;
  if (S > 1) {
    const size_t tiles = (size_t)grid.x * grid.y;
    void* ws = nullptr;
    const int rc = split_workspace(stream, tiles * S * sh.bm * bnw * sizeof(float),
                                   tiles * tuning().cnt_stride, &ws, &cnt);
    if (rc != TAO_OK) return rc;
    slab = reinterpret_cast<typename P::Acc*>(ws);
  }
  const uint8_t* xb = reinterpret_cast<const uint8_t*>(x);
  const auto args = std::make_tuple(grid, stream, xb, pol, bias, y, M, N, K, sps, slab, cnt);
  auto go = [&](auto fn) { std::apply(fn, args); };
  if (sh.nw == 2) {  // 32 columns per wave: each A fragment read feeds two MFMAs
    switch (sh.bm * 8 + sh.kg) {
      case 16 * 8 + 1: go(launch_one<16, 1, 2, P>); break;
      case 16 * 8 + 2: go(launch_one<16, 2, 2, P>); break;
      case 32 * 8 + 1: go(launch_one<32, 1, 2, P>); break;
      case 32 * 8 + 2: go(launch_one<32, 2, 2, P>); break;
      case 64 * 8 + 1: go(launch_one<64, 1, 2, P>); break;
      default: go(launch_one<64, 2, 2, P>); break;
    }
    return check_launch("gemm_mfma_kernel");
  }
  switch (sh.bm * 8 + sh.kg) {
    case 16 * 8 + 1: go(launch_one<16, 1, 1, P>); break;
    case 16 * 8 + 2: go(launch_one<16, 2, 1, P>); break;
    case 16 * 8 + 4: go(launch_one<16, 4, 1, P>); break;
    case 32 * 8 + 1: go(launch_one<32, 1, 1, P>); break;
    case 32 * 8 + 2: go(launch_one<32, 2, 1, P>); break;
    case 32 * 8 + 4: go(launch_one<32, 4, 1, P>); break;
    case 64 * 8 + 1: go(launch_one<64, 1, 1, P>); break;
    case 64 * 8 + 2: go(launch_one<64, 2, 1, P>); break;
    default: go(launch_one<128, 1, 1, P>); break;
  }
  return check_launch("gemm_mfma_kernel");
}

// Largest M served by the GEMV kernels (tao_tune_linear_crossover; 0 = built-in).
// Built-in crossover (experiments/bench_paths.py --crossover): the GEMV wins at M <= 2, and at
// M <= 4 for small weights; the MFMA kernel's per-M cost is nearly flat.
bool use_gemv(int64_t M, int64_t N, int64_t K) {
  const int v = tao::tuning().max_gemv_m;
  if (v > 0) return M <= v;
  return M <= 2 || (M <= 4 && N * K <= (32LL << 20));
}

int gshift_of(int64_t g) {
  switch (g) {
    case 32: return 0;
    case 64: return 1;
    case 128: return 2;
    case 256: return 3;
    default: return -1;
  }
}

}  // namespace

// the skinny-M crossover, for the single-fetch partials entry (gemm_sf.hip), which serves only
// shapes the plain linear runs on the single-fetch kernel
bool int4_linear_takes_gemv(int64_t M, int64_t N, int64_t K) { return use_gemv(M, N, K); }

// the float8 dynamic-activation route's crossover (rule and measurements: fp8_dyn_host.h)
bool fp8dyn_takes_gemv(int64_t M, int64_t N, int64_t K) {
  return fp8dyn_route_gemv(M, N, K, tuning().fp8dyn_mfma, tuning().max_gemv_m);
}

int fp8_scaled_mm_launch(const uint8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                         const uint16_t* bias, uint16_t* y, int M, int N, int K,
                         hipStream_t stream) {
  Fp8Dyn pol;
  pol.w = reinterpret_cast<const uint4*>(wq);
  pol.wscale = ws;
  pol.xscale = xs;
  return launch_gemm(xq, pol, bias, y, M, N, K, stream);
}

// the MX route's crossover: the float8 dynamic-activation rule (same GEMV decomposition, same MFMA
// tile), with its own force switch (tao_tune_mx_mfma)
bool mx_takes_gemv(int64_t M, int64_t N, int64_t K) {
  return fp8dyn_route_gemv(M, N, K, tuning().mx_mfma, tuning().max_gemv_m);
}

template <class P>
int launch_mx(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq, const uint8_t* ws,
              const uint16_t* bias, uint16_t* y, int M, int N, int K, hipStream_t stream) {
  P pol;
  pol.w = reinterpret_cast<const uint4*>(wq);
  pol.wscale = ws;
  pol.xscale = xs;
  return launch_gemm(xq, pol, bias, y, M, N, K, stream);
}

int mx_scaled_mm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq, const uint8_t* ws,
                        const uint16_t* bias, uint16_t* y, int M, int N, int K,
                        hipStream_t stream) {
  if (K % 256 == 0)  // (the entry has checked the scale arrays' 8-B alignment)
    return launch_mx<MxFp8<true>>(xq, xs, wq, ws, bias, y, M, N, K, stream);
  return launch_mx<MxFp8<false>>(xq, xs, wq, ws, bias, y, M, N, K, stream);
}

// MXFP4 weights (mx_fp4.hip): the same route rule (mx_takes_gemv) and the same split by K % 256
int mxfp4w_scaled_mm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq,
                            const uint8_t* ws, const uint16_t* bias, uint16_t* y, int M, int N,
                            int K, hipStream_t stream) {
  if (K % 256 == 0)
    return launch_mx<MxFp8Fp4<true>>(xq, xs, wq, ws, bias, y, M, N, K, stream);
  return launch_mx<MxFp8Fp4<false>>(xq, xs, wq, ws, bias, y, M, N, K, stream);
}

// the blockwise float8 route (block_fp8.hip): the same rule again, its force switch
// tao_tune_blockfp8_mfma
bool blockfp8_takes_gemv(int64_t M, int64_t N, int64_t K) {
  return fp8dyn_route_gemv(M, N, K, tuning().blockfp8_mfma, tuning().max_gemv_m);
}

int blockfp8_scaled_mm_launch(const uint8_t* xq, const float* xs, const uint8_t* wq,
                              const float* ws, const uint16_t* bias, uint16_t* y, int M, int N,
                              int K, hipStream_t stream) {
  BlockFp8 pol;
  pol.w = reinterpret_cast<const uint4*>(wq);
  pol.wscale = ws;
  pol.xscale = xs;
  return launch_gemm(xq, pol, bias, y, M, N, K, stream);
}

// W4A8 (w4a8.hip): every M above the GEMV's goes to the Int8DynW4 instance
int w4a8_scaled_mm_launch(const int8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                          const uint16_t* bias, uint16_t* y, int M, int N, int K,
                          hipStream_t stream) {
  Int8DynW4 pol;
  pol.w = reinterpret_cast<const uint4*>(wq);
  pol.wscale = ws;
  pol.xscale = xs;
  return launch_gemm(xq, pol, bias, y, M, N, K, stream);
}

int int8_scaled_mm_launch(const int8_t* xq, const uint16_t* xs, const int8_t* wq,
                          const uint16_t* ws, const uint16_t* bias, uint16_t* y, int M, int N,
                          int K, hipStream_t stream) {
  // The LDS-staged kernel where its unsplit 64-row tiles fill >= 192 workgroups (M >= 128):
  // M = 128 N = 6144 14.9 vs 20.0 µs, M = 256 4096^2 14.8 vs 16.5, M = 512 22.5 vs 30.8; ties at
  // N >= 14336; the per-wave-column kernel keeps M = 64..128 at N = 4096 (11.8 vs 12.6 µs).
  if (use_sf(2, M, N, K, 0)) return sf_int8dyn(xq, xs, wq, ws, bias, y, M, N, K, stream);
  if (use_tile(2, M, N, K))
    return tile_int8dyn(xq, xs, wq, ws, bias, y, M, N, K, stream, tuning().tile_splits);
  const int algo = tao::tuning().gemm_algo;
  const long t64 = (long)((N + 63) / 64) * ((M + 63) / 64);
  const bool tuned = algo == 0 && tuned_shape(Int8Dyn::kPathId, M, N, K) != nullptr;
  if (K % kI8Step == 0 && !tuned && (algo == 2 || (algo == 0 && M >= 128 && t64 >= 192)))
    return launch_i8_lds(xq, xs, wq, ws, bias, y, M, N, K, algo == 0, stream);
  Int8Dyn pol;
  pol.w = reinterpret_cast<const uint4*>(wq);
  pol.wscale = ws;
  pol.xscale = xs;
  return launch_gemm(xq, pol, bias, y, M, N, K, stream);
}

}  // namespace tao

extern "C" int tao_int4wo_linear_bf16(const uint16_t* x, const uint32_t* packed,
                                      const uint16_t* sz, const uint16_t* bias, uint16_t* y,
                                      int64_t M, int64_t N, int64_t K, int64_t group_size,
                                      void* stream) {
  int rc = tao::int4_check_linear_args(x, packed, sz, y, M, N, K, group_size);
  if (rc != TAO_OK) return rc;
  if (M == 0 || N == 0) return TAO_OK;
  hipStream_t st = tao::as_stream(stream);
  if (tao::use_gemv(M, N, K))
    return tao::int4wo_gemv(x, packed, sz, bias, y, M, N, K, group_size, st);
  if (tao::use_sf(0, M, N, K, group_size))
    return tao::sf_int4(x, packed, sz, tao::gshift_of(group_size) + 5, bias, y, (int)M, (int)N,
                        (int)K, st);
  if (tao::use_tile(0, M, N, K))
    return tao::tile_int4(x, packed, sz, tao::gshift_of(group_size), bias, y, (int)M, (int)N,
                          (int)K, st, tao::tuning().tile_splits);
  if (tao::tuning().int4_mfma32 == 1)  // 32x32x16 MFMA kernel (tao_tune_int4_mfma32)
    return tao::launch_gemm32_int4(x, packed, sz, tao::gshift_of(group_size), bias, y, (int)M,
                                   (int)N, (int)K, st);
  // measured table entries with nw 32 name the 32x32x16 kernel and its (bm, splits)
  if (const tao::TunedShape* t = tao::tuned_shape(tao::Int4WO::kPathId, (int)M, (int)N, (int)K))
    if (t->nw == 32)
      return tao::launch_gemm32_int4(x, packed, sz, tao::gshift_of(group_size), bias, y, (int)M,
                                     (int)N, (int)K, st, t->bm, t->splits);
  tao::Int4WO pol;
  pol.wq = reinterpret_cast<const uint4*>(packed);
  pol.sz = reinterpret_cast<const uint32_t*>(sz);
  pol.gshift = tao::gshift_of(group_size);
  return tao::launch_gemm(x, pol, bias, y, (int)M, (int)N, (int)K, st);
}

extern "C" int tao_int8wo_linear_bf16(const uint16_t* x, const int8_t* w, const uint16_t* scale,
                                      const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                                      int64_t K, void* stream) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "int8 weight-only linear: negative size");
  TAO_CHECK_ARG(K % 32 == 0, "int8 weight-only linear: K (%lld) must be a multiple of 32",
                (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31) && K < (1LL << 31) && M < (1LL << 31),
                "int8 weight-only linear: size out of range");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "int8 weight-only linear: K must be > 0");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(scale, 2, "scale");
  hipStream_t st = tao::as_stream(stream);
  if (tao::use_gemv(M, N, K)) return tao::int8wo_gemv(x, w, scale, bias, y, M, N, K, st);
  if (tao::use_tile(1, M, N, K))
    return tao::tile_int8wo(x, w, scale, bias, y, (int)M, (int)N, (int)K, st,
                            tao::tuning().tile_splits);
  tao::Int8WO pol;
  pol.w = reinterpret_cast<const uint4*>(w);
  pol.scale = scale;
  return tao::launch_gemm(x, pol, bias, y, (int)M, (int)N, (int)K, st);
}

extern "C" int tao_fp8wo_linear_bf16(const uint16_t* x, const uint8_t* w, const float* scale,
                                     const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                                     int64_t K, void* stream) {
  TAO_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "fp8 weight-only linear: negative size");
  TAO_CHECK_ARG(K % 32 == 0, "fp8 weight-only linear: K (%lld) must be a multiple of 32",
                (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31) && K < (1LL << 31) && M < (1LL << 31),
                "fp8 weight-only linear: size out of range");
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "fp8 weight-only linear: K must be > 0");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(scale, 4, "scale");
  hipStream_t st = tao::as_stream(stream);
  if (tao::use_gemv(M, N, K)) return tao::fp8wo_gemv(x, w, scale, bias, y, M, N, K, st);
  tao::Fp8WO pol;
  pol.w = reinterpret_cast<const uint4*>(w);
  pol.scale = scale;
  return tao::launch_gemm(x, pol, bias, y, (int)M, (int)N, (int)K, st);
}

extern "C" int tao_tune_linear_crossover(int max_gemv_m) {
  TAO_CHECK_ARG(max_gemv_m >= 0 && max_gemv_m <= 8, "tune: max_gemv_m must be in [0, 8]");
  tao::tuning().max_gemv_m = max_gemv_m;
  return TAO_OK;
}

extern "C" int tao_tune_fp8dyn_mfma(int on) {
  TAO_CHECK_ARG(on == 0 || on == 1, "tune: fp8dyn mfma must be 0 (built-in route) or 1");
  tao::tuning().fp8dyn_mfma = on;
  return TAO_OK;
}

extern "C" int tao_tune_mx_mfma(int on) {
  TAO_CHECK_ARG(on == 0 || on == 1, "tune: mx mfma must be 0 (built-in route) or 1");
  tao::tuning().mx_mfma = on;
  return TAO_OK;
}

extern "C" int tao_tune_blockfp8_mfma(int on) {
  TAO_CHECK_ARG(on == 0 || on == 1, "tune: blockfp8 mfma must be 0 (built-in route) or 1");
  tao::tuning().blockfp8_mfma = on;
  return TAO_OK;
}

// gemm_i8_lds_kernel selection in int8_scaled_mm_launch: 0 = auto, 1 = never, 2 = always (K % 128)
extern "C" int tao_tune_gemm_algo(int algo) {
  TAO_CHECK_ARG(algo >= 0 && algo <= 2,
                "tune: gemm algo must be 0 (auto), 1 (per-wave-column kernel only) or 2 (LDS-staged "
                "int8 kernel whenever K %% 128 == 0)");
  tao::tuning().gemm_algo = algo;
  return TAO_OK;
}

extern "C" int tao_tune_gemm_order(int order) {
  TAO_CHECK_ARG(order == 0 || order == 1,
                "tune: gemm order must be 0 (plain grid order) or 1 (XCD-grouped M tiles)");
  tao::tuning().gemm_order = order;
  return TAO_OK;
}

// Columns per wave of the MFMA GEMMs: 0 = built-in, 1 = 16, 2 = 32 (each A fragment read from
// LDS feeds two MFMAs). Calling thread only; for A/B measurement.
extern "C" int tao_tune_gemm_nw(int nw) {
  TAO_CHECK_ARG(nw >= 0 && nw <= 2, "tune: gemm nw must be 0 (auto), 1 or 2");
  tao::tuning().gemm_nw = nw;
  return TAO_OK;
}

// The measured shape table (gemm_table.inc): 0 = used (built-in), 1 = off (heuristic only).
// Calling thread only; for A/B measurement.
extern "C" int tao_tune_gemm_table(int off) {
  TAO_CHECK_ARG(off == 0 || off == 1, "tune: gemm table must be 0 (on) or 1 (off)");
  tao::tuning().gemm_table = off;
  return TAO_OK;
}

extern "C" int tao_tune_gemm(int m_tile, int k_groups, int splits) {
  TAO_CHECK_ARG(m_tile == 0 || m_tile == 16 || m_tile == 32 || m_tile == 64 || m_tile == 128,
                "tune: m_tile must be 0 (auto), 16, 32, 64 or 128");
  TAO_CHECK_ARG(k_groups == 0 || k_groups == 1 || k_groups == 2 || k_groups == 4,
                "tune: k_groups must be 0 (auto), 1, 2 or 4");
  TAO_CHECK_ARG(splits >= 0 && splits <= 64, "tune: splits must be in [0, 64]");
  tao::tuning().bm = m_tile;
  tao::tuning().kg = k_groups;
  tao::tuning().splits = splits;
  return TAO_OK;
}
