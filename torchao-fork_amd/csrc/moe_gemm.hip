// The many-token expert FFN of an MoE layer on 3-D int4 weights (torchao/prototype/moe_quant):
//   tao_moe_route                  : stable counting sort of the T * A token activations by expert
//   tao_int4wo_grouped_linear_bf16 : every expert's linear over its own sorted rows in one launch,
//                                    the token gather folded into the x load; with a second weight
//                                    stack, gate and up together and SwiGLU in the epilogue
//   tao_moe_combine_bf16           : the expert-weighted sum back to token order, in a fixed order
// Replaces the many-token branch of ConditionalFeedForwardAOQuantizable
// (prototype/moe_quant/quantizable_moe_modules.py:113-191): argsort / histc / cumsum, a host-side
// slice per expert (one device-to-host sync each), x[indices] and three linears per expert, cat,
// gather, mul and a scatter_add of bf16 atomics: about 10 + 6 E launches and E syncs. Here: four or
// five launches, no sync, no atomics on data, graph-capturable, a pure function of the inputs.
// No kernel here waits on another workgroup: no tickets, no spin loops, no split-K.
#include "gemm_mfma_policy.h"
#include "moe_host.h"

namespace tao {

TAO_DECODE_ERROR_WORD(moe_decode_status)

namespace {

// ---- route ---------------------------------------------------------------------------------
// One workgroup per expert e, 256 threads. Pass 1 counts the activations whose clamped expert is
// below e (offsets[e]); pass 2 walks the indices in order, 256 at a time, and gives the entries of
// expert e their rank by a ballot prefix within each wave and the four waves' totals through LDS:
// ascending flat index within the expert, which is what argsort(stable=True) gives.
__device__ __forceinline__ int clamp_expert(int64_t v, int E) {
  return v < 0 ? 0 : (v >= E ? E - 1 : (int)v);
}

__global__ __launch_bounds__(256) void moe_route_kernel(const int64_t* __restrict__ idx, int R,
                                                        int E, int* __restrict__ offsets,
                                                        int* __restrict__ order,
                                                        int* __restrict__ inverse) {
  __shared__ int red[4];
  __shared__ int tot[2][4];
  const int e = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int below = 0;
  bool bad = false;
  for (int i = tid; i < R; i += 256) {
    const int64_t v = idx[i];
    bad |= v < 0 || v >= E;
    below += clamp_expert(v, E) < e ? 1 : 0;
  }
  if (e == 0 && bad) flag_decode_error(kDecodeErrExpert);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) below += __shfl_xor(below, d);
  if (lane == 0) red[wave] = below;
  __syncthreads();
  const int base = red[0] + red[1] + red[2] + red[3];
  if (tid == 0) {
    offsets[e] = base;
    if (e == E - 1) offsets[E] = R;
  }
  int run = 0;  // entries of expert e before this round
  for (int i0 = 0, round = 0; i0 < R; i0 += 256, ++round) {
    const int i = i0 + tid;
    const bool mine = i < R && clamp_expert(idx[i], E) == e;
    const unsigned long long b = __ballot(mine);
    const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (lane == 0) tot[round & 1][wave] = __popcll(b);
    __syncthreads();  // (the other buffer was last read before the previous round's barrier)
    const int* t = tot[round & 1];
    const int wbase = (wave > 0 ? t[0] : 0) + (wave > 1 ? t[1] : 0) + (wave > 2 ? t[2] : 0);
    if (mine) {
      const int p = base + run + wbase + before;  // < R: a count of distinct entries
      order[p] = i;
      inverse[i] = p;
    }
    run += t[0] + t[1] + t[2] + t[3];
  }
}

// ---- combine -------------------------------------------------------------------------------
// One thread per 8 columns of one token: the token's A sorted positions in ascending order (a
// bubble network on registers, A <= 8), then acc = bf16(acc + bf16(y2[p] * w)) from +0: the
// reference's mul, then scatter_add as the CPU executes it (source rows in ascending order).
__global__ __launch_bounds__(256) void moe_combine_kernel(const uint4* __restrict__ y2,
                                                          const uint16_t* __restrict__ w,
                                                          const int* __restrict__ inverse,
                                                          uint4* __restrict__ out, int T, int A,
                                                          int D8, int R) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y;
  if (c >= D8) return;
  int pos[kMoeMaxTopK];
  float wt[kMoeMaxTopK];
#pragma unroll
  for (int a = 0; a < kMoeMaxTopK; ++a) {
    const int f = t * A + (a < A ? a : A - 1);
    const int p = inverse[f];
    pos[a] = a < A ? (p < 0 ? 0 : (p >= R ? R - 1 : p)) : 0x7FFFFFFF;
    wt[a] = bf16_to_f32(w[f]);
  }
#pragma unroll
  for (int i = 0; i < kMoeMaxTopK - 1; ++i) {
#pragma unroll
    for (int j = 0; j < kMoeMaxTopK - 1 - i; ++j) {
      const bool sw = pos[j] > pos[j + 1];
      const int pa = sw ? pos[j + 1] : pos[j], pb = sw ? pos[j] : pos[j + 1];
      const float wa = sw ? wt[j + 1] : wt[j], wb = sw ? wt[j] : wt[j + 1];
      pos[j] = pa;
      pos[j + 1] = pb;
      wt[j] = wa;
      wt[j + 1] = wb;
    }
  }
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
  for (int a = 0; a < kMoeMaxTopK; ++a) {
    if (a < A) {
      const uint4 v = y2[(size_t)pos[a] * D8 + c];
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[2 * i] = round_bf16(acc[2 * i] + round_bf16(bf16lo_to_f32(d[i]) * wt[a]));
        acc[2 * i + 1] = round_bf16(acc[2 * i + 1] + round_bf16(bf16hi_to_f32(d[i]) * wt[a]));
      }
    }
  }
  out[(size_t)t * D8 + c] = make_uint4(pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]),
                                       pack_bf16x2(acc[4], acc[5]), pack_bf16x2(acc[6], acc[7]));
}

// ---- grouped linear ------------------------------------------------------------------------
// gemm_mfma_kernel's int4 tile (gemm_mfma.hip) with one k-group, 16 columns per wave and no
// split-K, built from the same parts: Int4WO's setup / load / prep / frag / slot / xswz on the
// expert's own pointers, LineLoader<128> behind them, the D-deep register ring and the
// double-buffered XOR-swizzled x image on v_mfma_f32_16x16x32_bf16. What differs:
//  * blockIdx.y is a tile number, not a row: each wave finds the tile's expert and row range in
//    `offsets` by itself (lane l: experts 4 l .. 4 l + 3, a shuffle prefix over the tile counts),
//    so a workgroup past the last tile returns before its first barrier;
//  * an x row is fetched through src_row[p] / row_div (the token gather), rows past the expert's
//    range are clamped to its last row for the load and dropped at the store;
//  * DUAL: a second weight stack rides in the ring and keeps a second accumulator set over the
//    same A fragments; the epilogue writes swiglu_pair(bf16 a, bf16 b).
constexpr int kBN = 64;
constexpr int kSlots = 32;  // 16-B x slots per row per step: 256 bf16

__device__ __forceinline__ int x_slot(int row, int slot) {
  return row * kSlots + (slot ^ Int4WO::xswz(row));
}

struct MoeTile {
  int e, m0, m1;  // expert, first sorted row of the tile, end of the expert's rows
};

// the tile `ty` in BM-row tiles over the experts' ranges; e < 0: past the last tile. Every value
// is clamped to [0, R], so whatever `offsets` holds, no row outside the buffers is named.
template <int BM>
__device__ __forceinline__ MoeTile find_tile(const int* __restrict__ offsets, int E, int R, int ty,
                                             int lane) {
  int lo[5], nt[4];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int i = 4 * lane + q;
    const int v = offsets[i < E ? i : E];
    lo[q] = v < 0 ? 0 : (v > R ? R : v);
  }
  int s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = lo[q + 1] - lo[q];
    nt[q] = (4 * lane + q < E && c > 0) ? (c + BM - 1) / BM : 0;
    s += nt[q];
  }
  int incl = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d);
    if (lane >= d) incl += v;
  }
  int a = incl - s;
  const unsigned long long b = __ballot(ty >= a && ty < incl);
  MoeTile t{-1, 0, 0};
  if (b == 0) return t;
  int e = 0, m0 = 0, m1 = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (ty >= a && ty < a + nt[q]) {
      e = 4 * lane + q;
      m0 = lo[q] + (ty - a) * BM;
      m1 = lo[q + 1];
    }
    a += nt[q];
  }
  const int src = __ffsll(b) - 1;
  t.e = __builtin_amdgcn_readfirstlane(__shfl(e, src));
  t.m0 = __builtin_amdgcn_readfirstlane(__shfl(m0, src));
  t.m1 = __builtin_amdgcn_readfirstlane(__shfl(m1, src));
  return t;
}

template <int BM, int D, bool DUAL>
__global__ __launch_bounds__(256) void moe_grouped_linear_kernel(
    const uint8_t* __restrict__ x, int x_rows, const int* __restrict__ src_row, int row_div,
    Int4WO pa, Int4WO pb, const int* __restrict__ offsets, int R, int E, uint16_t* __restrict__ y,
    int N, int K) {
  typedef Int4WO P;
  typedef f32x4_t Acc;
  constexpr int NS = DUAL ? 2 : 1;             // weight stacks
  constexpr int MT = BM / 16;
  constexpr int XSB = 512;                     // x bytes per row per step
  constexpr int RPP = 256 / kSlots;            // x rows loaded per 256-thread pass
  constexpr int XLOADS = BM * kSlots / 256;    // 16-B x pieces per thread per step
  constexpr int TILE = BM * kSlots;            // uint4 per x tile
  // one LDS array: [2][x tile], then the per-wave weight stages (one per stack)
  __shared__ uint4 lds[2 * TILE + 4 * NS * P::kStage];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const MoeTile tile = find_tile<BM>(offsets, E, R, (int)blockIdx.y, lane);
  if (tile.e < 0) return;  // past the last tile (wave-uniform and the same in all four waves)
  const int m_blk = tile.m0, m_end = tile.m1;
  const int nsteps = (K + P::kKStep - 1) / P::kKStep;
  const int row_bytes = K * 2;

  // the expert's slices of the stacks: [N][K/32] chunks, [N][K/g] (scale, zero) dwords
  const size_t wchunks = (size_t)N * (size_t)(K >> 5);
  const size_t zdwords = (size_t)N * (size_t)(K >> 5 >> pa.gshift);
  pa.wq += (size_t)tile.e * wchunks;
  pa.sz += (size_t)tile.e * zdwords;
  if constexpr (DUAL) {
    pb.wq += (size_t)tile.e * wchunks;
    pb.sz += (size_t)tile.e * zdwords;
  }
  const int bn = blockIdx.x * kBN + wave * 16 + (lane & 15);
  typename P::Lane wl[NS];
  wl[0] = pa.setup(bn, lane, N, K);
  if constexpr (DUAL) wl[1] = pb.setup(bn, lane, N, K);
  const int kq = lane >> 4;
  uint4* xs = lds;
  uint4* wstage = lds + 2 * TILE + wave * NS * P::kStage;

  // this thread's x pieces: sorted rows m_blk + row0 + RPP i, clamped to the expert's last row
  // (computed and dropped), fetched from x row src_row[p] / row_div, itself clamped to x
  const int row0 = tid / kSlots, xslot = tid % kSlots;
  const int xslot_b = xslot * 16;
  const Rsrc xrs = make_rsrc(x, (uint32_t)x_rows * (uint32_t)row_bytes);
  uint32_t xv[XLOADS];
  int xlds[XLOADS];
#pragma unroll
  for (int i = 0; i < XLOADS; ++i) {
    const int p = m_blk + row0 + RPP * i;
    const int pc = p < m_end ? p : m_end - 1;
    int r = pc;
    if (src_row != nullptr) r = src_row[pc] / row_div;
    r = r < 0 ? 0 : (r < x_rows ? r : x_rows - 1);
    xv[i] = (uint32_t)r * (uint32_t)row_bytes + xslot_b;
    xlds[i] = x_slot(row0 + RPP * i, xslot);
  }
  const bool ragged = (row_bytes % XSB) != 0;

  Acc acc[NS][MT];
#pragma unroll
  for (int w = 0; w < NS; ++w)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[w][t] = Acc{0, 0, 0, 0};

  uint4 xr[D][XLOADS];
  typename P::Chunk wr[D][NS];

  auto load_step = [&](int j, uint4 (&xdst)[XLOADS], typename P::Chunk (&wdst)[NS])
                       __attribute__((always_inline)) {
    const int st = j < nsteps ? j : nsteps - 1;  // past the last step: re-read it (never used)
#pragma unroll
    for (int i = 0; i < XLOADS; ++i) xdst[i] = bload16(xrs, xv[i], st * XSB);
    wdst[0] = pa.load(wl[0], st);
    if constexpr (DUAL) wdst[1] = pb.load(wl[1], st);
  };
  auto store_x = [&](const uint4 (&src)[XLOADS], int j) __attribute__((always_inline)) {
    uint4* dst = xs + (j & 1) * TILE;
    if (!ragged) {
#pragma unroll
      for (int i = 0; i < XLOADS; ++i) dst[xlds[i]] = src[i];
    } else {
      // k tail -> 0 (an AND mask: a select here compiles to a branch)
      const uint32_t keep = j * XSB + xslot_b < row_bytes ? ~0u : 0u;
#pragma unroll
      for (int i = 0; i < XLOADS; ++i) dst[xlds[i]] = and16(src[i], keep);
    }
  };
  auto body = [&](auto uc, int j) __attribute__((always_inline)) {
    constexpr int u = decltype(uc)::value;
    load_step(j + D - 1, xr[(u + D - 1) % D], wr[(u + D - 1) % D]);
    typename P::Prep pw[NS];
    pw[0] = pa.prep(wr[u][0], wstage, lane);
    if constexpr (DUAL) pw[1] = pb.prep(wr[u][1], wstage + P::kStage, lane);
    const uint4* xb = xs + (j & 1) * TILE;
#pragma unroll
    for (int s = 0; s < P::kMfma; ++s) {
      bf16x8_t bfrag[NS];
      bfrag[0] = pa.frag(pw[0], s);
      if constexpr (DUAL) bfrag[1] = pb.frag(pw[1], s);
      const int slot = P::slot(s, kq);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        // one A fragment read from LDS feeds both stacks
        const uint4 a = xb[x_slot(t * 16 + (lane & 15), slot)];
#pragma unroll
        for (int w = 0; w < NS; ++w) acc[w][t] = P::mfma(a, bfrag[w], acc[w][t]);
      }
    }
    if (j + 1 < nsteps) store_x(xr[(u + 1) % D], j + 1);
    __syncthreads();
  };

  static_for<0, D - 1>([&](auto i) __attribute__((always_inline)) {
    load_step(decltype(i)::value, xr[decltype(i)::value], wr[decltype(i)::value]);
  });
  store_x(xr[0], 0);
  __syncthreads();

  int j = 0;
  for (; j + D <= nsteps; j += D)
    static_for<0, D>([&](auto uc) __attribute__((always_inline)) {
      body(uc, j + decltype(uc)::value);
    });
  static_for<0, D - 1>([&](auto uc) __attribute__((always_inline)) {
    if (j + decltype(uc)::value < nsteps) body(uc, j + decltype(uc)::value);
  });

  // C/D map: col = lane & 15 (n), row = 4 * (lane >> 4) + i (m)
  if (bn < N) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m_blk + t * 16 + 4 * (lane >> 4) + i;
        if (m < m_end) {
          uint16_t v = f32_to_bf16(acc[0][t][i]);
          if constexpr (DUAL)
            v = swiglu_pair((uint32_t)v | ((uint32_t)f32_to_bf16(acc[1][t][i]) << 16));
          y[(size_t)m * N + bn] = v;
        }
      }
    }
  }
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

template <int BM, bool DUAL>
void launch_grouped_linear(dim3 grid, hipStream_t st, const uint8_t* x, int x_rows,
                           const int* src_row, int row_div, const Int4WO& pa, const Int4WO& pb,
                           const int* offsets, int R, int E, uint16_t* y, int N, int K) {
  // ring depth as gemm_mfma.hip's launch_one has it for the 512-B x rows of int4
  constexpr int D = BM <= 16 ? 4 : (BM <= 32 ? 3 : 2);
  launch((moe_grouped_linear_kernel<BM, D, DUAL>), grid, dim3(256), 0, st, x, x_rows, src_row,
         row_div, pa, pb, offsets, R, E, y, N, K);
}

}  // namespace

}  // namespace tao

extern "C" int tao_moe_route(const int64_t* expert_indices, int64_t R, int64_t A, int64_t E,
                             int32_t* offsets, int32_t* order, int32_t* inverse, void* stream) {
  TAO_CHECK_ARG(E >= 1 && E <= tao::kMoeMaxExperts, "moe route: E (%lld) must be in [1, %d]",
                (long long)E, tao::kMoeMaxExperts);
  TAO_CHECK_ARG(A >= 1 && A <= tao::kMoeMaxTopK, "moe route: top-k (%lld) must be in [1, %d]",
                (long long)A, tao::kMoeMaxTopK);
  TAO_CHECK_ARG(R >= 0 && R < (1LL << 24) && R % A == 0,
                "moe route: R (%lld) must be a multiple of top-k (%lld) below 2^24", (long long)R,
                (long long)A);
  TAO_CHECK_ARG(offsets != nullptr, "moe route: offsets is required");
  TAO_CHECK_ARG(R == 0 || (expert_indices != nullptr && order != nullptr && inverse != nullptr),
                "moe route: expert_indices, order and inverse are required");
  tao::launch(tao::moe_route_kernel, dim3((unsigned)E), dim3(256), 0, tao::as_stream(stream),
              expert_indices, (int)R, (int)E, offsets, order, inverse);
  return tao::check_launch("moe_route_kernel");
}

extern "C" int tao_moe_row_tile(int64_t R, int64_t E) {
  return tao::moe_row_tile(R, E, tao::tuning().moe_bm);
}

extern "C" int tao_moe_dual(int64_t R, int64_t E) {
  return tao::moe_dual(tao::moe_row_tile(R, E, tao::tuning().moe_bm), tao::tuning().moe_dual) ? 1
                                                                                              : 0;
}

extern "C" int tao_int4wo_grouped_linear_bf16(const uint16_t* x, int64_t x_rows,
                                              const int32_t* src_row, int64_t row_div,
                                              const uint32_t* packed,
                                              const uint16_t* scales_and_zeros,
                                              const uint32_t* packed_b,
                                              const uint16_t* scales_and_zeros_b,
                                              const int32_t* offsets, int64_t R, int64_t E,
                                              uint16_t* y, int64_t N, int64_t K,
                                              int64_t group_size, void* stream) {
  const int gs = tao::gshift_of(group_size);
  TAO_CHECK_ARG(gs >= 0, "int4 grouped linear: qGroupSize must be 32, 64, 128, or 256 (got %lld)",
                (long long)group_size);
  TAO_CHECK_ARG(E >= 1 && E <= tao::kMoeMaxExperts,
                "int4 grouped linear: E (%lld) must be in [1, %d]", (long long)E,
                tao::kMoeMaxExperts);
  TAO_CHECK_ARG(R >= 0 && R < (1LL << 24) && N >= 0 && N < (1LL << 31) && K >= 0 &&
                    K < (1LL << 31) && x_rows >= 0 && x_rows < (1LL << 31),
                "int4 grouped linear: size out of range");
  TAO_CHECK_ARG(K % 32 == 0 && K % group_size == 0,
                "int4 grouped linear: K (%lld) must be a multiple of 32 and of group_size (%lld)",
                (long long)K, (long long)group_size);
  TAO_CHECK_ARG(N * (K / 2) < (1LL << 32) && x_rows * K * 2 < (1LL << 32),
                "int4 grouped linear: an expert's weight and x must each stay below 4 GiB");
  TAO_CHECK_ARG(row_div >= 1 && row_div < (1LL << 31), "int4 grouped linear: row_div must be >= 1");
  TAO_CHECK_ARG((packed_b == nullptr) == (scales_and_zeros_b == nullptr),
                "int4 grouped linear: the second stack needs both packed_b and scales_and_zeros_b");
  if (R == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0 && x_rows > 0, "int4 grouped linear: K and x_rows must be > 0");
  TAO_CHECK_ARG(src_row != nullptr || x_rows >= R,
                "int4 grouped linear: without src_row x must hold R (%lld) rows, got %lld",
                (long long)R, (long long)x_rows);
  TAO_CHECK_ARG(x != nullptr && packed != nullptr && scales_and_zeros != nullptr &&
                    offsets != nullptr && y != nullptr,
                "int4 grouped linear: x, packed, scales_and_zeros, offsets and y are required");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(packed, 16, "packed weight");
  TAO_CHECK_ALIGN(scales_and_zeros, 4, "scales_and_zeros");
  if (packed_b != nullptr) {
    TAO_CHECK_ALIGN(packed_b, 16, "packed weight (second stack)");
    TAO_CHECK_ALIGN(scales_and_zeros_b, 4, "scales_and_zeros (second stack)");
  }
  // an expert's slices keep the 16-B alignment of the stack: N * K / 2 bytes each
  TAO_CHECK_ARG((N * (K / 2)) % 16 == 0,
                "int4 grouped linear: an expert's N * K / 2 weight bytes must be a multiple of 16");
  const int bm = tao::moe_row_tile(R, E, tao::tuning().moe_bm);
  tao::Int4WO pa, pb;
  pa.wq = reinterpret_cast<const uint4*>(packed);
  pa.sz = reinterpret_cast<const uint32_t*>(scales_and_zeros);
  pa.gshift = gs;
  pb = pa;
  const bool dual = packed_b != nullptr;
  if (dual) {
    pb.wq = reinterpret_cast<const uint4*>(packed_b);
    pb.sz = reinterpret_cast<const uint32_t*>(scales_and_zeros_b);
  }
  const dim3 grid((unsigned)((N + tao::kBN - 1) / tao::kBN),
                  (unsigned)tao::moe_tile_bound(R, E, bm));
  hipStream_t st = tao::as_stream(stream);
  const uint8_t* xb = reinterpret_cast<const uint8_t*>(x);
#define TAO_MOE_GO(BM, DUAL)                                                                     \
  tao::launch_grouped_linear<BM, DUAL>(grid, st, xb, (int)x_rows, src_row, (int)row_div, pa, pb, \
                                       offsets, (int)R, (int)E, y, (int)N, (int)K)
  if (dual) {
    if (bm == 16) TAO_MOE_GO(16, true);
    else if (bm == 32) TAO_MOE_GO(32, true);
    else TAO_MOE_GO(64, true);
  } else {
    if (bm == 16) TAO_MOE_GO(16, false);
    else if (bm == 32) TAO_MOE_GO(32, false);
    else TAO_MOE_GO(64, false);
  }
#undef TAO_MOE_GO
  return tao::check_launch("moe_grouped_linear_kernel");
}

extern "C" int tao_moe_combine_bf16(const uint16_t* y2, const uint16_t* expert_weights,
                                    const int32_t* inverse, uint16_t* out, int64_t T, int64_t A,
                                    int64_t D, void* stream) {
  TAO_CHECK_ARG(A >= 1 && A <= tao::kMoeMaxTopK, "moe combine: top-k (%lld) must be in [1, %d]",
                (long long)A, tao::kMoeMaxTopK);
  TAO_CHECK_ARG(T >= 0 && T <= 65535 && T * A < (1LL << 24),
                "moe combine: T (%lld) must be in [0, 65535]", (long long)T);
  TAO_CHECK_ARG(D >= 0 && D < (1LL << 31) && D % 8 == 0,
                "moe combine: D (%lld) must be a multiple of 8", (long long)D);
  if (T == 0 || D == 0) return TAO_OK;
  TAO_CHECK_ARG(y2 != nullptr && expert_weights != nullptr && inverse != nullptr && out != nullptr,
                "moe combine: y2, expert_weights, inverse and out are required");
  TAO_CHECK_ALIGN(y2, 16, "y2");
  TAO_CHECK_ALIGN(out, 16, "out");
  const int D8 = (int)(D / 8);
  tao::launch(tao::moe_combine_kernel, dim3((unsigned)((D8 + 255) / 256), (unsigned)T), dim3(256),
              0, tao::as_stream(stream), reinterpret_cast<const uint4*>(y2), expert_weights,
              inverse, reinterpret_cast<uint4*>(out), (int)T, (int)A, D8, (int)(T * A));
  return tao::check_launch("moe_combine_kernel");
}

extern "C" int tao_tune_moe(int bm, int dual) {
  TAO_CHECK_ARG(bm == 0 || bm == 16 || bm == 32 || bm == 64,
                "tune: moe bm must be 0 (built-in rule), 16, 32 or 64");
  TAO_CHECK_ARG(dual >= 0 && dual <= 2,
                "tune: moe dual must be 0 (built-in rule), 1 (gate and up in two launches) or 2 "
                "(one launch)");
  tao::tuning().moe_bm = bm;
  tao::tuning().moe_dual = dual;
  return TAO_OK;
}
