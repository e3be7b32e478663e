// 2:4 sparse int8 linear (Int8DynamicActivationInt8WeightConfig(layout=SemiSparseLayout())):
// int8 dynamic activations x a 2:4-compressed int8 weight on the sparse MFMA of gfx950. Replaces
// torch._cslt_compress / torch._cslt_sparse_mm (torchao/dtypes/uintx/semi_sparse_layout.py:42-73,
// 173-206), which a ROCm build of torch does not provide.
//
// Storage (ours; the reference's is cuSPARSELt-opaque). A dense weight [N][K], K % 128 == 0, of
// which every aligned group of four k holds at most two nonzeros, is kept as
//   values int8  [N][K/2]   the two kept elements of every group, in ascending position;
//   meta   int32 [N][K/32]  dword j of a row: sixteen 2-bit positions, bits [2i+1:2i] the position
//                           (0-3, inside its group of four) of value 16 j + i of the row.
// 0.5 + 0.125 = 0.625 B per dense weight. The kept positions of a group are its nonzero positions
// ascending, padded (fewer than two nonzeros) with its lowest zero positions, then sorted.
// A "chunk" is 16 B of values (32 dense k) plus its one meta dword; unchanged, the two are the A
// operand (4 VGPRs) and the index operand (cbsz = abid = 0: the whole register) of one lane of
// v_smfmac_i32_16x16x128_i8. Measured with one instruction (experiments/probe_smfmac_layout.hip,
// profiles/smfmac_layout_probe.txt): A lane (i = lane & 15, ga = lane >> 4) is row i and the 32
// dense k of chunk ga; value b of the lane is indexed by bits [2b+1:2b]; its partner in B is lane
// group 2 (ga & 1) + (b >> 3), byte 16 (ga >> 1) + 4 ((b & 7) >> 1) + position. So with chunk ga
// = dense k 32 ga .. 32 ga + 31 of a 128-k step, B lane (n = lane & 15, gb = lane >> 4) holds of
// column n the bytes k = 16 gb .. + 15 (VGPRs 0-3) and k = 64 + 16 gb .. + 15 (VGPRs 4-7): the
// two 16-B pieces of the dense 16x16x64 i8 MFMA, twice. The output is C[i][n]: a lane holds rows
// 4 (lane >> 4) .. + 3 of column lane & 15.
//
// Kernels:
//   sp24_compress_kernel / sp24_decompress_kernel: one thread per chunk, 16-B loads and stores;
//     a group with more than two nonzeros sets the caller's error word.
//   sp24_gemv_kernel (M up to the route boundary, sparse24_host.h): the byte-weight decomposition of
//     tao_gemv.h with a chunk per lane (a slice is 2048 dense k of one row). The int8 tokens are
//     staged in LDS. Per four kept values: the selector of one v_perm_b32 is built from 8 bits of
//     meta (sp24_selector), the permute gathers the four partner bytes out of two x dwords and one
//     v_dot4_i32_i8 follows; the selector is shared by the tile's tokens. NPT > 0 (one token): the
//     bf16 token is quantised into LDS under the first weight loads (int8_quant_row.h), as
//     int8dyn_gemv_kernel's FQ form does.
//   sp24_gemm_kernel: W is the A operand. A wave owns 16 output features and the BM tokens of its
//     tile; its A fragment and index register go from HBM to registers (no LDS, no re-layout) and
//     serve BM / 16 smfmacs per 128-k step. The x tile goes through a double-buffered, XOR-swizzled
//     LDS image, one barrier per step. K is split over KG k-groups inside the workgroup, summed in
//     k-group order through LDS (integer sums: any order is exact). A lane ends with four
//     consecutive output features of one token: one 8-B store of bf16.
// Epilogue of both routes, tao_int8_scaled_mm_bf16's: bf16(bf16(bf16(acc) * xs[m]) * ws[n])
// (+ bias), so every output equals the dense op on the decompressed weight bit for bit.
#include "int8_quant_row.h"
#include "sparse24_host.h"
#include "tao_gemv.h"

namespace tao {

namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// ---- compress / decompress ------------------------------------------------------------------------
// One dense group (4 int8 in a dword) -> its two kept bytes (low 16 bits) and 4-bit position code
// (p0 | p1 << 2); more than two nonzeros: the lowest two are kept and *bad is set.
__device__ __forceinline__ uint32_t sp24_pick(uint32_t d, uint32_t* code, bool* bad) {
  uint32_t keep = ((d & 0xFFu) ? 1u : 0u) | ((d & 0xFF00u) ? 2u : 0u) |
                  ((d & 0xFF0000u) ? 4u : 0u) | ((d & 0xFF000000u) ? 8u : 0u);
  if (__popc(keep) > 2) *bad = true;
  if (__popc(keep) < 2) keep |= (keep + 1u) & ~keep;  // lowest zero position
  if (__popc(keep) < 2) keep |= (keep + 1u) & ~keep;
  const uint32_t p0 = __ffs(keep) - 1, p1 = __ffs(keep & (keep - 1u)) - 1;
  *code = p0 | (p1 << 2);
  return ((d >> (8 * p0)) & 0xFFu) | (((d >> (8 * p1)) & 0xFFu) << 8);
}

__global__ __launch_bounds__(256) void sp24_compress_kernel(const uint4* __restrict__ w,
                                                            uint4* __restrict__ values,
                                                            uint32_t* __restrict__ meta,
                                                            int* __restrict__ err, int64_t nchunks) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nchunks) return;
  const uint4 lo = w[2 * t], hi = w[2 * t + 1];
  const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t v[4] = {0u, 0u, 0u, 0u}, m = 0u;
  bool bad = false;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    uint32_t code;
    v[g >> 1] |= sp24_pick(d[g], &code, &bad) << (16 * (g & 1));
    m |= code << (4 * g);
  }
  values[t] = make_uint4(v[0], v[1], v[2], v[3]);
  meta[t] = m;
  if (bad) atomicOr(err, 1);
}

__global__ __launch_bounds__(256) void sp24_decompress_kernel(const uint4* __restrict__ values,
                                                              const uint32_t* __restrict__ meta,
                                                              uint4* __restrict__ w,
                                                              int64_t nchunks) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nchunks) return;
  const uint4 vv = values[t];
  const uint32_t v[4] = {vv.x, vv.y, vv.z, vv.w}, m = meta[t];
  uint32_t d[8];
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const uint32_t pair = v[g >> 1] >> (16 * (g & 1)), code = m >> (4 * g);
    d[g] = ((pair & 0xFFu) << (8 * (code & 3u))) | (((pair >> 8) & 0xFFu) << (8 * ((code >> 2) & 3u)));
  }
  w[2 * t] = make_uint4(d[0], d[1], d[2], d[3]);
  w[2 * t + 1] = make_uint4(d[4], d[5], d[6], d[7]);
}

// ---- sparse GEMV ---------------------------------------------------------------------------------
struct Sp24GemvArgs {
  const void* x;         // int8 q [M][K] (NPT > 0: the bf16 token [K])
  const uint16_t* xs;    // [M] bf16 per-token scales (NPT > 0: unused)
  const uint4* v;        // values [N][K/32] chunks
  const uint32_t* meta;  // [N][K/32]
  const uint16_t* ws;    // [N]
  const uint16_t* bias;  // [N] or null
  uint16_t* y;           // [M][N]
  int M, N, K, Wk, G, S;
};

// v_perm_b32 selector of values dword j of a chunk: its four kept values are (p0, p1) of dense
// group 2 j (x dword d0, selector bytes 0-3) and of group 2 j + 1 (x dword d1, bytes 4-7). The four
// 2-bit fields of meta byte m go to bits 8 f by two shift-ors: t = m | m << 12, then t | t << 6 has
// every field at its byte with nothing else under the mask. The cheapest of the three expansions
// compared by instruction count; one multiply by 0x41041 is not among them, its
// overlapping copies carry into the next byte.
__device__ __forceinline__ uint32_t sp24_selector(uint32_t meta, int j) {
  const uint32_t m = (meta >> (8 * j)) & 0xFFu;
  const uint32_t t = m | (m << 12);
  return ((t | (t << 6)) & 0x03030303u) | 0x04040000u;
}

__device__ __forceinline__ int sp24_sdot4(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}

// where 16-B piece i of a token's int8 row sits in LDS: the two pieces of 32-B chunk c swap on
// every other run of 8 chunks, so that the two halves of a wave's 32-B reads use distinct bank
// groups (wo8_decode_kernel's rotation, tao_gemv.h)
__device__ __forceinline__ int sp24_x_piece(int i) { return (i & ~1) | ((i + (i >> 4)) & 1); }

template <int MT, int RPW, int NPT>
__global__ __launch_bounds__(512) void sp24_gemv_kernel(Sp24GemvArgs a) {
  constexpr bool FQ = NPT > 0;  // NPT: 16-B pieces of the bf16 token per thread (K <= 8 NPT T)
  static_assert(!FQ || MT == 1, "the fused quantisation is per token, M == 1");
  constexpr int V = RPW * MT;
  // [G][Wk][V] int partials | [8] wave maxima | int8 tokens [MT][K]
  extern __shared__ int lds_i[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wk = wave % a.Wk;
  const int rg = wave / a.Wk;
  const int row0 = (blockIdx.x * a.G + rg) * RPW;
  const int K = a.K, N = a.N, S = a.S, Wk = a.Wk;
  const int nchunk = K >> 5;  // chunks per row
  const int np = K >> 4;      // 16-B pieces of an int8 token
  const int nw = a.G * a.Wk;
  float* wmax = reinterpret_cast<float*>(lds_i + nw * V);
  uint4* xl = reinterpret_cast<uint4*>(lds_i + ((nw * V + 8 + 3) & ~3));

  int acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0;

  uint4 wv[RPW];
  uint32_t wm[RPW];
  auto load_w = [&](int s) __attribute__((always_inline)) {
    const int c = s * 64 + lane;
    const int cc = c < nchunk ? c : nchunk - 1;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const size_t i = (size_t)(n < N ? n : N - 1) * nchunk + cc;
      wv[r] = ld_nt_u4(a.v + i);
      wm[r] = ld_nt(a.meta + i);
    }
  };

  float sx[MT];
  if constexpr (FQ) {
    // the token's pieces before the first slice's weights (vector loads retire in issue order),
    // then amax, scale and codes: int8_quant_per_token_kernel's arithmetic (int8_dyn.hip)
    const uint4* xr = reinterpret_cast<const uint4*>(a.x);
    const int nvec = K >> 3;
    uint4 xv[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;
      xv[u] = xr[i < nvec ? i : nvec - 1];  // clamped, masked below
    }
    load_w(wk);  // Wk <= S: every wave owns a slice
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const bool ok = threadIdx.x + u * (int)blockDim.x < nvec;
      const uint4 v = ok ? xv[u] : make_uint4(0u, 0u, 0u, 0u);
      m = bf16_abs_max2(v.x, m);
      m = bf16_abs_max2(v.y, m);
      m = bf16_abs_max2(v.z, m);
      m = bf16_abs_max2(v.w, m);
    }
    m = wave_max(m);
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    float amax = wmax[0];
    for (int w = 1; w < nw; ++w) amax = fmaxf(amax, wmax[w]);
    const float st = token_scale(amax);
    const float rs = round_bf16(1.f / st);
    uint2* xq = reinterpret_cast<uint2*>(xl);
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = threadIdx.x + u * (int)blockDim.x;  // 8 codes: half of int8 piece i >> 1
      if (i < nvec) xq[2 * sp24_x_piece(i >> 1) + (i & 1)] = quant8(xv[u], rs);
    }
    sx[0] = st;
  } else {
    load_w(wk);
    const uint4* xg = reinterpret_cast<const uint4*>(a.x);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int mm = m < a.M ? m : a.M - 1;
      sx[m] = bf16_to_f32(a.xs[mm]);
      for (int i = threadIdx.x; i < np; i += (int)blockDim.x)
        xl[m * np + sp24_x_piece(i)] = xg[(size_t)mm * np + i];
    }
  }
  __syncthreads();

  for (int s = wk; s < S; s += Wk) {
    if (s != wk) load_w(s);
    const int c = s * 64 + lane;
    const bool cval = c < nchunk;
    const int cc = cval ? c : nchunk - 1;
    const int rot = (cc >> 3) & 1;
    const uint32_t keep = cval ? ~0u : 0u;  // lanes past K add exactly 0
    uint32_t xd[MT][8];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const uint4 lo = xl[m * np + 2 * cc + rot], hi = xl[m * np + 2 * cc + (rot ^ 1)];
      xd[m][0] = lo.x & keep, xd[m][1] = lo.y & keep, xd[m][2] = lo.z & keep, xd[m][3] = lo.w & keep;
      xd[m][4] = hi.x & keep, xd[m][5] = hi.y & keep, xd[m][6] = hi.z & keep, xd[m][7] = hi.w & keep;
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const uint32_t wd[4] = {wv[r].x, wv[r].y, wv[r].z, wv[r].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t sel = sp24_selector(wm[r], j);
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[r][m] = sp24_sdot4(__builtin_amdgcn_perm(xd[m][2 * j + 1], xd[m][2 * j], sel), wd[j],
                                 acc[r][m]);
      }
    }
  }

  int v[V];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) v[r * MT + m] = acc[r][m];
  wave_reduce_scatter<V>(v, lane);

  const WgTotal<int> t = wg_combine<V>(v[0], lds_i, lane, wk, rg, Wk);
  if (t.writer) {
    const int r = t.widx / MT, m = t.widx % MT;
    const int n = row0 + r;
    if (n < N && m < a.M) {
      float o = round_bf16(round_bf16((float)t.total) * sx[m]);
      o = round_bf16(o * bf16_to_f32(a.ws[n]));
      if (a.bias != nullptr) o = round_bf16(o + bf16_to_f32(a.bias[n]));
      a.y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

template <int MT, int RPW, int NPT>
int launch_sp24_gemv(Sp24GemvArgs a, const WoGemvLaunch& L, hipStream_t stream) {
  a.S = L.S;
  a.Wk = L.Wk;
  a.G = L.G;
  const size_t lds =
      (((size_t)L.G * L.Wk * RPW * MT + 8 + 3) & ~(size_t)3) * sizeof(int) + (size_t)MT * a.K;
  launch((sp24_gemv_kernel<MT, RPW, NPT>), dim3(L.grid), dim3(L.threads), lds, stream, a);
  return check_launch(NPT > 0 ? "sp24_gemv_fq_kernel" : "sp24_gemv_kernel");
}

// up to kWoGemvMaxM tokens in one launch
int sp24_gemv(Sp24GemvArgs a, hipStream_t stream) {
  const WoTune& tu = tuning().sp24;
  return dispatch_gemv_tile(a.M, tu.rpw, [&](auto mt, auto rpw) {
    constexpr int MT = decltype(mt)::value, RPW = decltype(rpw)::value;
    const WoGemvLaunch L = wo_gemv_launch(a.K / 32, a.N, MT, RPW, tu.wk, tu.g);
    return launch_sp24_gemv<MT, RPW, 0>(a, L, stream);
  });
}

// one bf16 token, quantised in the prologue: pieces per thread 1, 2, 4 or 8
template <int RPW>
int sp24_gemv_fq_rpw(Sp24GemvArgs a, hipStream_t stream) {
  const WoTune& tu = tuning().sp24;
  const WoGemvLaunch L = wo_gemv_launch(a.K / 32, a.N, 1, RPW, tu.wk, tu.g);
  const int per = (a.K / 8 + L.threads - 1) / L.threads;
  if (per <= 1) return launch_sp24_gemv<1, RPW, 1>(a, L, stream);
  if (per <= 2) return launch_sp24_gemv<1, RPW, 2>(a, L, stream);
  if (per <= 4) return launch_sp24_gemv<1, RPW, 4>(a, L, stream);
  if (per <= 8) return launch_sp24_gemv<1, RPW, 8>(a, L, stream);
  return set_error(TAO_ERR_INVALID_ARGUMENT,
                   "int8 sp24 dyn linear: K (%d) too long for the token prologue of %d threads",
                   a.K, L.threads);
}
int sp24_gemv_fq(Sp24GemvArgs a, hipStream_t stream) {
  switch (tuning().sp24.rpw) {
    case 2: return sp24_gemv_fq_rpw<2>(a, stream);
    case 8: return sp24_gemv_fq_rpw<8>(a, stream);
    default: return sp24_gemv_fq_rpw<4>(a, stream);
  }
}

// ---- sparse MFMA GEMM ----------------------------------------------------------------------------
struct Sp24GemmArgs {
  const int8_t* xq;      // [M][K]
  const uint16_t* xs;    // [M]
  const uint4* v;        // values [N][K/32] chunks
  const uint32_t* meta;  // [N][K/32]
  const uint16_t* ws;    // [N]
  const uint16_t* bias;  // [N] or null
  uint16_t* y;           // [M][N]
  int M, N, K, KG;
};

// The x tile of one 128-k step: BM rows of 8 16-B slots, slot s of row r at r * 8 + (s ^ mask(r)),
// mask(r) = (r >> 1) & 7. B lane (n, kq) reads slots kq and 4 + kq of row n. ds_read_b128 serves a
// wave in the lane groups listed at gemm_mfma.hip's x_slot: a group holds kq = 2 i at rows
// {0-3, 12-15} and kq = 2 i + 1 at rows {4-11}. The 16-B granule of (r, s) is 8 (r & 1) + (s ^
// mask(r)) mod 16: the first eight rows give 8 (r & 1) + (s0 ^ {0, 1, 6, 7}), the others 8 (r & 1)
// + (s0 ^ {2, 3, 4, 5}): sixteen distinct granules, every read conflict-free. The fill (8 lanes =
// the 8 slots of one row) is conflict-free either way.
__device__ __forceinline__ int sp24_x_slot(int row, int slot) {
  return row * 8 + (slot ^ ((row >> 1) & 7));
}

template <int BM, int NWV>
__global__ __launch_bounds__(512) void sp24_gemm_kernel(Sp24GemmArgs a) {
  constexpr int MT = BM / 16;            // 16-token tiles per wave
  constexpr int T = 64 * NWV;            // threads of a k-group
  constexpr int TILE = BM * 8;           // uint4 per x tile
  constexpr int XL = (TILE + T - 1) / T;  // 16-B x pieces per thread per step
  // [KG][2][TILE] x tiles; after the k loop [KG - 1][NWV][MT][64] accumulators
  extern __shared__ u32x4_t lds_x[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int kg = __builtin_amdgcn_readfirstlane(tid / T);
  const int wave = __builtin_amdgcn_readfirstlane((tid % T) >> 6);
  const int ktid = tid % T;
  const int M = a.M, N = a.N, K = a.K, KG = a.KG;
  const int n_blk = blockIdx.x * 16 * NWV;
  const int m_blk = blockIdx.y * BM;
  const int nsteps = K >> 7;
  const int J = (nsteps + KG - 1) / KG;  // steps per k-group: k-group g takes g, g + KG, ...
  const int nq = K >> 5;                 // chunks per weight row
  const int arow = n_blk + 16 * wave + (lane & 15);
  const size_t abase = (size_t)(arow < N ? arow : N - 1) * nq + (lane >> 4);
  u32x4_t* tile = lds_x + kg * 2 * TILE;

  size_t xsrc[XL];  // byte offset of this thread's piece of step 0
  int xdst[XL];
#pragma unroll
  for (int u = 0; u < XL; ++u) {
    const int p = ktid + u * T;
    const int row = (p >> 3) < BM ? (p >> 3) : BM - 1, slot = p & 7;
    const int gm = m_blk + row;
    xsrc[u] = (size_t)(gm < M ? gm : M - 1) * K + slot * 16;
    xdst[u] = sp24_x_slot(row, slot);
  }

  i32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = i32x4_t{0, 0, 0, 0};

  // a step past the end is loaded clamped and not computed
  const int s_first = kg < nsteps ? kg : nsteps - 1;
  uint4 av = ld_nt_u4(a.v + abase + 4 * s_first);
  uint32_t am = ld_nt(a.meta + abase + 4 * s_first);
  u32x4_t xr[XL];
#pragma unroll
  for (int u = 0; u < XL; ++u)
    xr[u] = *reinterpret_cast<const u32x4_t*>(a.xq + xsrc[u] + (size_t)s_first * 128);
#pragma unroll
  for (int u = 0; u < XL; ++u)
    if (ktid + u * T < TILE) tile[xdst[u]] = xr[u];
  __syncthreads();

  for (int j = 0; j < J; ++j) {
    const bool more = j + 1 < J;
    uint4 avn = av;
    uint32_t amn = am;
    if (more) {
      const int sj = kg + (j + 1) * KG, sn = sj < nsteps ? sj : nsteps - 1;
      avn = ld_nt_u4(a.v + abase + 4 * sn);
      amn = ld_nt(a.meta + abase + 4 * sn);
#pragma unroll
      for (int u = 0; u < XL; ++u)
        xr[u] = *reinterpret_cast<const u32x4_t*>(a.xq + xsrc[u] + (size_t)sn * 128);
    }
    if (kg + j * KG < nsteps) {  // k-group-uniform
      const u32x4_t* buf = tile + (j & 1) * TILE;
      const i32x4_t af = {(int)av.x, (int)av.y, (int)av.z, (int)av.w};
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int row = 16 * t + (lane & 15), kq = lane >> 4;
        const u32x4_t lo = buf[sp24_x_slot(row, kq)], hi = buf[sp24_x_slot(row, 4 + kq)];
        const i32x8_t bf = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
                            (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        acc[t] = __builtin_amdgcn_smfmac_i32_16x16x128_i8(af, bf, acc[t], (int)am, 0, 0);
      }
    }
    if (more) {
      // the other buffer was last read in step j - 1, before the barrier that ended it
      u32x4_t* nxt = tile + ((j + 1) & 1) * TILE;
#pragma unroll
      for (int u = 0; u < XL; ++u)
        if (ktid + u * T < TILE) nxt[xdst[u]] = xr[u];
    }
    __syncthreads();
    av = avn;
    am = amn;
  }

  // k-groups 1 .. KG - 1 hand their tiles to k-group 0, which sums them in k-group order
  i32x4_t* red = reinterpret_cast<i32x4_t*>(lds_x);
  if (kg > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t) red[(((kg - 1) * NWV + wave) * MT + t) * 64 + lane] = acc[t];
  }
  __syncthreads();
  if (kg != 0) return;
  for (int q = 1; q < KG; ++q) {
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] += red[(((q - 1) * NWV + wave) * MT + t) * 64 + lane];
  }

  // lane: token 16 t + (lane & 15), output features n0 .. n0 + 3
  const int n0 = n_blk + 16 * wave + 4 * (lane >> 4);
  float wsc[4], bs[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + r < N ? n0 + r : N - 1;
    wsc[r] = bf16_to_f32(a.ws[n]);
    bs[r] = a.bias != nullptr ? bf16_to_f32(a.bias[n]) : 0.f;
  }
  const bool vec = (N & 3) == 0 && n0 + 3 < N;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m_blk + 16 * t + (lane & 15);
    if (m >= M) continue;  // row tail
    const float sxm = bf16_to_f32(a.xs[m]);
    uint16_t o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float f = round_bf16(round_bf16((float)acc[t][r]) * sxm);
      f = round_bf16(f * wsc[r]);
      if (a.bias != nullptr) f = round_bf16(f + bs[r]);
      o[r] = f32_to_bf16(f);
    }
    uint16_t* yp = a.y + (size_t)m * N + n0;
    if (vec) {
      *reinterpret_cast<uint2*>(yp) = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16),
                                                 (uint32_t)o[2] | ((uint32_t)o[3] << 16));
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n0 + r < N) yp[r] = o[r];
    }
  }
}

template <int BM, int NWV>
int launch_sp24_gemm(Sp24GemmArgs a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + 16 * NWV - 1) / (16 * NWV)), (unsigned)((a.M + BM - 1) / BM));
  const size_t lds = (size_t)a.KG * 2 * BM * 128;
  launch((sp24_gemm_kernel<BM, NWV>), grid, dim3(64 * NWV * a.KG), lds, stream, a);
  return check_launch("sp24_gemm_kernel");
}

int sp24_gemm(Sp24GemmArgs a, hipStream_t stream) {
  const Tuning& tu = tuning();
  const Sp24GemmShape s = sp24_gemm_shape(a.M, a.N, a.K, tu.sp24_bm, tu.sp24_nwv, tu.sp24_kg);
  a.KG = s.kg;
#define TAO_SP24_NWV(BM)                                    \
  switch (s.nwv) {                                          \
    case 1: return launch_sp24_gemm<BM, 1>(a, stream);      \
    case 2: return launch_sp24_gemm<BM, 2>(a, stream);      \
    default: return launch_sp24_gemm<BM, 4>(a, stream);     \
  }
  switch (s.bm) {
    case 16: TAO_SP24_NWV(16)
    case 32: TAO_SP24_NWV(32)
    default: TAO_SP24_NWV(64)
  }
#undef TAO_SP24_NWV
}

// what the four entries check of a compressed weight's shape
int check_sp24_shape(const char* what, int64_t N, int64_t K) {
  TAO_CHECK_ARG(N >= 0 && K >= 0, "%s: negative size", what);
  TAO_CHECK_ARG(K % 128 == 0, "%s: K (%lld) must be a multiple of 128", what, (long long)K);
  TAO_CHECK_ARG(N < (1LL << 31) && K < (1LL << 31) && N * K < (1LL << 36),
                "%s: size out of range", what);
  return TAO_OK;
}

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_int8_sp24_compress(const int8_t* w, int8_t* values, int32_t* meta, int32_t* err, int64_t N,
                           int64_t K, void* stream) {
  if (const int rc = check_sp24_shape("int8 sp24 compress", N, K)) return rc;
  if (N == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ARG(w != nullptr && values != nullptr && meta != nullptr && err != nullptr,
                "int8 sp24 compress: w, values, meta and err are required");
  TAO_CHECK_ALIGN(w, 16, "w");
  TAO_CHECK_ALIGN(values, 16, "values");
  TAO_CHECK_ALIGN(meta, 4, "meta");
  TAO_CHECK_ALIGN(err, 4, "err");
  const int64_t nchunks = N * K / 32;
  launch(sp24_compress_kernel, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint4*>(w), reinterpret_cast<uint4*>(values),
         reinterpret_cast<uint32_t*>(meta), reinterpret_cast<int*>(err), nchunks);
  return check_launch("sp24_compress_kernel");
}

int tao_int8_sp24_decompress(const int8_t* values, const int32_t* meta, int8_t* w, int64_t N,
                             int64_t K, void* stream) {
  if (const int rc = check_sp24_shape("int8 sp24 decompress", N, K)) return rc;
  if (N == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ARG(w != nullptr && values != nullptr && meta != nullptr,
                "int8 sp24 decompress: values, meta and w are required");
  TAO_CHECK_ALIGN(values, 16, "values");
  TAO_CHECK_ALIGN(meta, 4, "meta");
  TAO_CHECK_ALIGN(w, 16, "w");
  const int64_t nchunks = N * K / 32;
  launch(sp24_decompress_kernel, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint4*>(values),
         reinterpret_cast<const uint32_t*>(meta), reinterpret_cast<uint4*>(w), nchunks);
  return check_launch("sp24_decompress_kernel");
}

int tao_int8_sp24_route(int64_t M, int64_t N, int64_t K) {
  (void)N;
  return sp24_route(M, K, tuning().sp24.route, tuning().sp24.max_m);
}

int tao_int8_sp24_scaled_mm_bf16(const int8_t* xq, const uint16_t* xs, const int8_t* values,
                                 const int32_t* meta, const uint16_t* ws, const uint16_t* bias,
                                 uint16_t* y, int64_t M, int64_t N, int64_t K, void* stream) {
  if (const int rc = check_sp24_shape("int8 sp24 scaled mm", N, K)) return rc;
  TAO_CHECK_ARG(M >= 0 && M < (1LL << 20), "int8 sp24 scaled mm: M (%lld) must be in [0, 2^20)",
                (long long)M);
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "int8 sp24 scaled mm: K must be > 0");
  TAO_CHECK_ARG(xq != nullptr && xs != nullptr && values != nullptr && meta != nullptr &&
                    ws != nullptr && y != nullptr,
                "int8 sp24 scaled mm: xq, xs, values, meta, ws and y are required");
  TAO_CHECK_ALIGN(xq, 16, "xq");
  TAO_CHECK_ALIGN(values, 16, "values");
  TAO_CHECK_ALIGN(meta, 4, "meta");
  TAO_CHECK_ALIGN(y, 8, "y");
  const hipStream_t st = as_stream(stream);
  const int route = sp24_route(M, K, tuning().sp24.route, tuning().sp24.max_m);
  if (route == kSp24RouteGemm) {
    Sp24GemmArgs a{xq, xs, reinterpret_cast<const uint4*>(values),
                   reinterpret_cast<const uint32_t*>(meta), ws, bias, y, (int)M, (int)N, (int)K, 1};
    return sp24_gemm(a, st);
  }
  TAO_CHECK_ARG(sp24_gemv_fits(M, K),
                "int8 sp24 scaled mm: the GEMV stages its tokens in LDS, K (%lld) is too long",
                (long long)K);
  // for_gemv_pieces (tao_gemv.h) walks bf16 tokens; these are int8 rows with a scale each
  for (int64_t m0 = 0; m0 < M; m0 += kWoGemvMaxM) {
    const int m = (int)(M - m0 < kWoGemvMaxM ? M - m0 : kWoGemvMaxM);
    Sp24GemvArgs a{xq + m0 * K, xs + m0, reinterpret_cast<const uint4*>(values),
                   reinterpret_cast<const uint32_t*>(meta), ws, bias, y + m0 * N, m, (int)N, (int)K,
                   0, 0, 0};
    if (const int rc = sp24_gemv(a, st)) return rc;
  }
  return TAO_OK;
}

int tao_int8_sp24_dyn_linear_bf16(const uint16_t* x, const int8_t* values, const int32_t* meta,
                                  const uint16_t* ws, const uint16_t* bias, uint16_t* y, int64_t M,
                                  int64_t N, int64_t K, void* stream) {
  if (const int rc = check_sp24_shape("int8 sp24 dyn linear", N, K)) return rc;
  TAO_CHECK_ARG(M >= 0 && M <= 1,
                "int8 sp24 dyn linear: the fused path is one token (M <= 1, got %lld)", (long long)M);
  TAO_CHECK_ARG(K <= 32768, "int8 sp24 dyn linear: K (%lld) must be <= 32768 (token prologue)",
                (long long)K);
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "int8 sp24 dyn linear: K must be > 0");
  TAO_CHECK_ARG(x != nullptr && values != nullptr && meta != nullptr && ws != nullptr &&
                    y != nullptr,
                "int8 sp24 dyn linear: x, values, meta, ws and y are required");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(values, 16, "values");
  TAO_CHECK_ALIGN(meta, 4, "meta");
  Sp24GemvArgs a{x, nullptr, reinterpret_cast<const uint4*>(values),
                 reinterpret_cast<const uint32_t*>(meta), ws, bias, y, 1, (int)N, (int)K, 0, 0, 0};
  return sp24_gemv_fq(a, as_stream(stream));
}

int tao_tune_sp24(int route, int max_gemv_m, int rows_per_wave, int waves_k, int row_groups) {
  TAO_CHECK_ARG(route >= kSp24RouteAuto && route <= kSp24RouteGemm,
                "tune: sp24 route must be 0 (auto), 1 (gemv) or 2 (sparse MFMA gemm)");
  if (const int rc = check_wo_tune("sp24", 0, max_gemv_m, rows_per_wave, waves_k, row_groups))
    return rc;
  tuning().sp24 = WoTune{route, max_gemv_m, rows_per_wave, waves_k, row_groups};
  return TAO_OK;
}

int tao_tune_sp24_gemm(int bm, int waves_n, int k_groups) {
  TAO_CHECK_ARG(bm == 0 || bm == 16 || bm == 32 || bm == 64,
                "tune: sp24 gemm bm must be 0 (auto), 16, 32 or 64");
  TAO_CHECK_ARG(waves_n == 0 || waves_n == 1 || waves_n == 2 || waves_n == 4,
                "tune: sp24 gemm waves_n must be 0 (auto), 1, 2 or 4");
  TAO_CHECK_ARG(k_groups >= 0 && k_groups <= 8, "tune: sp24 gemm k_groups must be in [0, 8]");
  tuning().sp24_bm = bm;
  tuning().sp24_nwv = waves_n;
  tuning().sp24_kg = k_groups;
  return TAO_OK;
}

}  // extern "C"
