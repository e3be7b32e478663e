// 2:4 sparse int4 weight-only linear (Int4WeightOnlyConfig(layout=MarlinSparseLayout())): bf16
// activations x a 2:4-compressed symmetric uint4 weight (zero point 8). Replaces the reference's
// CUDA-only marlin_24_gemm (torchao/dtypes/uintx/marlin_sparse_layout.py:37-74,
// torchao/csrc/cuda/sparse_marlin), which a ROCm build does not have.
//
// Storage (ours; the reference's Marlin pre-packing is not reproduced). A dense weight of codes
// [N][K], K % 128 == 0, of which every aligned group of four k holds at most two codes != 8, is
// kept as
//   values int32 [N][K/16]  dword j of a row: the eight kept codes of dense k 16 j .. 16 j + 15,
//                           code i in bits [4i+3:4i], in ascending position;
//   meta   int32 [N][K/32]  sparse24.hip's: sixteen 2-bit positions per dword;
//   scale  bf16  [K/g][N]   one per (group, row), group-major: the four rows a GEMM lane ends with
//                           are one 8-B load.
// 0.25 + 0.125 = 0.375 B per dense weight plus scales. Kept positions of a group: its non-8
// positions ascending, padded with its lowest code-8 positions, then sorted.
//
// y[m][n] = bf16( sum_g s[g][n] * sum_{k in g} x[m][k] (q[n][k] - 8) + bias[n] ): fp32 throughout,
// one rounding; both routes form it, so they agree bit for bit wherever the fp32 sums are exact.
//
// v_smfmac_f32_16x16x64_bf16, measured with one instruction
// (experiments/probe_smfmac_bf16_layout.hip, profiles/smfmac_bf16_layout_probe.txt): A lane
// (i = lane & 15, ga = lane >> 4) is row i and 16 dense k ("chunk ga", 8 kept values). With
// cbsz = 0, value b of the lane is indexed by bits [2b+1:2b] of the 16-bit half abid & 1 of the
// index register (abid bit 1 is ignored; with cbsz = 1 abid is ignored and the low half used).
// Its partner in B is lane group 2 (ga & 1) + (b >> 2), element 8 (ga >> 1) + 4 ((b & 3) >> 1) +
// position: B lane (n, gb) holds of column n, in elements 0-7, dense k 8 (gb & 1) .. + 7 of chunk
// gb >> 1 and, in elements 8-15, the same of chunk 2 + (gb >> 1). The output is C[i][n]: a lane
// holds rows 4 (lane >> 4) .. + 3 of column lane & 15.
//
// Kernels:
//   int4_sp24_compress_kernel / int4_sp24_decompress_kernel: one thread per 32 dense k, from and to
//     int32 codes (16-B accesses); a group with more than two non-8 codes sets the error word.
//   int4_sp24_gemv_kernel (M up to the route boundary, int4_sparse24_host.h): tao_gemv.h's row /
//     k-wave / row-group decomposition with 16 B of values and 8 B of meta per lane (a slice is
//     4096 dense k of one row). The bf16 tokens are staged once in LDS. Per dense group of four a
//     v_perm_b32 selector built from 4 bits of meta picks the two partner bf16 halves out of the
//     group's two x dwords; it is shared by the tile's tokens. The two kept nibbles become the
//     exact bf16 pair (128 + q) (the magic exponent of int4_gemv.hip), one v_dot2_f32_bf16 takes
//     the pair and a second against (-136, -136) takes the 128 + 8 back: gfx950 has no packed
//     bf16 subtract, and a dot2 is cheaper than converting the pair. The lane's fp32 sum over its 64
//     k meets the group's scale once.
//   int4_sp24_gemm_kernel: W is the sparse A operand. A wave owns 16 output features and the BM
//     tokens of its tile. Per 128-k step a lane loads 8 B of values and its meta dword from HBM
//     into registers (no LDS, no re-layout): the 32 dense k 32 ga .. + 31 of its row. Values dword
//     t (chunk ga of smfmac t = dense k 32 ga + 16 t .. + 15) is decoded to four VGPRs of bf16
//     (q - 8) and the meta dword is the index register of both (abid = t). The two smfmacs of a
//     step are one scale group: they accumulate into a zeroed fragment, then acc += s * part. (A
//     16-B load per lane would spread a smfmac over two scale groups; 8 B keeps the group whole.)
//     The k order the smfmac wants is met by the LDS read addresses of x: B lane (n, gb) of smfmac
//     t reads 16-B slots 4 (gb >> 1) + 2 t + (gb & 1) and 8 + the same of row n of a
//     double-buffered, XOR-swizzled image, one barrier per step. K is split over KG k-groups
//     inside the workgroup, summed in k-group order through LDS.
#include "int4_sparse24_host.h"
#include "tao_gemv.h"

namespace tao {

namespace {

typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16_t __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint2 ld_nt_u2(const uint2* p) {  // 8-B non-temporal load
  const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
  return make_uint2(v[0], v[1]);
}

// ---- compress / decompress ------------------------------------------------------------------------
// One dense group (four int32 codes) -> its two kept codes (low 8 bits: code p0 | code p1 << 4) and
// 4-bit position code (p0 | p1 << 2); more than two codes != 8: the lowest two are kept, *bad set.
__device__ __forceinline__ uint32_t i4sp24_pick(uint4 c, uint32_t* code, bool* bad) {
  const uint32_t q[4] = {c.x & 15u, c.y & 15u, c.z & 15u, c.w & 15u};
  uint32_t keep = (q[0] != 8u ? 1u : 0u) | (q[1] != 8u ? 2u : 0u) | (q[2] != 8u ? 4u : 0u) |
                  (q[3] != 8u ? 8u : 0u);
  if (__popc(keep) > 2) *bad = true;
  if (__popc(keep) < 2) keep |= (keep + 1u) & ~keep;  // lowest code-8 position
  if (__popc(keep) < 2) keep |= (keep + 1u) & ~keep;
  const uint32_t p0 = __ffs(keep) - 1, p1 = __ffs(keep & (keep - 1u)) - 1;
  *code = p0 | (p1 << 2);
  const uint32_t packed = q[0] | (q[1] << 4) | (q[2] << 8) | (q[3] << 12);
  return ((packed >> (4 * p0)) & 15u) | (((packed >> (4 * p1)) & 15u) << 4);
}

__global__ __launch_bounds__(256) void int4_sp24_compress_kernel(const uint4* __restrict__ codes,
                                                                 uint2* __restrict__ values,
                                                                 uint32_t* __restrict__ meta,
                                                                 int* __restrict__ err,
                                                                 int64_t nunits) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nunits) return;
  uint32_t v[2] = {0u, 0u}, m = 0u;
  bool bad = false;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    uint32_t code;
    v[g >> 2] |= i4sp24_pick(codes[8 * t + g], &code, &bad) << (8 * (g & 3));
    m |= code << (4 * g);
  }
  values[t] = make_uint2(v[0], v[1]);
  meta[t] = m;
  if (bad) atomicOr(err, 1);
}

__global__ __launch_bounds__(256) void int4_sp24_decompress_kernel(
    const uint2* __restrict__ values, const uint32_t* __restrict__ meta, uint4* __restrict__ codes,
    int64_t nunits) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nunits) return;
  const uint2 vv = values[t];
  const uint32_t v[2] = {vv.x, vv.y}, m = meta[t];
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const uint32_t pair = v[g >> 2] >> (8 * (g & 3)), code = m >> (4 * g);
    const uint32_t p0 = code & 3u, p1 = (code >> 2) & 3u, q0 = pair & 15u, q1 = (pair >> 4) & 15u;
    uint32_t d[4];
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p) d[p] = p == p1 ? q1 : (p == p0 ? q0 : 8u);
    codes[8 * t + g] = make_uint4(d[0], d[1], d[2], d[3]);
  }
}

// ---- sparse GEMV ---------------------------------------------------------------------------------
struct I4Sp24Args {
  const uint16_t* x;      // bf16 [M][K]
  const uint4* v;         // values [N][K/64] lane chunks of 16 B
  const uint2* meta;      // [N][K/64] lane chunks of 8 B
  const uint16_t* scale;  // bf16 [K/g][N]
  const uint16_t* bias;   // [N] or null
  uint16_t* y;            // [M][N]
  int M, N, K;
  int per_row;            // group_size == K: one scale per row
  int Wk, G, S, KG;
};

// The v_perm_b32 selectors of the four dense groups of one values dword from their 16 bits of meta.
// Group g keeps positions (p0, p1) = bits [4g+1:4g], [4g+3:4g+2]; its x is the dword pair (d1:d0) =
// bf16 halves 0-3, half p at bytes 2p, 2p + 1. The fields of a meta byte go to one byte each as
// sp24_selector does (sparse24.hip), doubled; a permute of that word with itself repeats each
// field over a half's two bytes and 0x01000100 makes the second byte of each the odd one.
__device__ __forceinline__ void i4sp24_selectors(uint32_t meta16, uint32_t (&sel)[4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t m = (meta16 >> (8 * h)) & 0xFFu;
    const uint32_t t = m | (m << 12);
    const uint32_t f = ((t | (t << 6)) & 0x03030303u) << 1;  // bytes: 2 p0, 2 p1 | 2 p0', 2 p1'
    sel[2 * h] = __builtin_amdgcn_perm(f, f, 0x01010000u) | 0x01000100u;
    sel[2 * h + 1] = __builtin_amdgcn_perm(f, f, 0x03030202u) | 0x01000100u;
  }
}

// The four bf16 pairs (128 + q_2g, 128 + q_2g+1) of a values dword: byte g holds both nibbles
__device__ __forceinline__ void i4sp24_pairs(uint32_t w, uint32_t (&p)[4]) {
  const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;
  p[0] = __builtin_amdgcn_perm(hi, lo, 0x0C040C00u) | 0x43004300u;
  p[1] = __builtin_amdgcn_perm(hi, lo, 0x0C050C01u) | 0x43004300u;
  p[2] = __builtin_amdgcn_perm(hi, lo, 0x0C060C02u) | 0x43004300u;
  p[3] = __builtin_amdgcn_perm(hi, lo, 0x0C070C03u) | 0x43004300u;
}

// where 16-B piece i of a token's bf16 row sits in LDS: the eight pieces of lane chunk c = i >> 3
// are XORed with (c >> 1) & 7, so that the 16 lanes of a ds_read_b128 pass (128 B apart) use
// sixteen distinct 16-B granules of the 256-B bank line
__device__ __forceinline__ int i4sp24_x_piece(int i) { return i ^ ((i >> 4) & 7); }

template <int MT, int RPW>
__global__ __launch_bounds__(512) void int4_sp24_gemv_kernel(I4Sp24Args a) {
  constexpr int V = RPW * MT;
  // [G][Wk][V] float partials | bf16 tokens [MT][K]
  extern __shared__ float lds_f[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wk = wave % a.Wk;
  const int rg = wave / a.Wk;
  const int row0 = (blockIdx.x * a.G + rg) * RPW;
  const int K = a.K, N = a.N, S = a.S, Wk = a.Wk;
  const int nchunk = K >> 6;  // lane chunks per row
  const int np = K >> 3;      // 16-B pieces of a bf16 token
  uint4* xl = reinterpret_cast<uint4*>(lds_f + ((a.G * a.Wk * V + 3) & ~3));

  float acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

  uint4 wv[RPW];
  uint2 wm[RPW];
  auto load_w = [&](int s) __attribute__((always_inline)) {
    const int c = s * 64 + lane;
    const int cc = c < nchunk ? c : nchunk - 1;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = row0 + r;
      const size_t i = (size_t)(n < N ? n : N - 1) * nchunk + cc;
      wv[r] = ld_nt_u4(a.v + i);
      wm[r] = ld_nt_u2(a.meta + i);
    }
  };

  load_w(wk);  // Wk <= S: every wave owns a slice; in flight under the staging of x
  const uint4* xg = reinterpret_cast<const uint4*>(a.x);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mm = m < a.M ? m : a.M - 1;
    for (int i = threadIdx.x; i < np; i += (int)blockDim.x)
      xl[m * np + i4sp24_x_piece(i)] = xg[(size_t)mm * np + i];
  }
  __syncthreads();

  for (int s = wk; s < S; s += Wk) {
    if (s != wk) load_w(s);
    const int c = s * 64 + lane;
    if (c < nchunk) {  // lanes past K add nothing
      const int sw = (c >> 1) & 7;
      float d[RPW][MT];
#pragma unroll
      for (int r = 0; r < RPW; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) d[r][m] = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // values dword j: dense k 16 j .. + 15 of the chunk
        uint32_t xd[MT][8];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const uint4 lo = xl[m * np + 8 * c + ((2 * j) ^ sw)];
          const uint4 hi = xl[m * np + 8 * c + ((2 * j + 1) ^ sw)];
          xd[m][0] = lo.x, xd[m][1] = lo.y, xd[m][2] = lo.z, xd[m][3] = lo.w;
          xd[m][4] = hi.x, xd[m][5] = hi.y, xd[m][6] = hi.z, xd[m][7] = hi.w;
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          const uint32_t wd[4] = {wv[r].x, wv[r].y, wv[r].z, wv[r].w};
          const uint32_t md = (j < 2 ? wm[r].x : wm[r].y) >> (16 * (j & 1));
          uint32_t sel[4], p[4];
          i4sp24_selectors(md, sel);
          i4sp24_pairs(wd[j], p);
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
              const uint32_t xp = __builtin_amdgcn_perm(xd[m][2 * g + 1], xd[m][2 * g], sel[g]);
              d[r][m] = dot2_bf16(xp, p[g], d[r][m]);
              d[r][m] = dot2_bf16(xp, 0xC308C308u, d[r][m]);  // (-136, -136)
            }
        }
      }
      const int grp = a.per_row ? 0 : c >> 1;
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const int n = row0 + r;
        const float sc = bf16_to_f32(a.scale[(size_t)grp * N + (n < N ? n : N - 1)]);
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[r][m] += sc * d[r][m];
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
      float o = t.total;
      if (a.bias != nullptr) o += bf16_to_f32(a.bias[n]);
      a.y[(size_t)m * N + n] = f32_to_bf16(o);
    }
  }
}

template <int MT, int RPW>
int launch_i4sp24_gemv(I4Sp24Args a, const WoGemvLaunch& L, hipStream_t stream) {
  a.S = L.S;
  a.Wk = L.Wk;
  a.G = L.G;
  const size_t lds =
      (((size_t)L.G * L.Wk * RPW * MT + 3) & ~(size_t)3) * sizeof(float) + (size_t)MT * a.K * 2;
  launch((int4_sp24_gemv_kernel<MT, RPW>), dim3(L.grid), dim3(L.threads), lds, stream, a);
  return check_launch("int4_sp24_gemv_kernel");
}

// up to kWoGemvMaxM tokens in one launch. Every workgroup stages the tokens, so by default row
// groups fill it to 8 waves at every M (a slice is 4096 k: most rows are one or two slices long).
int i4sp24_gemv(I4Sp24Args a, hipStream_t stream) {
  const WoTune& tu = tuning().i4sp24;
  return dispatch_gemv_tile(a.M, tu.rpw, [&](auto mt, auto rpw) {
    constexpr int MT = decltype(mt)::value, RPW = decltype(rpw)::value;
    const WoGemvLaunch L = wo_gemv_launch(a.K / 64, a.N, MT, RPW, tu.wk, tu.g > 0 ? tu.g : 8);
    return launch_i4sp24_gemv<MT, RPW>(a, L, stream);
  });
}

// ---- sparse MFMA GEMM ----------------------------------------------------------------------------
// The x tile of one 128-k step: BM rows of 16 16-B slots, slot s of row r at r * 16 + (s ^ (r & 15)).
// The 16 lanes of a ds_read_b128 pass read one slot of 16 rows: sixteen distinct granules of the
// 256-B bank line. The fill (16 lanes = the 16 slots of one row) is a permutation of one line.
__device__ __forceinline__ int i4sp24_x_slot(int row, int slot) {
  return row * 16 + (slot ^ (row & 15));
}

// eight codes of a values dword -> the A operand of one smfmac: bf16 (q - 8), value b = code b.
// (128 + q) is formed in the fp32 mantissa, 136 subtracted exactly, the pair converted back.
__device__ __forceinline__ bf16x8_t i4sp24_decode(uint32_t w) {
  bf16x8_t o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t b = w >> (8 * i);
    const f32x2_t f = {__uint_as_float(0x43000000u | ((b & 15u) << 16)) - 136.f,
                       __uint_as_float(0x43000000u | ((b & 0xF0u) << 12)) - 136.f};
    const bf16x2_t h = __builtin_convertvector(f, bf16x2_t);
    o[2 * i] = h[0];
    o[2 * i + 1] = h[1];
  }
  return o;
}

template <int BM, int NWV>
__global__ __launch_bounds__(512) void int4_sp24_gemm_kernel(I4Sp24Args a) {
  constexpr int MT = BM / 16;             // 16-token tiles per wave
  constexpr int T = 64 * NWV;             // threads of a k-group
  constexpr int TILE = BM * 16;           // uint4 per x tile
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
  const int arow = n_blk + 16 * wave + (lane & 15);
  // the lane's 8 B of values and meta dword of step 0, in units of each
  const size_t abase = (size_t)(arow < N ? arow : N - 1) * (K >> 5) + (lane >> 4);
  const uint2* av_p = reinterpret_cast<const uint2*>(a.v);
  const uint32_t* am_p = reinterpret_cast<const uint32_t*>(a.meta);
  u32x4_t* tile = lds_x + kg * 2 * TILE;

  // lane: token 16 t + (lane & 15), output features n0 .. n0 + 3
  const int n0 = n_blk + 16 * wave + 4 * (lane >> 4);
  const bool vec = (N & 3) == 0 && n0 + 3 < N;
  auto load_scale = [&](int step, float (&sc)[4]) __attribute__((always_inline)) {
    const uint16_t* sp = a.scale + (size_t)(a.per_row ? 0 : step) * N;
    if (vec) {
      const uint2 u = *reinterpret_cast<const uint2*>(sp + n0);
      sc[0] = bf16lo_to_f32(u.x), sc[1] = bf16hi_to_f32(u.x);
      sc[2] = bf16lo_to_f32(u.y), sc[3] = bf16hi_to_f32(u.y);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[r] = bf16_to_f32(sp[n0 + r < N ? n0 + r : N - 1]);
    }
  };

  size_t xsrc[XL];  // element offset of this thread's piece of step 0
  int xdst[XL];
#pragma unroll
  for (int u = 0; u < XL; ++u) {
    const int p = ktid + u * T;
    const int row = (p >> 4) < BM ? (p >> 4) : BM - 1, slot = p & 15;
    const int gm = m_blk + row;
    xsrc[u] = (size_t)(gm < M ? gm : M - 1) * K + slot * 8;
    xdst[u] = i4sp24_x_slot(row, slot);
  }

  f32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // a step past the end is loaded clamped and not computed
  const int s_first = kg < nsteps ? kg : nsteps - 1;
  uint2 av = ld_nt_u2(av_p + abase + 4 * s_first);
  uint32_t am = ld_nt(am_p + abase + 4 * s_first);
  float sc[4];
  load_scale(s_first, sc);
  u32x4_t xr[XL];
#pragma unroll
  for (int u = 0; u < XL; ++u)
    xr[u] = *reinterpret_cast<const u32x4_t*>(a.x + xsrc[u] + (size_t)s_first * 128);
#pragma unroll
  for (int u = 0; u < XL; ++u)
    if (ktid + u * T < TILE) tile[xdst[u]] = xr[u];
  __syncthreads();

  for (int j = 0; j < J; ++j) {
    const bool more = j + 1 < J;
    uint2 avn = av;
    uint32_t amn = am;
    float scn[4] = {sc[0], sc[1], sc[2], sc[3]};
    if (more) {
      const int sj = kg + (j + 1) * KG, sn = sj < nsteps ? sj : nsteps - 1;
      avn = ld_nt_u2(av_p + abase + 4 * sn);
      amn = ld_nt(am_p + abase + 4 * sn);
      load_scale(sn, scn);
#pragma unroll
      for (int u = 0; u < XL; ++u)
        xr[u] = *reinterpret_cast<const u32x4_t*>(a.x + xsrc[u] + (size_t)sn * 128);
    }
    if (kg + j * KG < nsteps) {  // k-group-uniform
      const u32x4_t* buf = tile + (j & 1) * TILE;
      const bf16x8_t a0 = i4sp24_decode(av.x), a1 = i4sp24_decode(av.y);
      const int gb = lane >> 4, s0 = 4 * (gb >> 1) + (gb & 1);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int row = 16 * t + (lane & 15);
        const u32x4_t b[4] = {buf[i4sp24_x_slot(row, s0)], buf[i4sp24_x_slot(row, 8 + s0)],
                              buf[i4sp24_x_slot(row, s0 + 2)], buf[i4sp24_x_slot(row, 10 + s0)]};
        struct Pair { u32x4_t lo, hi; };
        const bf16x16_t b0 = __builtin_bit_cast(bf16x16_t, (Pair{b[0], b[1]}));
        const bf16x16_t b1 = __builtin_bit_cast(bf16x16_t, (Pair{b[2], b[3]}));
        f32x4_t part = {0.f, 0.f, 0.f, 0.f};
        part = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a0, b0, part, (int)am, 0, 0);
        part = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a1, b1, part, (int)am, 0, 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] += sc[r] * part[r];
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
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = scn[r];
  }

  // k-groups 1 .. KG - 1 hand their tiles to k-group 0, which sums them in k-group order
  f32x4_t* red = reinterpret_cast<f32x4_t*>(lds_x);
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

  float bs[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    bs[r] = a.bias != nullptr ? bf16_to_f32(a.bias[n0 + r < N ? n0 + r : N - 1]) : 0.f;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m_blk + 16 * t + (lane & 15);
    if (m >= M) continue;  // token tail
    uint16_t o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16(acc[t][r] + bs[r]);
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
int launch_i4sp24_gemm(I4Sp24Args a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + 16 * NWV - 1) / (16 * NWV)), (unsigned)((a.M + BM - 1) / BM));
  const size_t lds = (size_t)a.KG * 2 * BM * 256;
  launch((int4_sp24_gemm_kernel<BM, NWV>), grid, dim3(64 * NWV * a.KG), lds, stream, a);
  return check_launch("int4_sp24_gemm_kernel");
}

int i4sp24_gemm(I4Sp24Args a, hipStream_t stream) {
  const Tuning& tu = tuning();
  const I4Sp24GemmShape s =
      i4sp24_gemm_shape(a.M, a.N, a.K, tu.i4sp24_bm, tu.i4sp24_nwv, tu.i4sp24_kg);
  a.KG = s.kg;
#define TAO_I4SP24_NWV(BM)                                  \
  switch (s.nwv) {                                          \
    case 1: return launch_i4sp24_gemm<BM, 1>(a, stream);    \
    case 2: return launch_i4sp24_gemm<BM, 2>(a, stream);    \
    default: return launch_i4sp24_gemm<BM, 4>(a, stream);   \
  }
  switch (s.bm) {
    case 16: TAO_I4SP24_NWV(16)
    case 32: TAO_I4SP24_NWV(32)
    default: TAO_I4SP24_NWV(64)
  }
#undef TAO_I4SP24_NWV
}

// what the entries check of a compressed weight's shape
int check_i4sp24_shape(const char* what, int64_t N, int64_t K) {
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

int tao_int4_sp24_compress(const int32_t* codes, int32_t* values, int32_t* meta, int32_t* err,
                           int64_t N, int64_t K, void* stream) {
  if (const int rc = check_i4sp24_shape("int4 sp24 compress", N, K)) return rc;
  if (N == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ARG(codes != nullptr && values != nullptr && meta != nullptr && err != nullptr,
                "int4 sp24 compress: codes, values, meta and err are required");
  TAO_CHECK_ALIGN(codes, 16, "codes");
  TAO_CHECK_ALIGN(values, 8, "values");
  TAO_CHECK_ALIGN(meta, 4, "meta");
  TAO_CHECK_ALIGN(err, 4, "err");
  const int64_t nunits = N * K / 32;
  launch(int4_sp24_compress_kernel, dim3((unsigned)((nunits + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint4*>(codes),
         reinterpret_cast<uint2*>(values), reinterpret_cast<uint32_t*>(meta),
         reinterpret_cast<int*>(err), nunits);
  return check_launch("int4_sp24_compress_kernel");
}

int tao_int4_sp24_decompress(const int32_t* values, const int32_t* meta, int32_t* codes, int64_t N,
                             int64_t K, void* stream) {
  if (const int rc = check_i4sp24_shape("int4 sp24 decompress", N, K)) return rc;
  if (N == 0 || K == 0) return TAO_OK;
  TAO_CHECK_ARG(codes != nullptr && values != nullptr && meta != nullptr,
                "int4 sp24 decompress: values, meta and codes are required");
  TAO_CHECK_ALIGN(values, 8, "values");
  TAO_CHECK_ALIGN(meta, 4, "meta");
  TAO_CHECK_ALIGN(codes, 16, "codes");
  const int64_t nunits = N * K / 32;
  launch(int4_sp24_decompress_kernel, dim3((unsigned)((nunits + 255) / 256)), dim3(256), 0,
         as_stream(stream), reinterpret_cast<const uint2*>(values),
         reinterpret_cast<const uint32_t*>(meta), reinterpret_cast<uint4*>(codes), nunits);
  return check_launch("int4_sp24_decompress_kernel");
}

int tao_int4_sp24_route(int64_t M, int64_t N, int64_t K) {
  (void)N;
  return i4sp24_route(M, K, tuning().i4sp24.route, tuning().i4sp24.max_m);
}

int tao_int4_sp24_linear_bf16(const uint16_t* x, const int32_t* values, const int32_t* meta,
                              const uint16_t* scale, const uint16_t* bias, uint16_t* y, int64_t M,
                              int64_t N, int64_t K, int64_t group_size, void* stream) {
  if (const int rc = check_i4sp24_shape("int4 sp24 linear", N, K)) return rc;
  TAO_CHECK_ARG(M >= 0 && M < (1LL << 20), "int4 sp24 linear: M (%lld) must be in [0, 2^20)",
                (long long)M);
  TAO_CHECK_ARG(group_size == 128 || group_size == K,
                "int4 sp24 linear: group_size (%lld) must be 128 or K (%lld)",
                (long long)group_size, (long long)K);
  if (M == 0 || N == 0) return TAO_OK;
  TAO_CHECK_ARG(K > 0, "int4 sp24 linear: K must be > 0");
  TAO_CHECK_ARG(x != nullptr && values != nullptr && meta != nullptr && scale != nullptr &&
                    y != nullptr,
                "int4 sp24 linear: x, values, meta, scale and y are required");
  TAO_CHECK_ALIGN(x, 16, "x");
  TAO_CHECK_ALIGN(values, 16, "values");
  TAO_CHECK_ALIGN(meta, 8, "meta");
  TAO_CHECK_ALIGN(scale, 8, "scale");
  TAO_CHECK_ALIGN(y, 8, "y");
  const hipStream_t st = as_stream(stream);
  const int route = i4sp24_route(M, K, tuning().i4sp24.route, tuning().i4sp24.max_m);
  I4Sp24Args a{x, reinterpret_cast<const uint4*>(values), reinterpret_cast<const uint2*>(meta),
               scale, bias, y, (int)M, (int)N, (int)K, group_size == K ? 1 : 0,
               0, 0, 0, 1};
  if (route == kI4Sp24RouteGemm) return i4sp24_gemm(a, st);
  TAO_CHECK_ARG(i4sp24_gemv_fits(M, K),
                "int4 sp24 linear: the GEMV stages its tokens in LDS, K (%lld) is too long",
                (long long)K);
  return for_gemv_pieces(x, y, M, N, K, [&](const uint16_t* xp, uint16_t* yp, int m) {
    I4Sp24Args p = a;
    p.x = xp;
    p.y = yp;
    p.M = m;
    return i4sp24_gemv(p, st);
  });
}

int tao_tune_int4_sp24(int route, int max_gemv_m, int rows_per_wave, int waves_k, int row_groups,
                       int bm, int waves_n, int k_groups) {
  TAO_CHECK_ARG(route >= kI4Sp24RouteAuto && route <= kI4Sp24RouteGemm,
                "tune: int4_sp24 route must be 0 (auto), 1 (gemv) or 2 (sparse MFMA gemm)");
  if (const int rc = check_wo_tune("int4_sp24", 0, max_gemv_m, rows_per_wave, waves_k, row_groups))
    return rc;
  TAO_CHECK_ARG(bm == 0 || bm == 16 || bm == 32 || bm == 64,
                "tune: int4_sp24 bm must be 0 (auto), 16, 32 or 64");
  TAO_CHECK_ARG(waves_n == 0 || waves_n == 1 || waves_n == 2 || waves_n == 4,
                "tune: int4_sp24 waves_n must be 0 (auto), 1, 2 or 4");
  TAO_CHECK_ARG(k_groups >= 0 && k_groups <= 8, "tune: int4_sp24 k_groups must be in [0, 8]");
  tuning().i4sp24 = WoTune{route, max_gemv_m, rows_per_wave, waves_k, row_groups};
  tuning().i4sp24_bm = bm;
  tuning().i4sp24_nwv = waves_n;
  tuning().i4sp24_kg = k_groups;
  return TAO_OK;
}

}  // extern "C"
