// int8 x int8 GEMM with both operands staged through LDS: the second Int8Dyn GEMM (routed to by
// int8_scaled_mm_launch, gemm_mfma.hip, at M >= 128).
// gemm_mfma_kernel gives each wave 16 columns x all BM rows: every MFMA reads its own 1-KiB A
// fragment from LDS and every 16-column weight piece is regrouped per wave, ~2 KiB of LDS
// traffic per MFMA, so at M = 128 the LDS port, not the MFMA or HBM, sets the pace. Here a
// workgroup tile is BM x 64 with the 4 waves in 2 x 2 (wave (wm, wn): rows wm BM/2 .., columns
// wn 32 ..), so each A fragment feeds 2 MFMAs and each B fragment BM/32: 0.75 KiB per MFMA at
// BM = 128. Per 128-k step the workgroup loads x [BM][128 B] and W [64][128 B] in full 128-B
// lines (8 threads per row) D steps ahead into registers, then stores them to a double-buffered
// LDS image whose 16-B chunks are XOR-swizzled by (row >> 1) & 7: the 16 lanes of each
// ds_write_b128 / ds_read_b128 pass (two rows x 8 chunks; 16 consecutive rows at one chunk) hit
// 16 distinct bank groups. One barrier per step. K is split across workgroups with the same
// fence-free slab hand-off as gemm_mfma_kernel; the epilogue is Int8Dyn's (bit-exact).
#include "tao_gemm.h"
#include "tao_mfma.h"

namespace tao {
namespace {

__device__ __forceinline__ int i8_swz(int row, int c) { return row * 8 + (c ^ ((row >> 1) & 7)); }

template <int BM, int D, int BN = 64>
__global__ __launch_bounds__(256) void gemm_i8_lds_kernel(
    const int8_t* __restrict__ x, const int8_t* __restrict__ w, const uint16_t* __restrict__ xscale,
    const uint16_t* __restrict__ wscale, const uint16_t* __restrict__ bias,
    uint16_t* __restrict__ y, int M, int N, int K, int sps, i32x4_t* __restrict__ slab,
    unsigned* __restrict__ cnt, int fenced, int order, int cs) {
  constexpr int XL = BM / 32;           // x chunks per thread per step
  constexpr int WL = BN / 32;           // W chunks per thread per step (BN rows x 8 chunks)
  constexpr int MT = BM / 32, NT = BN / 32;  // 16x16 output tiles per wave
  constexpr int XT = BM * 8, WT = BN * 8;    // uint4 per image
  __shared__ uint4 lds[2 * (XT + WT)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const TileId tid3 = xcd_tile(order);
  const int n_blk = tid3.n * BN, m_blk = tid3.m * BM;
  const int nsteps = K / kI8Step;
  const int s0 = tid3.z * sps;
  const int s1 = s0 + sps < nsteps ? s0 + sps : nsteps;  // launcher: no empty slice
  const int J = s1 - s0;

  // load slots: row lr + 32 i, 16-B chunk lc; rows past M / N clamped (computed, dropped)
  const int lr = tid >> 3, lc = tid & 7;
  const Rsrc xrs = make_rsrc(x, (uint32_t)M * (uint32_t)K);
  const Rsrc wrs = make_rsrc(w, (uint32_t)N * (uint32_t)K);
  uint32_t xv[XL], wv[WL];
  int xo[XL], wo[WL];
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    const int r = lr + 32 * i, gm = m_blk + r < M ? m_blk + r : M - 1;
    xv[i] = (uint32_t)gm * (uint32_t)K + 16 * lc;
    xo[i] = i8_swz(r, lc);
  }
#pragma unroll
  for (int i = 0; i < WL; ++i) {
    const int r = lr + 32 * i, gn = n_blk + r < N ? n_blk + r : N - 1;
    wv[i] = (uint32_t)gn * (uint32_t)K + 16 * lc;
    wo[i] = XT + i8_swz(r, lc);
  }

  i32x4_t acc[MT][NT];
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = i32x4_t{0, 0, 0, 0};

  // Epilogue operands loaded up front (gemm_mfma_kernel's reason): the x scales of this lane's
  // 4 rows per M tile as bf16 pairs (rows clamped), the w scale and bias of its NT columns.
  uint2 xsf[MT];
  float wsf[NT], bsf[NT];
  {
    const int q = (lane >> 4) & 3, c16 = lane & 15;
#pragma unroll
    for (int a = 0; a < MT; ++a) {
      uint32_t hh[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m_blk + wm * (BM / 2) + a * 16 + 4 * q + i;
        hh[i] = xscale[m < M ? m : M - 1];
      }
      xsf[a] = make_uint2(hh[0] | (hh[1] << 16), hh[2] | (hh[3] << 16));
    }
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      const int n = n_blk + wn * (BN / 2) + b * 16 + c16;
      const int nn = n < N ? n : N - 1;
      wsf[b] = bf16_to_f32(wscale[nn]);
      bsf[b] = bias != nullptr ? bf16_to_f32(bias[nn]) : 0.f;
    }
  }

  uint4 xr[D][XL], wr[D][WL];
  auto load_step = [&](int j, uint4 (&xd)[XL], uint4 (&wd)[WL]) __attribute__((always_inline)) {
    const int st = s0 + j < s1 ? s0 + j : s1 - 1;  // past the slice: re-read (never predicated)
#pragma unroll
    for (int i = 0; i < XL; ++i) xd[i] = bload16(xrs, xv[i], st * kI8Step);
#pragma unroll
    for (int i = 0; i < WL; ++i) wd[i] = bload16<kNT>(wrs, wv[i], st * kI8Step);
  };
  auto store_step = [&](const uint4 (&xd)[XL], const uint4 (&wd)[WL], int buf)
      __attribute__((always_inline)) {
    uint4* img = lds + buf * (XT + WT);
#pragma unroll
    for (int i = 0; i < XL; ++i) img[xo[i]] = xd[i];
#pragma unroll
    for (int i = 0; i < WL; ++i) img[wo[i]] = wd[i];
  };
  const int fr = lane & 15, kq = lane >> 4;
  auto compute = [&](int buf) __attribute__((always_inline)) {
    const uint4* img = lds + buf * (XT + WT);
#pragma unroll
    for (int b = 0; b < 2; ++b) {  // two 64-k blocks per step: chunks 4 b + kq
      const int c = 4 * b + kq;
      i32x4_t bf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        bf[nt] = __builtin_bit_cast(i32x4_t, img[XT + i8_swz(wn * (BN / 2) + nt * 16 + fr, c)]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const i32x4_t af =
            __builtin_bit_cast(i32x4_t, img[i8_swz(wm * (BM / 2) + mt * 16 + fr, c)]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[nt], acc[mt][nt], 0, 0, 0);
      }
    }
  };
  // slot u holds local step j (j % D == u, compile-time); its registers are free once stored
  auto body = [&](auto uc, int j) __attribute__((always_inline)) {
    constexpr int u = decltype(uc)::value;
    load_step(j + D, xr[u], wr[u]);
    compute(j & 1);
    if (j + 1 < J) store_step(xr[(u + 1) % D], wr[(u + 1) % D], (j + 1) & 1);
    __syncthreads();
  };
  static_for<0, D>([&](auto i) __attribute__((always_inline)) {
    load_step(decltype(i)::value, xr[decltype(i)::value], wr[decltype(i)::value]);
  });
  store_step(xr[0], wr[0], 0);
  __syncthreads();
  int j = 0;
  for (; j + D <= J; j += D)
    static_for<0, D>([&](auto uc) __attribute__((always_inline)) {
      body(uc, j + decltype(uc)::value);
    });
  static_for<0, D - 1>([&](auto uc) __attribute__((always_inline)) {
    if (j + decltype(uc)::value < J) body(uc, j + decltype(uc)::value);
  });

  const int S = gridDim.z;
  if (S > 1) {  // slab hand-off as in gemm_mfma_kernel (last_arriver, tao_common.h)
    const unsigned tile = tid3.m * gridDim.x + tid3.n;
    constexpr uint32_t kZ = 4 * MT * NT * 64 * sizeof(i32x4_t);  // one slice's slab
    const Rsrc srs = make_rsrc(reinterpret_cast<const uint8_t*>(slab) + (size_t)tile * S * kZ,
                               (uint32_t)(S * kZ));
    const uint32_t lo = (uint32_t)((wave * MT * NT * 64 + lane) * sizeof(i32x4_t));
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int b = 0; b < NT; ++b)
        bstore16<kSC1>(srs, lo + (a * NT + b) * 64 * sizeof(i32x4_t), tid3.z * kZ,
                       __builtin_bit_cast(uint4, acc[a][b]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!last_arriver(&cnt[tile * cs], (unsigned)S, reinterpret_cast<unsigned*>(lds), fenced)) return;
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int b = 0; b < NT; ++b) acc[a][b] = i32x4_t{0, 0, 0, 0};
    for (int z = 0; z < S; ++z) {  // slice order
      i32x4_t part[MT][NT];
#pragma unroll
      for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
          part[a][b] = __builtin_bit_cast(
              i32x4_t, bload16<kSC1>(srs, lo + (a * NT + b) * 64 * sizeof(i32x4_t), z * kZ));
#pragma unroll
      for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] += part[a][b];
    }
  }

  // C/D map: col = lane & 15 (n), row = 4 (lane >> 4) + i (m); Int8Dyn's epilogue
#pragma unroll
  for (int b = 0; b < NT; ++b) {
    const int n = n_blk + wn * (BN / 2) + b * 16 + fr;
    if (n >= N) continue;
    const float sw = wsf[b];
    const float bv = bsf[b];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m_blk + wm * (BM / 2) + a * 16 + 4 * kq + i;
        if (m < M) {
          const uint32_t xw = (i < 2) ? xsf[a].x : xsf[a].y;
          const float xsc = (i & 1) ? bf16hi_to_f32(xw) : bf16lo_to_f32(xw);
          float v = round_bf16(round_bf16((float)acc[a][b][i]) * xsc);
          v = round_bf16(v * sw);
          if (bias != nullptr) v = round_bf16(v + bv);
          y[(size_t)m * N + n] = f32_to_bf16(v);
        }
      }
  }
}

}  // namespace

// register-ring depth: tao_tune_gemm_depth (0 = built-in 3 / 4); column tile: tao_tune_gemm_bn
// (0 = built-in 64, or 128)
int launch_i8_lds(const int8_t* xq, const uint16_t* xs, const int8_t* wq, const uint16_t* ws,
                  const uint16_t* bias, uint16_t* y, int M, int N, int K, bool auto_mode,
                  hipStream_t stream) {
  const int nsteps = K / kI8Step;
  // auto: 128-column tiles once 128 x 128 tiles alone number >= 256 (M >= 256;
  // profiles/r1_sweep_i8_bn.jsonl: M=512 14336x4096 54.6 vs 70.6 us; no gain at M = 128)
  const int tbn = tao::tuning().i8_bn;
  const int bn = tbn ? (tbn == 128 ? 128 : 64)
                     : (auto_mode && M >= 256 &&
                                (long)((N + 127) / 128) * ((M + 127) / 128) >= 256
                            ? 128
                            : 64);
  const long ntile = (N + bn - 1) / bn;
  // auto (profiles/r1_sweep_i8_lds.jsonl): the M = 128 tile once it alone fills a round of
  // workgroups, else 64; no split (every winning LDS shape ran unsplit). Forced (algo 2, the
  // parity tests' mode): split towards one round, slices of >= 4 steps (512 k).
  int bm = auto_mode ? (bn == 128 || ntile * ((M + 127) / 128) >= 224 ? 128 : 64)
                     : (M > 64 ? 128 : 64);
  const int tb = tao::tuning().bm;
  if (tb == 64 || tb == 128) bm = tb;
  const long tiles = ntile * ((M + bm - 1) / bm);
  int splits = 1;
  while (!auto_mode && tiles * splits < 224 && splits * 2 <= 16 && nsteps >= 4 * splits * 2)
    splits *= 2;
  const int ts = tao::tuning().splits;
  if (ts) splits = ts < nsteps ? ts : nsteps;
  const int sps = (nsteps + splits - 1) / splits;
  const int S = (nsteps + sps - 1) / sps;
  const dim3 grid((N + bn - 1) / bn, (M + bm - 1) / bm, S);
  i32x4_t* slab = nullptr;
  unsigned* cnt = nullptr;
  if (S > 1) {
    void* wsp = nullptr;
    const size_t t = (size_t)grid.x * grid.y;
    const int rc = split_workspace(stream, t * S * bm * bn * sizeof(int), t * tuning().cnt_stride,
                                   &wsp, &cnt);
    if (rc != TAO_OK) return rc;
    slab = reinterpret_cast<i32x4_t*>(wsp);
  }
  const int td = tao::tuning().i8_depth;
  const int d = td ? td : (bm == 128 ? 3 : 4);
  auto go = [&](auto kern) {
    launch(kern, grid, dim3(256), 0, stream, xq, wq, xs, ws, bias, y, M, N, K, sps, slab, cnt,
           tuning().splitk_fenced, tuning().gemm_order, tuning().cnt_stride);
  };
  if (bn == 128) {  // experiment (tao_tune_gemm_bn): ring depth 2 or 3
    if (bm == 128) {
      if (d == 2) go(gemm_i8_lds_kernel<128, 2, 128>);
      else go(gemm_i8_lds_kernel<128, 3, 128>);
    } else {
      if (d == 2) go(gemm_i8_lds_kernel<64, 2, 128>);
      else go(gemm_i8_lds_kernel<64, 3, 128>);
    }
  } else if (bm == 128) {
    if (d == 2) go(gemm_i8_lds_kernel<128, 2>);
    else if (d == 3) go(gemm_i8_lds_kernel<128, 3>);
    else if (d == 4) go(gemm_i8_lds_kernel<128, 4>);
    else go(gemm_i8_lds_kernel<128, 6>);
  } else {
    if (d == 2) go(gemm_i8_lds_kernel<64, 2>);
    else if (d == 3) go(gemm_i8_lds_kernel<64, 3>);
    else if (d == 4) go(gemm_i8_lds_kernel<64, 4>);
    else if (d == 6) go(gemm_i8_lds_kernel<64, 6>);
    else go(gemm_i8_lds_kernel<64, 8>);
  }
  return check_launch("gemm_i8_lds_kernel");
}

}  // namespace tao

extern "C" int tao_tune_gemm_bn(int bn) {
  TAO_CHECK_ARG(bn == 0 || bn == 64 || bn == 128, "tune: LDS int8 GEMM bn must be 0, 64 or 128");
  tao::tuning().i8_bn = bn;
  return TAO_OK;
}

extern "C" int tao_tune_gemm_depth(int depth) {
  TAO_CHECK_ARG(depth == 0 || depth == 2 || depth == 3 || depth == 4 || depth == 6 || depth == 8,
                "tune: LDS int8 GEMM depth must be 0 (built-in), 2, 3, 4, 6 or 8 (8: M tile 64)");
  tao::tuning().i8_depth = depth;
  return TAO_OK;
}
