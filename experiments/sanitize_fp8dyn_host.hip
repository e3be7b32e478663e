// Stand-alone host program for the sanitizers: runs the host-side arithmetic of the float8
// dynamic-activation linear (csrc/fp8_dyn_host.h: GEMV launch shape, fused-prologue sizing, route
// choice; with a chunk width and token-scale bytes, the launch shape of all four formats of
// csrc/scaled_gemv.h) over a sweep of arguments and checks the invariants the kernels rely on.
// No GPU call.
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=all -I torchao-fork_amd/csrc \
//     -fsanitize=address,undefined experiments/sanitize_fp8dyn_host.hip \
//     -o sanitize_fp8dyn_host && ./sanitize_fp8dyn_host
// (the unprefixed flag links the host runtimes; the device side ignores it with a warning)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fp8_dyn_host.h"

namespace tao {  // what the internal headers expect from capi.cpp
int set_error(int code, const char*, ...) { return code; }
}  // namespace tao

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);               \
      return 1;                                                          \
    }                                                                    \
  } while (0)

// The formats of scaled_gemv.h as its launcher describes them to fp8dyn_launch_shape: the k in a
// 16-B weight chunk, the k in a scale block and the bytes of one stored token scale (per-row
// scales: none kept in LDS).
struct Fmt {
  int chunk_k, block_k, scale_size;
};
static const Fmt kFmt[4] = {
    {16, 16, 0},   // fp8dyn: per-row scales
    {16, 32, 1},   // mx: an E8M0 byte per 32 k
    {32, 32, 1},   // mxfp4w: the same, e2m1 weight chunks of 32 k
    {16, 128, 4},  // blockfp8: an fp32 per 128 k
};

// The expectation: what each format's own launcher computed before the four kernels became one,
// restated from those sources. fp8dyn, mx and blockfp8 called the 16-k launch shape and mx /
// blockfp8 added their scale bytes to its lds; mxfp4w re-derived the whole shape for 32-k chunks.
struct OldShape {
  int S, Wk, G, grid, threads, per;
  size_t lds;
};
static OldShape old_shape(int f, int N, int K, int rpw, int mt, int wk, int g, bool fq) {
  const int nchunk = f == 2 ? K / 32 : K / 16;
  OldShape o{(nchunk + 63) / 64, 0, g, 0, 0, 0, 0};
  o.Wk = wk < o.S ? wk : o.S;
  while (o.G > 1 && o.Wk * o.G > 8) o.G >>= 1;
  while (fq && (int64_t)64 * o.Wk * o.G * 8 * 16 < K && o.Wk * o.G * 2 <= 8) o.G *= 2;
  const int rows_per_wg = o.G * rpw;
  o.grid = (int)(((int64_t)N + rows_per_wg - 1) / rows_per_wg);
  const int nw = o.G * o.Wk;
  o.threads = 64 * nw;
  o.lds = (size_t)nw * rpw * mt * sizeof(float);
  if (fq) {
    o.lds = (((size_t)nw * rpw * mt + 8 + 3) & ~(size_t)3) * sizeof(float) + (size_t)K;
    if (f == 1 || f == 2) o.lds += (size_t)((K / 32 + 15) & ~15);
    if (f == 3) o.lds += (size_t)((K / 128 * 4 + 15) & ~15);
    o.per = (K / 8 + o.threads - 1) / o.threads;
  }
  return o;
}

int main() {
  using namespace tao;
  long cases = 0;
  const int Ks[] = {16, 112, 1024, 1040, 4096, 4112, 14336, 32768, 65536};
  const int Ns[] = {1, 37, 4096, 128256, 2147483647};
  const int shapes[][3] = {{4, 8, 1}, {8, 4, 2}, {2, 1, 1}, {4, 2, 4}, {8, 8, 1}, {4, 8, 8}, {2, 3, 2}};
  for (int K : Ks)
    for (int N : Ns)
      for (const auto& s : shapes)
        for (int fq = 0; fq < 2; ++fq)
          for (int mt : {1, 2, 4, 8}) {
            if (fq && mt != 1) continue;
            const int rpw = fq ? s[0] : 8 / mt > s[0] ? s[0] : 8 / mt;
            const Fp8DynLaunch L = fp8dyn_launch_shape(N, K, rpw, mt, s[1], s[2], fq != 0);
            ++cases;
            CHECK(L.Wk >= 1 && L.G >= 1 && L.Wk * L.G <= 8 && L.threads == 64 * L.Wk * L.G);
            CHECK(L.S == (K / 16 + 63) / 64 && L.Wk <= L.S);
            CHECK((long long)L.grid * L.G * rpw >= N && (long long)(L.grid - 1) * L.G * rpw < N);
            if (fq) {
              CHECK(L.per >= 1 && (long long)L.per * L.threads * 8 >= K);
              // the kernel's LDS carve-up: partials, 8 wave maxima, then K code bytes, 16-B aligned
              std::vector<unsigned char> lds(L.lds);
              const size_t off = (((size_t)L.Wk * L.G * rpw * mt + 8 + 3) & ~(size_t)3) * 4;
              CHECK(off % 16 == 0 && off + (size_t)K == L.lds);
              lds[off + K - 1] = 1;  // the last code byte is inside the allocation
              if (K <= 65536 && L.threads == 512) CHECK(L.per <= 16);
            }
          }
  // the decode kernel's launches (tao_fp8dq_decode_bf16): at most 8 token pieces per thread, 4
  // with the RMSNorm; row groups are added up to 8 waves before a K is refused
  for (int K : Ks)
    for (int N : Ns)
      for (const auto& s : shapes)
        for (int max_per : {4, 8}) {
          const int rpw = s[0];
          const Fp8DynLaunch L = fp8dyn_launch_shape(N, K, rpw, 1, s[1], s[2], true, max_per);
          const Fp8DynLaunch L16 = fp8dyn_launch_shape(N, K, rpw, 1, s[1], s[2], true);
          ++cases;
          CHECK(L.Wk >= 1 && L.G >= 1 && L.Wk * L.G <= 8 && L.threads == 64 * L.Wk * L.G);
          CHECK(L.S == (K / 16 + 63) / 64 && L.Wk == L16.Wk && L.G >= L16.G);
          CHECK((long long)L.grid * L.G * rpw >= N && (long long)(L.grid - 1) * L.G * rpw < N);
          CHECK(L.per >= 1 && (long long)L.per * L.threads * 8 >= K);
          // a thread holds more than max_per pieces only where no further row group fits
          if (L.per > max_per) CHECK(L.Wk * L.G * 2 > 8);
          // the entry's K limits are served by the built-in shape (8 rows, 4 waves, 2 groups)
          if (s[0] == 8 && s[1] == 4 && s[2] == 2 && K <= 4096 * max_per) CHECK(L.per <= max_per);
          std::vector<unsigned char> lds(L.lds);
          const size_t off = (((size_t)L.Wk * L.G * rpw + 8 + 3) & ~(size_t)3) * 4;
          CHECK(off % 16 == 0 && off + (size_t)K == L.lds);
          lds[off + K - 1] = 1;
        }
  // scaled_gemv.h's one host path: for every format, grid / threads / lds / per (and S, Wk, G)
  // equal what that format's own launcher computed before the kernels were merged (old_shape)
  const int fKs[] = {32, 128, 1024, 1056, 1152, 4096, 4224, 14336, 32768, 65536};
  for (int f = 0; f < 4; ++f)
    for (int K : fKs)
      for (int N : Ns)
        for (const auto& s : shapes)
          for (int fq = 0; fq < 2; ++fq)
            for (int mt : {1, 2, 4, 8}) {
              if (K % kFmt[f].block_k != 0 || (fq && mt != 1)) continue;
              const int rpw = fq ? s[0] : 8 / mt > s[0] ? s[0] : 8 / mt;
              const int sb = K / kFmt[f].block_k * kFmt[f].scale_size;
              const Fp8DynLaunch L = fp8dyn_launch_shape(N, K, rpw, mt, s[1], s[2], fq != 0, 16,
                                                         kFmt[f].chunk_k, sb);
              const OldShape o = old_shape(f, N, K, rpw, mt, s[1], s[2], fq != 0);
              ++cases;
              CHECK(L.S == o.S && L.Wk == o.Wk && L.G == o.G);
              CHECK(L.grid == o.grid && L.threads == o.threads && L.lds == o.lds);
              if (fq) {
                CHECK(L.per == o.per);
                // the kernel's carve-up: the scales start right behind the K code bytes
                std::vector<unsigned char> lds(L.lds);
                const size_t off = (((size_t)L.Wk * L.G * rpw * mt + 8 + 3) & ~(size_t)3) * 4;
                CHECK(off + (size_t)K + (size_t)sb <= L.lds);
                lds[off + K + sb - 1] = 1;  // the last scale byte (or code byte) is inside
              }
            }
  for (long long M : {0LL, 1LL, 2LL, 4LL, 5LL, 8LL, 9LL, 2147483647LL})
    for (long long N : {1LL, 4096LL, 14336LL, 2147483647LL})
      for (long long K : {16LL, 4096LL, 14336LL, 268435456LL})
        for (int mf = 0; mf < 2; ++mf)
          for (int v = 0; v <= 8; ++v) {
            if (N * K >= (1LL << 32)) continue;  // refused by the entry before the route is chosen
            const bool g = fp8dyn_route_gemv(M, N, K, mf, v);
            ++cases;
            if (mf) CHECK(!g);
            if (!mf && v > 0) CHECK(g == (M <= v));
            if (g) CHECK(M <= 8);  // the GEMV's widest instantiation holds 8 tokens
          }
  std::printf("fp8dyn host helpers: %ld cases clean\n", cases);
  return 0;
}
