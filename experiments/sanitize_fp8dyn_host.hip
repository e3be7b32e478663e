// Stand-alone host program for the sanitizers: runs the host-side arithmetic of the float8
// dynamic-activation linear (csrc/fp8_dyn_host.h: GEMV launch shape, fused-prologue sizing, route
// choice) over a sweep of arguments and checks the invariants the kernel relies on. No GPU call.
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
