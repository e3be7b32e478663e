// Stand-alone host program for the sanitizers: runs the host-side arithmetic of the NF4 linear
// (csrc/nf4_host.h: the route rule, the GEMV's tile choice, the factor count) over a sweep of
// arguments and checks the invariants nf4.hip and torch_ops.cpp rely on. No GPU call.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//     -I torchao-fork_amd/csrc experiments/sanitize_nf4_host.cpp -o sanitize_nf4_host \
//     && ./sanitize_nf4_host
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "nf4_host.h"

#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);  \
      return 1;                                             \
    }                                                       \
  } while (0)

int main() {
  using namespace tao;
  long cases = 0;
  const int64_t Ns[] = {1, 37, 4096, 14336, (1LL << 31) - 1};
  const int64_t Ks[] = {64, 1088, 4096, 14336, ((1LL << 31) - 1) / 64 * 64};
  for (int64_t N : Ns)
    for (int64_t K : Ks) {
      for (int64_t M = 0; M <= 4200; M = M < 40 ? M + 1 : M * 2 + 1) {
        for (int force = 0; force <= 2; ++force)
          for (int lim : {0, 1, 2, 8, 64}) {
            const int r = nf4_route(M, N, K, force, lim);
            CHECK(r == kNf4RouteGemv || r == kNf4RouteDequantMm);
            if (force != kNf4RouteAuto) CHECK(r == force);
            else CHECK((r == kNf4RouteGemv) == (M <= (lim > 0 ? lim : kNf4GemvDefaultM)));
            ++cases;
          }
      }
      // every block of the weight finds its factor
      const int64_t blocks = N * K / 64;
      if (blocks > 0) CHECK(((blocks - 1) >> 8) < nf4_num_factors(N, K));
      CHECK(nf4_num_factors(N, K) * 16384 >= N * K && (nf4_num_factors(N, K) - 1) * 16384 < N * K);
    }
  for (int m = 1; m <= kNf4GemvMaxM; ++m) {
    const Nf4GemvTile t = nf4_gemv_tile(m);
    CHECK(t.mt >= m && t.mt * t.rpw == (m == 1 ? 4 : 8));
    CHECK(t.mt == 1 || t.mt == 2 || t.mt == 4 || t.mt == 8);
    ++cases;
  }
  std::printf("nf4 host arithmetic ok (%ld cases)\n", cases);
  return 0;
}
