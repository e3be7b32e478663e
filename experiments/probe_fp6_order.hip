// One-instruction probe of v_cvt_scalef32_pk32_bf16_bf6 (e3m2) and v_cvt_scalef32_pk32_bf16_fp6
// (e2m3) with scale 1.0: which bits of the six operand dwords hold which element, where that
// element's bf16 lands in the 16 result dwords, and that all 64 codes decode to the format's
// value exactly.
//
//   hipcc --offload-arch=gfx950 -O2 experiments/probe_fp6_order.hip -o experiments/build/probe_fp6_order
//
// Hypothesis under test (csrc/fp6_codec.h): element i sits at bits 6 i .. 6 i + 5 of the operand
// read as a 192-bit little-endian number, and its result is half i & 1 of result dword i >> 1.
// Pass A: for every format, position p and code c, an operand with c at p and zeros elsewhere; the
// result must be value(c) at element p and +0 elsewhere. Pass B: operands with a different code
// at every position (code (7 p + r) & 63 for r = 0 .. 63), every element checked.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef uint32_t u32x6_t __attribute__((ext_vector_type(6)));
typedef __bf16 bf16x32_t __attribute__((ext_vector_type(32)));
typedef uint32_t u32x16_t __attribute__((ext_vector_type(16)));

__device__ void put(uint32_t (&o)[6], int p, uint32_t c) {
  const int bit = 6 * p, d = bit >> 5, sh = bit & 31;
  o[d] |= c << sh;
  if (sh > 26) o[d + 1] |= c >> (32 - sh);
}

// thread t: fmt = t >> 12, pass = (t >> 11) & 1, p = (t >> 6) & 31, c = t & 63
__global__ void probe(uint32_t* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int fmt = t >> 12, pass = (t >> 11) & 1, p = (t >> 6) & 31, c = t & 63;
  uint32_t o[6] = {0, 0, 0, 0, 0, 0};
  if (pass == 0) {
    put(o, p, (uint32_t)c);
  } else {
    for (int q = 0; q < 32; ++q) put(o, q, (uint32_t)((7 * q + c + p) & 63));
  }
  const u32x6_t v = {o[0], o[1], o[2], o[3], o[4], o[5]};
  bf16x32_t r;
  if (fmt == 0) r = __builtin_amdgcn_cvt_scalef32_pk32_bf16_bf6(v, 1.0f);
  else r = __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(v, 1.0f);
  const u32x16_t d = __builtin_bit_cast(u32x16_t, r);
  for (int i = 0; i < 16; ++i) out[(size_t)t * 16 + i] = d[i];
}

#define CK(x)                                                        \
  do {                                                               \
    hipError_t e_ = (x);                                             \
    if (e_ != hipSuccess) {                                          \
      std::printf("%s: %s\n", #x, hipGetErrorString(e_));           \
      return 1;                                                      \
    }                                                                \
  } while (0)

// bf16 bits of the value of code c from the format's definition (sign, ebits exponent, mbits
// mantissa, bias 2^(ebits - 1) - 1, subnormals, no inf / NaN)
static uint16_t value_bits(int fmt, int c) {
  const int ebits = fmt == 0 ? 3 : 2, mbits = fmt == 0 ? 2 : 3, bias = (1 << (ebits - 1)) - 1;
  const int s = c >> 5, e = (c >> mbits) & ((1 << ebits) - 1), m = c & ((1 << mbits) - 1);
  const float mag = e == 0 ? std::ldexp((float)m, 1 - bias - mbits)
                           : std::ldexp(1.0f + (float)m / (float)(1 << mbits), e - bias);
  const float f = s ? -mag : mag;
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return (uint16_t)(u >> 16);  // exact: at most 4 significant bits
}

int main() {
  const int nthreads = 2 * 2 * 32 * 64;
  const size_t n = (size_t)nthreads * 16;
  uint32_t* d = nullptr;
  CK(hipMalloc(&d, n * sizeof(uint32_t)));
  CK(hipMemset(d, 0xFF, n * sizeof(uint32_t)));
  probe<<<nthreads / 256, 256>>>(d);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<uint32_t> h(n);
  CK(hipMemcpy(h.data(), d, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  auto elem = [&](int t, int i) { return (uint16_t)(h[(size_t)t * 16 + (i >> 1)] >> (16 * (i & 1))); };
  int bad = 0;
  for (int fmt = 0; fmt < 2; ++fmt) {
    const char* name = fmt == 0 ? "e3m2 (bf6)" : "e2m3 (fp6)";
    // pass A: where does position p land (read from the codes with a non-zero value), and is
    // every code's value exact there
    std::printf("%s  position -> result element:", name);
    for (int p = 0; p < 32; ++p) {
      int where = -1, ok = 1;
      for (int c = 0; c < 64; ++c) {
        const int t = (fmt << 12) | (p << 6) | c;
        const uint16_t want = value_bits(fmt, c);
        for (int i = 0; i < 32; ++i) {
          const uint16_t got = elem(t, i);
          if (got != 0) {
            if (where < 0) where = i;
            if (i != where || got != want) ok = 0;
          }
        }
        if (where >= 0 && elem(t, where) != want) ok = 0;
      }
      std::printf(" %d%s", where, ok ? "" : "!");
      bad += !ok || where != p;
    }
    std::printf("\n");
    int badb = 0;
    for (int p = 0; p < 32; ++p)
      for (int c = 0; c < 64; ++c) {
        const int t = (fmt << 12) | (1 << 11) | (p << 6) | c;
        for (int q = 0; q < 32; ++q) badb += elem(t, q) != value_bits(fmt, (7 * q + c + p) & 63);
      }
    std::printf("%s  pass B (2048 full operands, element q = bits 6 q .. 6 q + 5): %d mismatches\n",
                name, badb);
    bad += badb;
  }
  std::printf("probe_fp6_order: %s\n",
              bad ? "DIFFERS from the bit-stream hypothesis" : "ok (bit-stream order, exact values)");
  CK(hipFree(d));
  return bad != 0;
}
