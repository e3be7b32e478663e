// One-MFMA probe of v_mfma_scale_f32_16x16x128_f8f6f4 with A = e4m3 (cbsz 0) and B = e2m1
// (blgp 4): which A byte each B nibble is multiplied with, and which lane's scale byte scales it.
//
//   hipcc --offload-arch=gfx950 -O2 experiments/probe_fp4_layout.hip -o experiments/build/probe_fp4_layout
//
// A positions are numbered a = 32 g + 4 v + b (lane group g = lane >> 4, operand VGPR v of 8, byte
// b); row i (< 7) of A holds 1.0 where bit i of a is set, so one-hot B data reads a back from the
// output column. B positions are (lane group g, VGPR d of 4, nibble p of 8, p = 0 the lowest).
// Pass 0: B one-hot (code 2 = 1.0) at one position in every column, scales 2^0: C[i][n] = bit i
// of the partner a. Pass 1: A all 1.0, lane group g supplies B scale byte 127 + g: C = 2^(group
// whose byte scaled that nibble). Pass 2: the same for A's scale with A one-hot at the partner.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__global__ void probe(float* out) {  // [128 positions][2 passes][64 lanes][4]
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
  i32x8_t abits, aones;
  for (int v = 0; v < 8; ++v) {
    unsigned w = 0;
    for (int b = 0; b < 4; ++b) {
      const int a = 32 * g + 4 * v + b;
      if (i < 7 && ((a >> i) & 1)) w |= 0x38u << (8 * b);
    }
    abits[v] = (int)w;
    aones[v] = 0x38383838;
  }
  for (int pos = 0; pos < 128; ++pos) {
    const int gb = pos >> 5, d = (pos >> 3) & 3, p = pos & 7;
    i32x8_t b = {0, 0, 0, 0, 0, 0, 0, 0};
    if (g == gb) b[d] = (int)(2u << (4 * p));
    const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
    const f32x4_t c0 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(abits, b, z, 0, 4, 0,
                                                                         0x7F7F7F7F, 0, 0x7F7F7F7F);
    const f32x4_t c1 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aones, b, z, 0, 4, 0,
                                                                         0x7F7F7F7F, 0, 127 + g);
    for (int r = 0; r < 4; ++r) {
      out[((pos * 2 + 0) * 64 + lane) * 4 + r] = c0[r];
      out[((pos * 2 + 1) * 64 + lane) * 4 + r] = c1[r];
    }
  }
}

#define CK(x)                                                        \
  do {                                                               \
    hipError_t e_ = (x);                                             \
    if (e_ != hipSuccess) {                                          \
      std::printf("%s: %s\n", #x, hipGetErrorString(e_));           \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main() {
  const size_t n = 128 * 2 * 64 * 4;
  float* d = nullptr;
  CK(hipMalloc(&d, n * sizeof(float)));
  CK(hipMemset(d, 0, n * sizeof(float)));
  probe<<<1, 64>>>(d);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<float> h(n);
  CK(hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
  // C[row][col]: lane l holds rows 4 (l >> 4) .. + 4 of column l & 15
  auto C = [&](int pos, int pass, int row, int col) {
    return h[((pos * 2 + pass) * 64 + (16 * (row >> 2) + col)) * 4 + (row & 3)];
  };
  int bad = 0;
  std::printf("B (g d p) -> A (g v b)  [k_A if A is 16 g + 4 v + b (v < 4), 64 + 16 g + 4 (v - 4) + b]"
              "  scale of lane group\n");
  for (int pos = 0; pos < 128; ++pos) {
    int a = 0, ok = 1;
    for (int i = 0; i < 16; ++i) {
      const float v = C(pos, 0, i, 0);
      if (v != 0.f && v != 1.f) ok = 0;
      if (i >= 7 && v != 0.f) ok = 0;
      if (v == 1.f) a |= 1 << i;
      for (int col = 1; col < 16; ++col)
        if (C(pos, 0, i, col) != v) ok = 0;
    }
    const float s = C(pos, 1, 0, 0);
    const int ag = a >> 5, av = (a >> 2) & 7, ab = a & 3;
    const int ka = av < 4 ? 16 * ag + 4 * av + ab : 64 + 16 * ag + 4 * (av - 4) + ab;
    std::printf("%d %d %d -> %d %d %d  k %3d  scale 2^%g%s\n", pos >> 5, (pos >> 3) & 3, pos & 7, ag,
                av, ab, ka, std::log2(s), ok ? "" : "  INCONSISTENT");
    bad += !ok;
  }
  std::printf("probe_fp4_layout: %s\n", bad ? "INCONSISTENT" : "ok");
  CK(hipFree(d));
  return bad != 0;
}
