// One-instruction probe of v_smfmac_i32_16x16x128_i8 (cbsz = abid = 0): which byte of the dense B
// operand each compressed A byte is multiplied with, and which two bits of the index register
// choose it.
//
//   hipcc --offload-arch=gfx950 -O2 experiments/probe_smfmac_layout.hip -o experiments/build/probe_smfmac_layout
//
// A (compressed, 4 VGPRs): lane (i = lane & 15, g = lane >> 4) holds 16 bytes of row i. B (dense,
// 8 VGPRs): lane (n = lane & 15, gb = lane >> 4) holds 32 bytes of column n. B byte j of lane
// group gb carries bit n of its own position 32 gb + j, so one-hot A data reads the partner's
// position back from the output columns. Pass 0, for every (g, A byte b, index field f, code p):
// A = 1 at byte b of the lanes of group g, index = p << 2f in every lane. The field whose code
// moves the partner is byte b's field, and the partner as a function of p is the position code.
// Pass 1: A = row number + 1 at (g 0, byte 0), B all ones: C[i][n] = i + 1 checks that output row i
// is A lane i and that a lane holds rows 4 (lane >> 4) .. + 3 of column lane & 15.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));

constexpr int kProbes = 4 * 16 * 16 * 4;

__global__ void probe(int* out) {  // [kProbes + 1][64 lanes][4]
  const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
  i32x8_t bpos, bones;
  for (int v = 0; v < 8; ++v) {
    unsigned w = 0;
    for (int b = 0; b < 4; ++b) {
      const int pos = 32 * g + 4 * v + b;
      if (n < 7 && ((pos >> n) & 1)) w |= 1u << (8 * b);
    }
    bpos[v] = (int)w;
    bones[v] = 0x01010101;
  }
  const i32x4_t z = {0, 0, 0, 0};
  for (int pr = 0; pr < kProbes; ++pr) {
    const int ga = pr >> 10, b = (pr >> 6) & 15, f = (pr >> 2) & 15, p = pr & 3;
    i32x4_t a = {0, 0, 0, 0};
    if (g == ga) a[b >> 2] = 1 << (8 * (b & 3));
    const i32x4_t c = __builtin_amdgcn_smfmac_i32_16x16x128_i8(a, bpos, z, p << (2 * f), 0, 0);
    for (int r = 0; r < 4; ++r) out[(pr * 64 + lane) * 4 + r] = c[r];
  }
  i32x4_t a = {0, 0, 0, 0};
  if (g == 0) a[0] = n + 1;
  const i32x4_t c = __builtin_amdgcn_smfmac_i32_16x16x128_i8(a, bones, z, 0, 0, 0);
  for (int r = 0; r < 4; ++r) out[(kProbes * 64 + lane) * 4 + r] = c[r];
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
  const size_t n = (size_t)(kProbes + 1) * 64 * 4;
  int* d = nullptr;
  CK(hipMalloc(&d, n * sizeof(int)));
  CK(hipMemset(d, 0, n * sizeof(int)));
  probe<<<1, 64>>>(d);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<int> h(n);
  CK(hipMemcpy(h.data(), d, n * sizeof(int), hipMemcpyDeviceToHost));
  // C[row][col]: lane l holds rows 4 (l >> 4) .. + 3 of column l & 15 (checked by pass 1)
  auto C = [&](int pr, int row, int col) {
    return h[((size_t)pr * 64 + (16 * (row >> 2) + col)) * 4 + (row & 3)];
  };
  int bad = 0;
  // partner position of a probe: bits read from columns 0-6 of row 0; every row must agree
  auto partner = [&](int pr) {
    int pos = 0;
    for (int col = 0; col < 16; ++col) {
      const int v = C(pr, 0, col);
      if ((v != 0 && v != 1) || (col >= 7 && v != 0)) bad++;
      if (v == 1) pos |= 1 << col;
      for (int row = 1; row < 16; ++row)
        if (C(pr, row, col) != v) bad++;
    }
    return pos;
  };
  std::printf("A (g b) -> index bits [hi:lo], B position (lane group, byte) for code 0 1 2 3\n");
  for (int ga = 0; ga < 4; ++ga)
    for (int b = 0; b < 16; ++b) {
      int field = -1, pos[4] = {0, 0, 0, 0};
      for (int f = 0; f < 16; ++f) {
        int q[4];
        for (int p = 0; p < 4; ++p) q[p] = partner(((ga * 16 + b) * 16 + f) * 4 + p);
        if (q[1] != q[0] || q[2] != q[0] || q[3] != q[0]) {
          if (field >= 0) bad++;  // two fields move this byte's partner
          field = f;
          for (int p = 0; p < 4; ++p) pos[p] = q[p];
        }
      }
      if (field < 0) bad++;
      std::printf("%d %2d -> [%2d:%2d]  (%d,%2d) (%d,%2d) (%d,%2d) (%d,%2d)\n", ga, b, 2 * field + 1,
                  2 * field, pos[0] >> 5, pos[0] & 31, pos[1] >> 5, pos[1] & 31, pos[2] >> 5,
                  pos[2] & 31, pos[3] >> 5, pos[3] & 31);
    }
  int rows_ok = 1;
  for (int row = 0; row < 16; ++row)
    for (int col = 0; col < 16; ++col)
      if (C(kProbes, row, col) != row + 1) rows_ok = 0;
  std::printf("output row i = A lane i, lane l holds rows 4 (l >> 4) .. + 3 of column l & 15: %s\n",
              rows_ok ? "yes" : "NO");
  bad += !rows_ok;
  std::printf("probe_smfmac_layout: %s\n", bad ? "INCONSISTENT" : "ok");
  CK(hipFree(d));
  return bad != 0;
}
