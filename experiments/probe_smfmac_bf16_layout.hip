// One-instruction probe of v_smfmac_f32_16x16x64_bf16: which element of the dense B operand each
// compressed A element is multiplied with, which two bits of the index register choose it, and what
// cbsz / abid select for 16-bit sources.
//
//   hipcc --offload-arch=gfx950 -O2 experiments/probe_smfmac_bf16_layout.hip -o experiments/build/probe_smfmac_bf16_layout
//
// A (compressed, 4 VGPRs): lane (i = lane & 15, g = lane >> 4) holds 8 bf16 of row i. B (dense,
// 8 VGPRs): lane (n = lane & 15, gb = lane >> 4) holds 16 bf16 of column n. B element e of lane
// group gb is the number 1 + 16 gb + e (exact in bf16), so a one-hot A of 1.0 reads its partner's
// position back as the output value. Pass 0 (cbsz = abid = 0), for every (g, A element b, index
// field f, code p): A = 1 at element b of the lanes of group g, index = p << 2f in every lane. The
// field whose code moves the partner is element b's field, and the partner as a function of p is
// the position code. Pass 1 repeats the field search for the elements of group 0 under other
// (cbsz, abid). Pass 2: A = row number + 1 at (g 0, element 0), B all ones: C[i][n] = i + 1 checks
// that output row i is A lane i and that a lane holds rows 4 (lane >> 4) .. + 3 of column lane & 15.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16_t __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kFull = 4 * 8 * 16 * 4;  // pass 0
constexpr int kVar = 8 * 16 * 4;       // pass 1, per (cbsz, abid)
constexpr int kVariants = 5;           // (0, 1) (0, 2) (0, 3) (1, 0) (1, 1)

__device__ bf16x16_t b_positions(int g) {
  bf16x16_t b;
  for (int e = 0; e < 16; ++e) b[e] = (__bf16)(float)(1 + 16 * g + e);
  return b;
}

template <int CBSZ, int ABID>
__device__ void search(float* out, int groups) {  // [groups * kVar][64][4]
  const int lane = threadIdx.x, g = lane >> 4;
  const bf16x16_t bpos = b_positions(g);
  const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
  for (int pr = 0; pr < groups * kVar; ++pr) {
    const int ga = pr >> 9, b = (pr >> 6) & 7, f = (pr >> 2) & 15, p = pr & 3;
    bf16x8_t a;
    for (int e = 0; e < 8; ++e) a[e] = (__bf16)((g == ga && e == b) ? 1.f : 0.f);
    const f32x4_t c = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a, bpos, z, p << (2 * f), CBSZ, ABID);
    for (int r = 0; r < 4; ++r) out[((size_t)pr * 64 + lane) * 4 + r] = c[r];
  }
}

__global__ void probe(float* out) {
  search<0, 0>(out, 4);
  float* v = out + (size_t)kFull * 256;
  search<0, 1>(v, 1);
  search<0, 2>(v + (size_t)kVar * 256, 1);
  search<0, 3>(v + (size_t)2 * kVar * 256, 1);
  search<1, 0>(v + (size_t)3 * kVar * 256, 1);
  search<1, 1>(v + (size_t)4 * kVar * 256, 1);
  const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
  bf16x8_t a;
  bf16x16_t ones;
  for (int e = 0; e < 8; ++e) a[e] = (__bf16)((g == 0 && e == 0) ? (float)(n + 1) : 0.f);
  for (int e = 0; e < 16; ++e) ones[e] = (__bf16)1.f;
  const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
  const f32x4_t c = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a, ones, z, 0, 0, 0);
  float* o = v + (size_t)kVariants * kVar * 256;
  for (int r = 0; r < 4; ++r) o[lane * 4 + r] = c[r];
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
  const size_t nprobes = (size_t)kFull + (size_t)kVariants * kVar + 1;
  const size_t n = nprobes * 64 * 4;
  float* d = nullptr;
  CK(hipMalloc(&d, n * sizeof(float)));
  CK(hipMemset(d, 0, n * sizeof(float)));
  probe<<<1, 64>>>(d);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<float> h(n);
  CK(hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
  int bad = 0;
  // partner of a probe: 1 + 16 gb + e in every output element (0: no partner); -1: they disagree
  auto partner = [&](size_t pr) {
    const float v = h[pr * 256];
    for (int i = 1; i < 256; ++i)
      if (h[pr * 256 + i] != v) return -1;
    return (int)v;
  };
  // of the 16 fields, the one whose code moves the partner of probes base + f * 4 + p
  auto report = [&](size_t base, bool strict) {
    int field = -1, pos[4] = {0, 0, 0, 0};
    for (int f = 0; f < 16; ++f) {
      int q[4];
      for (int p = 0; p < 4; ++p) q[p] = partner(base + f * 4 + p);
      if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0) bad++;
      if (q[1] != q[0] || q[2] != q[0] || q[3] != q[0]) {
        if (field >= 0) bad++;  // two fields move this element's partner
        field = f;
        for (int p = 0; p < 4; ++p) pos[p] = q[p] - 1;
      }
    }
    if (field < 0) {
      if (strict) bad++;
      std::printf("no field moves the partner (code 0 partner value %d)\n", partner(base));
      return;
    }
    std::printf("[%2d:%2d]  (%d,%2d) (%d,%2d) (%d,%2d) (%d,%2d)\n", 2 * field + 1, 2 * field,
                pos[0] >> 4, pos[0] & 15, pos[1] >> 4, pos[1] & 15, pos[2] >> 4, pos[2] & 15,
                pos[3] >> 4, pos[3] & 15);
  };
  std::printf("cbsz 0 abid 0: A (g b) -> index bits [hi:lo], B position (lane group, element) for code 0 1 2 3\n");
  for (int ga = 0; ga < 4; ++ga)
    for (int b = 0; b < 8; ++b) {
      std::printf("%d %d -> ", ga, b);
      report(((size_t)(ga * 8 + b) * 16) * 4, true);
    }
  const int var[kVariants][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 0}, {1, 1}};
  for (int v = 0; v < kVariants; ++v) {
    std::printf("cbsz %d abid %d, A group 0:\n", var[v][0], var[v][1]);
    for (int b = 0; b < 8; ++b) {
      std::printf("0 %d -> ", b);
      report((size_t)kFull + (size_t)v * kVar + (size_t)b * 64, false);
    }
  }
  const float* o = h.data() + ((size_t)kFull + (size_t)kVariants * kVar) * 256;
  int rows_ok = 1;
  for (int row = 0; row < 16; ++row)
    for (int col = 0; col < 16; ++col)
      if (o[(16 * (row >> 2) + col) * 4 + (row & 3)] != (float)(row + 1)) rows_ok = 0;
  std::printf("output row i = A lane i, lane l holds rows 4 (l >> 4) .. + 3 of column l & 15: %s\n",
              rows_ok ? "yes" : "NO");
  bad += !rows_ok;
  std::printf("probe_smfmac_bf16_layout: %s\n", bad ? "INCONSISTENT" : "ok");
  CK(hipFree(d));
  return bad != 0;
}
