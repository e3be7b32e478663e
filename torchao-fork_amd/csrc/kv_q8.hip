// Int8 KV cache of the end-to-end harness (torchao/_models/llama AffineQuantizedKVCache; the
// reference's --kv_cache_quantization, model.py:198-240): K and V rows are kept as per-row symmetric
// int8 codes [B][Hkv][T][128] with one bf16 scale per row [B][Hkv][T]. The reference dequantizes the
// whole cache to bf16 on every step (model.py:219-233); here
//   * rope_kv_q8_kernel is rope_kv_kernel (decode_ops.hip) with the cache write quantized by
//     int8_quant_row.h's arithmetic (the reference's _quantize_activation_per_token_absmax in bf16,
//     bit for bit), and the exact bf16 rows of the step kept aside (k_cur / v_cur);
//   * attn_q8_kernel is the one-pass decode attention (attn_single_kernel) reading the codes:
//     keys 0..pos-1 from the int8 caches, the key at pos from k_cur / v_cur ("the current token stays
//     exact", model.py:225, 231). The scales multiply the sums, not the elements:
//       score_t = k_scale[t] * (q . k8[t]) * scale,   o = sum_t p_t * v_scale[t] * v8[t]
//     in fp32, which skips the reference's bf16 rounding of each dequantized element (<= 2^-9
//     relative per element).
// Layout of a 16-key step: a code row is 128 B, so the 8 lanes of group g = lane / 8 cover one key
// with one 16-B load each (lane p8 = lane % 8 holds dims 16 p8 .. 16 p8 + 15); a wave covers keys
// t0 + g and t0 + 8 + g, K and V alike. Each lane keeps the P.V sums of its own 16 dims over its own
// keys (its group's score is already in the lane, so there is no broadcast of the weights); the 8
// groups are summed once per wave at the end. The signed bytes are sign-extended (hipcc emits one
// SDWA v_cvt_f32_i32 per byte): every product and every code is exact in fp32. (Biased bytes
// through v_cvt_f32_ubyte with a -128 sum(w) correction would save no instruction against that and
// subtract two sums 3-4x the result's size, which costs the split / unsplit agreement its margin.)
// One workgroup per query head and key range, as the bf16 kernel: with at most 4 ranges a workgroup
// per kv head would leave B * Hkv * 4 workgroups for 256 CUs; the G query heads of a kv head read
// the same codes through L2 / the Infinity Cache.
#include "int8_quant_row.h"
#include "tao_reduce.h"

namespace tao {

TAO_DECODE_ERROR_WORD(kvq8_decode_status)

namespace {

constexpr int kD = 128;          // head_dim
constexpr int kQ8Waves = 16;     // waves per attention workgroup (attn_single_kernel's)
constexpr int kPartStride = 132; // o[128], m, l, 2 pad (decode_ops.hip; tao_attn_merge_bf16)

// ---- RoPE + quantized KV-cache write: one wave per (token, head), one lane per pair ------------
// Grid (B * S, ceil((H + 2 Hkv) / 4)), 4 waves per workgroup. q heads are rotated and stored as
// rope_kv_kernel stores them. A k head is rotated and rounded to bf16, a v head taken as is; the
// row goes to k_cur / v_cur [B][Hkv][S][128], its amax over the bf16 values is a wave reduction,
// and codes and scale go to the caches at pos[s] (outside [0, T): reported, no cache row written).
__global__ __launch_bounds__(256) void rope_kv_q8_kernel(
    const uint16_t* __restrict__ qkv, const float* __restrict__ freqs,
    const int64_t* __restrict__ pos, uint16_t* __restrict__ q_out, int8_t* __restrict__ kc,
    int8_t* __restrict__ vc, uint16_t* __restrict__ ks, uint16_t* __restrict__ vs,
    uint16_t* __restrict__ k_cur, uint16_t* __restrict__ v_cur, int S, int H, int Hkv, int T) {
  constexpr int half = kD / 2;
  const int tok = blockIdx.x;  // b * S + s
  const int b = tok / S, s = tok % S;
  const int lane = threadIdx.x & 63;
  const int unit = blockIdx.y * 4 + (threadIdx.x >> 6);  // q heads, then k heads, then v heads
  if (unit >= H + 2 * Hkv) return;
  int64_t p = pos[s];
  const bool pok = p >= 0 && p < T;
  if (!pok) {
    if (blockIdx.y == 0 && threadIdx.x == 0) flag_decode_error(kDecodeErrKvPos);
    p = p < 0 ? 0 : T - 1;
  }
  uint32_t w = reinterpret_cast<const uint32_t*>(qkv + (size_t)tok * (H + 2 * Hkv) * kD)
      [unit * half + lane];  // pairs are interleaved: (x[2j], x[2j+1]) = one dword
  if (unit < H + Hkv) {
    const float2 cs = reinterpret_cast<const float2*>(freqs)[(size_t)p * half + lane];
    const float x0 = bf16lo_to_f32(w), x1 = bf16hi_to_f32(w);
    const float o0 = x0 * cs.x - x1 * cs.y, o1 = x1 * cs.x + x0 * cs.y;
    w = (uint32_t)f32_to_bf16(o0) | ((uint32_t)f32_to_bf16(o1) << 16);
  }
  if (unit < H) {
    reinterpret_cast<uint32_t*>(q_out)[(((size_t)b * H + unit) * S + s) * half + lane] = w;
    return;
  }
  const bool is_k = unit < H + Hkv;
  const int kh = is_k ? unit - H : unit - H - Hkv;
  const size_t head = (size_t)b * Hkv + kh;
  reinterpret_cast<uint32_t*>(is_k ? k_cur : v_cur)[(head * S + s) * half + lane] = w;
  const float amax = wave_max(bf16_abs_max2(w, 0.f));
  const float st = token_scale(amax);
  const float r = round_bf16(1.f / st);
  if (!pok) return;
  const uint32_t c = quant1(bf16lo_to_f32(w), r) | (quant1(bf16hi_to_f32(w), r) << 8);
  const size_t row = head * T + (size_t)p;
  reinterpret_cast<uint16_t*>((is_k ? kc : vc) + row * kD)[lane] = (uint16_t)c;
  if (lane == 0) (is_k ? ks : vs)[row] = f32_to_bf16(st);
}

// ---- decode attention over the int8 caches ------------------------------------------------------
__device__ __forceinline__ void s8x16_to_f32(const uint4 v, float (&f)[16]) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) f[4 * j + e] = (float)(int)(int8_t)(d[j] >> (8 * e));
}

__device__ __forceinline__ void bf16x16_to_f32(const uint4 a, const uint4 b, float (&f)[16]) {
  const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f[2 * j] = bf16lo_to_f32(d[j]);
    f[2 * j + 1] = bf16hi_to_f32(d[j]);
  }
}

struct Q8Step {  // one lane's share of a 16-key step: keys t0 + g (a) and t0 + 8 + g (b)
  uint4 ka, kb, va, vb;
  uint16_t ksa, ksb, vsa, vsb;
};

// q [B][H][1][128]; the query at position pos[0] attends the cached keys 0..L-2 (L = pos[0] + 1
// clamped to [1, T]) and the current key (k_cur / v_cur [B][Hkv][1][128]). SPLIT: split
// blockIdx.y of gridDim.y takes cached keys [lo, hi), each split ceil((L - 1) / NS) keys rounded up
// to 16, and writes its unnormalised partial (attn_single_kernel's record); split 0 also takes the
// current key, so it is never empty. The online softmax of the wave that takes the current key
// starts from it: m = s_cur, l = 1, o = v_cur.
template <int NW, bool SPLIT>
__global__ __launch_bounds__(NW * 64) void attn_q8_kernel(
    const uint16_t* __restrict__ q, const int8_t* __restrict__ kc, const int8_t* __restrict__ vc,
    const uint16_t* __restrict__ ks, const uint16_t* __restrict__ vs,
    const uint16_t* __restrict__ k_cur, const uint16_t* __restrict__ v_cur,
    const int64_t* __restrict__ pos, uint16_t* __restrict__ out, float* __restrict__ part, int H,
    int Hkv, int T, float scale) {
  __shared__ float wm[NW], wl[NW];
  __shared__ float wo[NW][kD];
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H, kvh = h / (H / Hkv);
  const int n = attn_len(pos[0], T) - 1;  // cached keys
  int lo = 0, hi = n;
  bool seed = true;
  if constexpr (SPLIT) {
    const int NS = gridDim.y, C = ((n + NS - 1) / NS + 15) & ~15;
    lo = (int)blockIdx.y * C;
    hi = lo + C < n ? lo + C : n;
    seed = blockIdx.y == 0;
    if (lo >= hi && !seed) {  // no keys in this split (uniform): the empty partial
      float* pr = part + ((size_t)bh * NS + blockIdx.y) * kPartStride;
      if (threadIdx.x < kD) pr[threadIdx.x] = 0.f;
      if (threadIdx.x == kD) pr[kD] = -INFINITY;
      if (threadIdx.x == kD + 1) pr[kD + 1] = 0.f;
      return;
    }
  }
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 3, p8 = lane & 7;
  const size_t kvhead = (size_t)b * Hkv + kvh, head = kvhead * T;
  const int8_t* kbase = kc + head * kD + p8 * 16;
  const int8_t* vbase = vc + head * kD + p8 * 16;
  const uint16_t* ksb = ks + head;
  const uint16_t* vsb = vs + head;
  auto load_step = [&](int t0) __attribute__((always_inline)) {
    // keys past the range re-read its last key (in bounds) and are masked below
    const int ta = t0 + g < hi ? t0 + g : hi - 1, tb = t0 + 8 + g < hi ? t0 + 8 + g : hi - 1;
    Q8Step st;
    st.ka = *reinterpret_cast<const uint4*>(kbase + (size_t)ta * kD);
    st.kb = *reinterpret_cast<const uint4*>(kbase + (size_t)tb * kD);
    st.va = *reinterpret_cast<const uint4*>(vbase + (size_t)ta * kD);
    st.vb = *reinterpret_cast<const uint4*>(vbase + (size_t)tb * kD);
    st.ksa = ksb[ta];
    st.ksb = ksb[tb];
    st.vsa = vsb[ta];
    st.vsb = vsb[tb];
    return st;
  };
  const int first = lo + wave * 16;
  Q8Step cur = {};
  if (first < hi) cur = load_step(first);  // before q, so q and the first keys arrive together
  // the current rows and q are issued together with the first keys: one round trip for all
  const bool seeds = seed && wave == 0;
  uint4 kraw[2] = {}, vraw[2] = {};
  if (seeds) {
    const uint4* kp = reinterpret_cast<const uint4*>(k_cur + kvhead * kD + p8 * 16);
    const uint4* vp = reinterpret_cast<const uint4*>(v_cur + kvhead * kD + p8 * 16);
    kraw[0] = kp[0];
    kraw[1] = kp[1];
    vraw[0] = vp[0];
    vraw[1] = vp[1];
  }
  float qf[16];
  {
    const uint4* qp = reinterpret_cast<const uint4*>(q + (size_t)bh * kD + p8 * 16);
    const uint4 q0 = qp[0], q1 = qp[1];
    bf16x16_to_f32(q0, q1, qf);
  }
  float m = -INFINITY, l = 0.f, o[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  if (seeds) {  // the current token, exact bf16
    float kf[16], vf[16];
    bf16x16_to_f32(kraw[0], kraw[1], kf);
    bf16x16_to_f32(vraw[0], vraw[1], vf);
    float sc = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sc = fmaf(qf[i], kf[i], sc);
    sc = wave_bfly<1, 8>(sc, lane, [](float a, float c) { return a + c; });
    m = sc * scale;
    l = 1.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = g == 0 ? vf[i] : 0.f;  // the groups are summed below
  }
  for (int t0 = first; t0 < hi; t0 += NW * 16) {
    Q8Step nx = cur;
    if (t0 + NW * 16 < hi) nx = load_step(t0 + NW * 16);  // wave-uniform prefetch of the next step
    float f[16];
    float sa = 0.f, sb = 0.f;
    s8x16_to_f32(cur.ka, f);
#pragma unroll
    for (int i = 0; i < 16; ++i) sa = fmaf(qf[i], f[i], sa);
    s8x16_to_f32(cur.kb, f);
#pragma unroll
    for (int i = 0; i < 16; ++i) sb = fmaf(qf[i], f[i], sb);
    sa = wave_bfly<1, 8>(sa, lane, [](float a, float c) { return a + c; });
    sb = wave_bfly<1, 8>(sb, lane, [](float a, float c) { return a + c; });
    const bool va = t0 + g < hi, vbk = t0 + 8 + g < hi;
    sa = va ? bf16_to_f32(cur.ksa) * sa * scale : -INFINITY;
    sb = vbk ? bf16_to_f32(cur.ksb) * sb * scale : -INFINITY;
    float mx = fmaxf(sa, sb);
    mx = wave_bfly<8, 64>(mx, lane, [](float a, float c) { return fmaxf(a, c); });
    const float mn = fmaxf(m, mx);  // finite: key t0 < hi is valid
    const float corr = __expf(m - mn);
    const float ea = va ? __expf(sa - mn) : 0.f, eb = vbk ? __expf(sb - mn) : 0.f;
    float es = ea + eb;  // each key sits in 8 lanes of one group: xor 8..32 counts it once
    es = wave_bfly<8, 64>(es, lane, [](float a, float c) { return a + c; });
    l = fmaf(l, corr, es);
    const float pa = ea * bf16_to_f32(cur.vsa), pb = eb * bf16_to_f32(cur.vsb);
    s8x16_to_f32(cur.va, f);
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = fmaf(pa, f[i], o[i] * corr);
    s8x16_to_f32(cur.vb, f);
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = fmaf(pb, f[i], o[i]);
    m = mn;
    cur = nx;
  }
  // sum the 8 key groups: lanes g == 0 end up with the wave's o over dims 16 p8 .. 16 p8 + 15
  // (xor 32 / 16 by permlane swaps; xor 8 through ds_bpermute: the DPP mirror of wave_bfly pairs
  // lane ^ 15, another p8)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float x = o[i];
    x += xor_partner<32>(x, lane);
    x += xor_partner<16>(x, lane);
    x += __shfl_xor(x, 8, 64);
    o[i] = x;
  }
  if (lane == 0) {
    wm[wave] = m;
    wl[wave] = l;
  }
  if (g == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      reinterpret_cast<float4*>(&wo[wave][16 * p8])[j] =
          make_float4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
  }
  __syncthreads();
  if (wave == 0) {  // merge the waves: lane = dim pair (attn_single_kernel's merge)
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) M = fmaxf(M, wm[w]);
    float a0 = 0.f, a1 = 0.f, ls = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float f = wm[w] == -INFINITY ? 0.f : __expf(wm[w] - M);  // waves with no keys
      ls = fmaf(wl[w], f, ls);
      a0 = fmaf(wo[w][2 * lane], f, a0);
      a1 = fmaf(wo[w][2 * lane + 1], f, a1);
    }
    if constexpr (SPLIT) {
      float* pr = part + ((size_t)bh * gridDim.y + blockIdx.y) * kPartStride;
      reinterpret_cast<float2*>(pr)[lane] = make_float2(a0, a1);
      if (lane == 0) reinterpret_cast<float2*>(pr + kD)[0] = make_float2(M, ls);
    } else {
      const float inv = 1.f / ls;
      reinterpret_cast<uint32_t*>(out)[(size_t)bh * (kD / 2) + lane] =
          (uint32_t)f32_to_bf16(a0 * inv) | ((uint32_t)f32_to_bf16(a1 * inv) << 16);
    }
  }
}

}  // namespace
}  // namespace tao

using namespace tao;

extern "C" {

int tao_rope_kv_q8_bf16(const uint16_t* qkv, const float* freqs, const int64_t* pos,
                        uint16_t* q_out, int8_t* k_cache, int8_t* v_cache, uint16_t* k_scale,
                        uint16_t* v_scale, uint16_t* k_cur, uint16_t* v_cur, int64_t B, int64_t S,
                        int64_t H, int64_t Hkv, int64_t D, int64_t T, void* stream) {
  TAO_CHECK_ARG(D == kD, "rope_kv_q8: head_dim must be 128 (got %lld)", (long long)D);
  TAO_CHECK_ARG(B > 0 && S > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && T > 0 &&
                    B * S < (1LL << 31) && H + 2 * Hkv <= 4 * 65535,
                "rope_kv_q8: bad sizes");
  TAO_CHECK_ALIGN(qkv, 4, "qkv");
  TAO_CHECK_ALIGN(freqs, 8, "freqs");
  TAO_CHECK_ALIGN(q_out, 4, "q_out");
  TAO_CHECK_ALIGN(k_cache, 2, "k_cache");
  TAO_CHECK_ALIGN(v_cache, 2, "v_cache");
  TAO_CHECK_ALIGN(k_scale, 2, "k_scale");
  TAO_CHECK_ALIGN(v_scale, 2, "v_scale");
  TAO_CHECK_ALIGN(k_cur, 4, "k_cur");
  TAO_CHECK_ALIGN(v_cur, 4, "v_cur");
  const dim3 grid((unsigned)(B * S), (unsigned)((H + 2 * Hkv + 3) / 4));
  launch(rope_kv_q8_kernel, grid, dim3(256), 0, as_stream(stream), qkv, freqs, pos, q_out,
         k_cache, v_cache, k_scale, v_scale, k_cur, v_cur, (int)S, (int)H, (int)Hkv, (int)T);
  return check_launch("rope_kv_q8_kernel");
}

int tao_attn_decode_q8_bf16(const uint16_t* q, const int8_t* k_cache, const int8_t* v_cache,
                            const uint16_t* k_scale, const uint16_t* v_scale,
                            const uint16_t* k_cur, const uint16_t* v_cur, const int64_t* pos,
                            float* partial, uint16_t* out, int64_t B, int64_t H, int64_t Hkv,
                            int64_t D, int64_t T, float scale, int64_t splits, void* stream) {
  TAO_CHECK_ARG(D == kD, "attn_decode_q8: head_dim must be 128 (got %lld)", (long long)D);
  TAO_CHECK_ARG(splits == 1 || splits == 2 || splits == 4,
                "attn_decode_q8: splits must be 1, 2 or 4 (got %lld)", (long long)splits);
  TAO_CHECK_ARG(B > 0 && Hkv > 0 && H > 0 && H % Hkv == 0 && T > 0 && B * H < (1LL << 31) &&
                    T < (1LL << 31),
                "attn_decode_q8: bad sizes");
  const int G = (int)(H / Hkv);
  TAO_CHECK_ARG(G == 1 || G == 2 || G == 4 || G == 8,
                "attn_decode_q8: H / Hkv must be 1, 2, 4 or 8");
  TAO_CHECK_ARG(splits == 1 ? out != nullptr : partial != nullptr,
                "attn_decode_q8: out (splits 1) or partial (splits 2, 4) is required");
  TAO_CHECK_ALIGN(q, 16, "q");
  TAO_CHECK_ALIGN(k_cache, 16, "k_cache");
  TAO_CHECK_ALIGN(v_cache, 16, "v_cache");
  TAO_CHECK_ALIGN(k_scale, 2, "k_scale");
  TAO_CHECK_ALIGN(v_scale, 2, "v_scale");
  TAO_CHECK_ALIGN(k_cur, 16, "k_cur");
  TAO_CHECK_ALIGN(v_cur, 16, "v_cur");
  TAO_CHECK_ALIGN(partial, 16, "partial");
  TAO_CHECK_ALIGN(out, 4, "out");
  hipStream_t st = as_stream(stream);
  const dim3 blk(64 * kQ8Waves);
  if (splits == 1)
    launch((attn_q8_kernel<kQ8Waves, false>), dim3((unsigned)(B * H)), blk, 0, st, q, k_cache,
           v_cache, k_scale, v_scale, k_cur, v_cur, pos, out, (float*)nullptr, (int)H, (int)Hkv,
           (int)T, scale);
  else
    launch((attn_q8_kernel<kQ8Waves, true>), dim3((unsigned)(B * H), (unsigned)splits), blk, 0, st,
           q, k_cache, v_cache, k_scale, v_scale, k_cur, v_cur, pos, (uint16_t*)nullptr, partial,
           (int)H, (int)Hkv, (int)T, scale);
  return check_launch("attn_q8_kernel");
}

}  // extern "C"
