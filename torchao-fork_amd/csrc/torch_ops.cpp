// torch dispatcher kernels (CUDA key = HIP on PyTorch-ROCm) for the quantized-linear ops that run
// once per linear per forward: int4_weight_only_linear, int8_weight_only_linear,
// int8_quantize_per_token, int8_scaled_mm, int8_dyn_linear, the float8 weight-only set
// fp8_weight_only_linear, fp8_quantize_rows, fp8_dequantize, and the float8 dynamic-activation set
// fp8_scaled_mm, fp8_dyn_linear, the MXFP8 set mx_quantize_rows, mx_scaled_mm, mx_dyn_linear, and the
// MXFP4-weight set mxfp4_quantize_rows, mxfp4w_scaled_mm, mxfp4w_dyn_linear, and the blockwise
// float8 set blockfp8_quantize_act, blockfp8_quantize_weight, blockfp8_dequantize_weight,
// blockfp8_scaled_mm, blockfp8_dyn_linear, and the activation pre-scale set act_prescale,
// int4_prescaled_linear, and the SmoothQuant set int8_smooth_quantize_per_token,
// int8_smooth_quantize_static, int8_smooth_dyn_linear, int8_smooth_static_linear, and the W4A8 set
// rowwise_scaled_linear_cutlass_s8s4, int8_quantize_per_token_f32, int4_quantize_rows_packed,
// w4a8_dyn_linear, and the NF4 set nf4_quantize_blocks, nf4_dequantize, nf4_linear, and the FP6 set
// fp6_quantize_rows, fp6_dequantize, fp6_weight_only_linear, and the MoE set moe_route,
// int4_grouped_linear, moe_combine.
//
// The schemas stay defined in torchao/ops.py (the reference's registration pattern,
// torchao/ops.py:12-21); this library only supplies their CUDA kernels, so a call goes
// dispatcher -> C++ -> the C-ABI (include/torchao_mi355x.h) with no Python frame. The Python
// impls it replaces cost ~19 µs of host time per call at M = 1, four times the 4096x4096 GEMV
// (experiments/eager_overhead.py, profiles/r2_eager_overhead*.json); aten._weight_int4pack_mm,
// which the reference calls here (tensor_core_tiled_layout.py:104), is a C++ kernel too.
//
// Argument checks and messages are those of the Python impls (ops.py), raised as RuntimeError.
// Host-only code: built with g++ against the torch headers (Makefile target `ops`).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include "../../include/torchao_mi355x.h"
#include "../../include/torchao_mi355x_tune.h"  // tao_nf4_linear_route, tao_fp6_linear_route
#include "fp6_host.h"
#include "moe_host.h"

namespace {

using at::Tensor;

void check_rc(int rc, const char* name) {
  TORCH_CHECK(rc == 0, name, " failed (status ", rc, "): ", tao_last_error());
}

hipStream_t stream_of(const Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

// x reshaped to [M, K], contiguous and 16-B aligned (the kernels' vector loads)
Tensor rows_of(const Tensor& x, int64_t K) {
  Tensor x2 = x.reshape({-1, K});
  if (!x2.is_contiguous() || reinterpret_cast<uintptr_t>(x2.data_ptr()) % 16) x2 = x2.contiguous();
  return x2;
}

std::vector<int64_t> out_shape(const Tensor& x, int64_t N) {
  std::vector<int64_t> s(x.sizes().begin(), x.sizes().end() - 1);
  s.push_back(N);
  return s;
}

template <class T>
const T* cptr(const Tensor& t) {
  return reinterpret_cast<const T*>(t.data_ptr());
}
template <class T>
T* mptr(const Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}

// Every operand must live on x's device: the kernels take raw device pointers, so a weight left
// on another GPU (e.g. after a partial .to()) or on the host would reach the launch as a foreign
// pointer. The reference's aten ops raise on such inputs; so does this.
void check_device(const Tensor& x, const Tensor& t, const char* name) {
  TORCH_CHECK(x.is_cuda(), "expected x on a HIP device, got ", x.device());
  TORCH_CHECK(t.device() == x.device(), name, " is on ", t.device(), " but x is on ", x.device(),
              ": all operands must be on the same device");
}
void check_device(const Tensor& x, const std::optional<Tensor>& t, const char* name) {
  if (t.has_value()) check_device(x, *t, name);
}

std::optional<Tensor> bf16_bias(const std::optional<Tensor>& bias) {
  if (!bias.has_value()) return std::nullopt;
  return bias->to(at::kBFloat16).contiguous();
}

// ---- int4 weight-only (ops.py _int4_linear_cuda) ----------------------------------------------
Tensor int4_weight_only_linear(const Tensor& x, const Tensor& packed_w, const Tensor& sz,
                               int64_t group_size, const std::optional<Tensor>& bias) {
  TORCH_CHECK(packed_w.dim() == 2 && packed_w.scalar_type() == at::kInt,
              "packed weight must be a 2D int32 [N, K/8] tensor");
  const int64_t N = packed_w.size(0), K = packed_w.size(1) * 8;
  TORCH_CHECK(group_size == 32 || group_size == 64 || group_size == 128 || group_size == 256,
              "qGroupSize must be 32, 64, 128, or 256");
  TORCH_CHECK(K % group_size == 0, "K (", K, ") must be divisible by qGroupSize");
  TORCH_CHECK(sz.scalar_type() == at::kBFloat16, "scales_and_zeros must be bfloat16");
  TORCH_CHECK(sz.dim() == 3 && sz.size(0) == N && sz.size(1) == K / group_size && sz.size(2) == 2,
              "scales_and_zeros must be [N, K/g, 2] = (", N, ", ", K / group_size, ", 2), got ",
              sz.sizes());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "int4 weight-only linear needs bf16 input");
  TORCH_CHECK(x.size(-1) == K, "x last dim ", x.size(-1), " != K ", K);
  TORCH_CHECK(packed_w.is_contiguous(), "packed_w must be contiguous");
  TORCH_CHECK(sz.is_contiguous(), "scales_and_zeros must be contiguous");
  check_device(x, packed_w, "packed_w");
  check_device(x, sz, "scales_and_zeros");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  check_rc(tao_int4wo_linear_bf16(cptr<uint16_t>(x2), cptr<uint32_t>(packed_w), cptr<uint16_t>(sz),
                                  b ? cptr<uint16_t>(*b) : nullptr, mptr<uint16_t>(y), M, N, K,
                                  group_size, stream_of(x)),
           "tao_int4wo_linear_bf16");
  return y.reshape(out_shape(x, N));
}

// ---- activation pre-scale (AWQ / SmoothQuant equalization; ops.py _act_prescale_cuda) -----------
Tensor check_act_scale(const Tensor& x, const Tensor& scale, int64_t K, const char* op) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, op, " (HIP) needs bf16 x, got ", x.scalar_type());
  TORCH_CHECK(scale.scalar_type() == at::kBFloat16, op, " (HIP) needs a bf16 scale, got ",
              scale.scalar_type());
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == K, "x last dim ", x.dim() ? x.size(-1) : 0, " != K ",
              K);
  TORCH_CHECK(scale.numel() == K, "scale must have K = ", K, " elements, got ", scale.numel());
  check_device(x, scale, "scale");
  Tensor s = scale.reshape({-1});
  if (!s.is_contiguous() || reinterpret_cast<uintptr_t>(s.data_ptr()) % 16) s = s.contiguous();
  return s;
}

Tensor act_prescale(const Tensor& x, const Tensor& scale) {
  const int64_t K = scale.numel();
  const Tensor s = check_act_scale(x, scale, K, "act_prescale");
  TORCH_CHECK(K % 8 == 0, "act_prescale needs K % 8 == 0, got K = ", K);
  const Tensor x2 = rows_of(x, K);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty(x2.sizes(), x.options());
  check_rc(tao_act_prescale_bf16(cptr<uint16_t>(x2), cptr<uint16_t>(s), mptr<uint16_t>(y),
                                 x2.size(0), K, stream_of(x)),
           "tao_act_prescale_bf16");
  return y.reshape(x.sizes());
}

// One token without a bias, where tao_int4wo_prescaled_linear_fused says so (K <= 4096, N * K <=
// 2^24): the fused launch. Otherwise the pre-scale into a buffer of the caching allocator, then the
// plain linear (bit-identical to calling the two ops).
Tensor int4_prescaled_linear(const Tensor& x, const Tensor& act_scale, const Tensor& packed_w,
                             const Tensor& sz, int64_t group_size,
                             const std::optional<Tensor>& bias) {
  TORCH_CHECK(packed_w.dim() == 2 && packed_w.scalar_type() == at::kInt,
              "packed weight must be a 2D int32 [N, K/8] tensor");
  const int64_t N = packed_w.size(0), K = packed_w.size(1) * 8;
  TORCH_CHECK(group_size == 32 || group_size == 64 || group_size == 128 || group_size == 256,
              "qGroupSize must be 32, 64, 128, or 256");
  TORCH_CHECK(K % group_size == 0, "K (", K, ") must be divisible by qGroupSize");
  TORCH_CHECK(sz.scalar_type() == at::kBFloat16, "scales_and_zeros must be bfloat16");
  TORCH_CHECK(sz.dim() == 3 && sz.size(0) == N && sz.size(1) == K / group_size && sz.size(2) == 2,
              "scales_and_zeros must be [N, K/g, 2] = (", N, ", ", K / group_size, ", 2), got ",
              sz.sizes());
  const Tensor s = check_act_scale(x, act_scale, K, "int4_prescaled_linear");
  TORCH_CHECK(packed_w.is_contiguous(), "packed_w must be contiguous");
  TORCH_CHECK(sz.is_contiguous(), "scales_and_zeros must be contiguous");
  check_device(x, packed_w, "packed_w");
  check_device(x, sz, "scales_and_zeros");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options());
  if (tao_int4wo_prescaled_linear_fused(M, N, K, b ? 1 : 0)) {
    check_rc(tao_int4wo_prescaled_linear_bf16(cptr<uint16_t>(x2), cptr<uint16_t>(s),
                                              cptr<uint32_t>(packed_w), cptr<uint16_t>(sz),
                                              nullptr, mptr<uint16_t>(y), 1, N, K, group_size,
                                              stream_of(x)),
             "tao_int4wo_prescaled_linear_bf16");
  } else if (M > 0) {
    Tensor xs = at::empty({M, K}, x.options());
    check_rc(tao_act_prescale_bf16(cptr<uint16_t>(x2), cptr<uint16_t>(s), mptr<uint16_t>(xs), M,
                                   K, stream_of(x)),
             "tao_act_prescale_bf16");
    check_rc(tao_int4wo_linear_bf16(cptr<uint16_t>(xs), cptr<uint32_t>(packed_w),
                                    cptr<uint16_t>(sz), b ? cptr<uint16_t>(*b) : nullptr,
                                    mptr<uint16_t>(y), M, N, K, group_size, stream_of(x)),
             "tao_int4wo_linear_bf16");
  }
  return y.reshape(out_shape(x, N));
}

// ---- int8 ------------------------------------------------------------------------------------
void check_int8_weight(const Tensor& w, const Tensor& scale) {
  TORCH_CHECK(w.dim() == 2 && w.scalar_type() == at::kChar, "w must be a 2D int8 tensor");
  TORCH_CHECK(scale.numel() == w.size(0), "scale must have N elements");
}

Tensor int8_weight_only_linear(const Tensor& x, const Tensor& w_int8, const Tensor& scale,
                               const std::optional<Tensor>& bias) {
  check_int8_weight(w_int8, scale);
  const int64_t N = w_int8.size(0), K = w_int8.size(1);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "int8 weight-only linear (HIP) needs bf16 x");
  TORCH_CHECK(x.size(-1) == K, "x last dim ", x.size(-1), " != K ", K);
  check_device(x, w_int8, "w_int8");
  check_device(x, scale, "scale");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const Tensor w = w_int8.contiguous();
  const Tensor s = scale.reshape({-1}).to(at::kBFloat16).contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  check_rc(tao_int8wo_linear_bf16(cptr<uint16_t>(x2), cptr<int8_t>(w), cptr<uint16_t>(s),
                                  b ? cptr<uint16_t>(*b) : nullptr, mptr<uint16_t>(y), M, N, K,
                                  stream_of(x)),
           "tao_int8wo_linear_bf16");
  return y.reshape(out_shape(x, N));
}

std::tuple<Tensor, Tensor> int8_quantize_per_token(const Tensor& x) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "int8 per-token quant (HIP) needs bf16 x");
  const int64_t K = x.size(-1);
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor q = at::empty({M, K}, x.options().dtype(at::kChar));
  Tensor s = at::empty({M, 1}, x.options().dtype(at::kBFloat16));
  check_rc(tao_int8_quant_per_token(cptr<uint16_t>(x2), mptr<int8_t>(q), mptr<uint16_t>(s), M, K,
                                    stream_of(x)),
           "tao_int8_quant_per_token");
  std::vector<int64_t> ss(x.sizes().begin(), x.sizes().end() - 1);
  ss.push_back(1);
  return {q.reshape(x.sizes()), s.reshape(ss)};
}

Tensor int8_scaled_mm(const Tensor& x_int8, const Tensor& x_scale, const Tensor& w_int8,
                      const Tensor& w_scale, const std::optional<Tensor>& bias) {
  check_int8_weight(w_int8, w_scale);
  const int64_t N = w_int8.size(0), K = w_int8.size(1);
  TORCH_CHECK(x_int8.scalar_type() == at::kChar, "x_int8 must be int8");
  TORCH_CHECK(x_int8.size(-1) == K, "x last dim ", x_int8.size(-1), " != K ", K);
  check_device(x_int8, x_scale, "x_scale");
  check_device(x_int8, w_int8, "w_int8");
  check_device(x_int8, w_scale, "w_scale");
  check_device(x_int8, bias, "bias");
  const Tensor x2 = x_int8.reshape({-1, K}).contiguous();
  const int64_t M = x2.size(0);
  const Tensor xs = x_scale.reshape({-1}).to(at::kBFloat16).contiguous();
  TORCH_CHECK(xs.numel() == M, "x_scale must have one entry per row");
  const Tensor ws = w_scale.reshape({-1}).to(at::kBFloat16).contiguous();
  const Tensor w = w_int8.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x_int8.device());
  Tensor y = at::empty({M, N}, x_int8.options().dtype(at::kBFloat16));
  check_rc(tao_int8_scaled_mm_bf16(cptr<int8_t>(x2), cptr<uint16_t>(xs), cptr<int8_t>(w),
                                   cptr<uint16_t>(ws), b ? cptr<uint16_t>(*b) : nullptr,
                                   mptr<uint16_t>(y), M, N, K, stream_of(x_int8)),
           "tao_int8_scaled_mm_bf16");
  return y.reshape(out_shape(x_int8, N));
}

Tensor int8_dyn_linear(const Tensor& x, const Tensor& w_int8, const Tensor& w_scale,
                       const std::optional<Tensor>& bias) {
  check_int8_weight(w_int8, w_scale);
  const int64_t N = w_int8.size(0), K = w_int8.size(1);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "int8_dyn_linear (HIP) needs bf16 x");
  TORCH_CHECK(x.size(-1) == K, "x last dim ", x.size(-1), " != K ", K);
  TORCH_CHECK(x.numel() == K, "int8_dyn_linear is one token (x.numel() == K)");
  check_device(x, w_int8, "w_int8");
  check_device(x, w_scale, "w_scale");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const Tensor ws = w_scale.reshape({-1}).to(at::kBFloat16).contiguous();
  const Tensor w = w_int8.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({1, N}, x.options().dtype(at::kBFloat16));
  check_rc(tao_int8_dyn_linear_bf16(cptr<uint16_t>(x2), cptr<int8_t>(w), cptr<uint16_t>(ws),
                                    b ? cptr<uint16_t>(*b) : nullptr, mptr<uint16_t>(y), 1, N, K,
                                    stream_of(x)),
           "tao_int8_dyn_linear_bf16");
  return y.reshape(out_shape(x, N));
}

// ---- SmoothQuant on the int8 dynamic / static linear (ops.py _int8_smooth_*_cuda) ----------------
// The per-tensor activation scale of the static recipe: one bf16 value on x's device.
Tensor check_smooth_act_scale(const Tensor& x, const Tensor& act_scale, const char* op) {
  TORCH_CHECK(act_scale.scalar_type() == at::kBFloat16 && act_scale.numel() == 1, op,
              " needs a bf16 act_scale of one element, got ", act_scale.scalar_type(), " with ",
              act_scale.numel());
  check_device(x, act_scale, "act_scale");
  return act_scale.reshape({1}).contiguous();
}

std::tuple<Tensor, Tensor> int8_smooth_quantize(const Tensor& x, const Tensor& smooth,
                                                const Tensor* act_scale, const char* op) {
  const int64_t K = smooth.numel();
  const Tensor s = check_act_scale(x, smooth, K, op);
  TORCH_CHECK(K % 16 == 0 && K > 0 && K <= 65536, op,
              " needs K % 16 == 0 and 0 < K <= 65536, got K = ", K);
  std::optional<Tensor> as;
  if (act_scale != nullptr) as = check_smooth_act_scale(x, *act_scale, op);
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor q = at::empty({M, K}, x.options().dtype(at::kChar));
  Tensor sc = at::empty({M}, x.options());
  check_rc(tao_int8_smooth_quant_bf16(cptr<uint16_t>(x2), cptr<uint16_t>(s),
                                      as ? cptr<uint16_t>(*as) : nullptr, mptr<int8_t>(q),
                                      mptr<uint16_t>(sc), M, K, stream_of(x)),
           "tao_int8_smooth_quant_bf16");
  return {q.reshape(x.sizes()), sc};
}

std::tuple<Tensor, Tensor> int8_smooth_quantize_per_token(const Tensor& x, const Tensor& smooth) {
  return int8_smooth_quantize(x, smooth, nullptr, "int8_smooth_quantize_per_token");
}

std::tuple<Tensor, Tensor> int8_smooth_quantize_static(const Tensor& x, const Tensor& smooth,
                                                       const Tensor& act_scale) {
  return int8_smooth_quantize(x, smooth, &act_scale, "int8_smooth_quantize_static");
}

// One token where tao_int8_smooth_linear_fused says so: the one launch. Otherwise the fused
// quantizer into buffers of the caching allocator, then int8_scaled_mm's entry (the GEMV for
// M <= 4, the MFMA above): bit-identical.
Tensor int8_smooth_linear(const Tensor& x, const Tensor& smooth, const Tensor* act_scale,
                          const Tensor& w_int8, const Tensor& w_scale,
                          const std::optional<Tensor>& bias, const char* op) {
  check_int8_weight(w_int8, w_scale);
  const int64_t N = w_int8.size(0), K = w_int8.size(1);
  const Tensor s = check_act_scale(x, smooth, K, op);
  TORCH_CHECK(K % 16 == 0 && K > 0 && K <= 65536, op,
              " needs K % 16 == 0 and 0 < K <= 65536, got K = ", K);
  std::optional<Tensor> as;
  if (act_scale != nullptr) as = check_smooth_act_scale(x, *act_scale, op);
  check_device(x, w_int8, "w_int8");
  check_device(x, w_scale, "w_scale");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const Tensor ws = w_scale.reshape({-1}).to(at::kBFloat16).contiguous();
  const Tensor w = w_int8.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  const uint16_t* asp = as ? cptr<uint16_t>(*as) : nullptr;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options());
  if (tao_int8_smooth_linear_fused(M, N, K, asp != nullptr)) {
    check_rc(tao_int8_smooth_linear_bf16(cptr<uint16_t>(x2), cptr<uint16_t>(s), asp,
                                         cptr<int8_t>(w), cptr<uint16_t>(ws),
                                         b ? cptr<uint16_t>(*b) : nullptr, mptr<uint16_t>(y), 1, N,
                                         K, stream_of(x)),
             "tao_int8_smooth_linear_bf16");
  } else if (M > 0) {
    Tensor q = at::empty({M, K}, x.options().dtype(at::kChar));
    Tensor sc = at::empty({M}, x.options());
    check_rc(tao_int8_smooth_quant_bf16(cptr<uint16_t>(x2), cptr<uint16_t>(s), asp,
                                        mptr<int8_t>(q), mptr<uint16_t>(sc), M, K, stream_of(x)),
             "tao_int8_smooth_quant_bf16");
    check_rc(tao_int8_scaled_mm_bf16(cptr<int8_t>(q), cptr<uint16_t>(sc), cptr<int8_t>(w),
                                     cptr<uint16_t>(ws), b ? cptr<uint16_t>(*b) : nullptr,
                                     mptr<uint16_t>(y), M, N, K, stream_of(x)),
             "tao_int8_scaled_mm_bf16");
  }
  return y.reshape(out_shape(x, N));
}

Tensor int8_smooth_dyn_linear(const Tensor& x, const Tensor& smooth, const Tensor& w_int8,
                              const Tensor& w_scale, const std::optional<Tensor>& bias) {
  return int8_smooth_linear(x, smooth, nullptr, w_int8, w_scale, bias, "int8_smooth_dyn_linear");
}

Tensor int8_smooth_static_linear(const Tensor& x, const Tensor& smooth, const Tensor& act_scale,
                                 const Tensor& w_int8, const Tensor& w_scale,
                                 const std::optional<Tensor>& bias) {
  return int8_smooth_linear(x, smooth, &act_scale, w_int8, w_scale, bias,
                            "int8_smooth_static_linear");
}

// ---- float8 (e4m3fn) weight-only (ops.py _fp8wo_linear_cuda & co) -----------------------------
void check_fp8_weight(const Tensor& w, const Tensor& scale) {
  TORCH_CHECK(w.dim() == 2 && w.scalar_type() == at::kFloat8_e4m3fn,
              "w must be a 2D float8_e4m3fn tensor");
  TORCH_CHECK(scale.numel() == w.size(0), "scale must have N elements");
}

Tensor fp8_weight_only_linear(const Tensor& x, const Tensor& w_fp8, const Tensor& scale,
                              const std::optional<Tensor>& bias) {
  check_fp8_weight(w_fp8, scale);
  const int64_t N = w_fp8.size(0), K = w_fp8.size(1);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "fp8 weight-only linear (HIP) needs bf16 x");
  TORCH_CHECK(x.size(-1) == K, "x last dim ", x.size(-1), " != K ", K);
  check_device(x, w_fp8, "w_fp8");
  check_device(x, scale, "scale");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const Tensor w = w_fp8.contiguous();
  const Tensor s = scale.reshape({-1}).to(at::kFloat).contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  check_rc(tao_fp8wo_linear_bf16(cptr<uint16_t>(x2), cptr<uint8_t>(w), cptr<float>(s),
                                 b ? cptr<uint16_t>(*b) : nullptr, mptr<uint16_t>(y), M, N, K,
                                 stream_of(x)),
           "tao_fp8wo_linear_bf16");
  return y.reshape(out_shape(x, N));
}

std::tuple<Tensor, Tensor> fp8_quantize_rows(const Tensor& w) {
  TORCH_CHECK(w.is_cuda(), "expected w on a HIP device, got ", w.device());
  TORCH_CHECK(w.scalar_type() == at::kBFloat16, "fp8 quantize (HIP) needs a bf16 weight");
  TORCH_CHECK(w.dim() >= 1, "fp8 quantize: w must have at least one dimension");
  const int64_t K = w.size(-1);
  TORCH_CHECK(K % 8 == 0, "K (", K, ") must be a multiple of 8");
  const Tensor w2 = rows_of(w, K);
  const int64_t R = w2.size(0);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  Tensor q = at::empty({R, K}, w.options().dtype(at::kFloat8_e4m3fn));
  Tensor s = at::empty({R}, w.options().dtype(at::kFloat));
  check_rc(tao_fp8_quantize_rows_bf16(cptr<uint16_t>(w2), mptr<uint8_t>(q), mptr<float>(s), R, K,
                                      stream_of(w)),
           "tao_fp8_quantize_rows_bf16");
  std::vector<int64_t> ss(w.sizes().begin(), w.sizes().end() - 1);
  ss.push_back(1);
  return {q.reshape(w.sizes()), s.reshape(ss)};
}

Tensor fp8_dequantize(const Tensor& q, const Tensor& scale) {
  TORCH_CHECK(q.is_cuda(), "expected q on a HIP device, got ", q.device());
  check_fp8_weight(q, scale);
  check_device(q, scale, "scale");
  const int64_t N = q.size(0), K = q.size(1);
  TORCH_CHECK(K % 8 == 0, "K (", K, ") must be a multiple of 8");
  const Tensor qc = q.contiguous();
  const Tensor s = scale.reshape({-1}).to(at::kFloat).contiguous();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(q.device());
  Tensor w = at::empty({N, K}, q.options().dtype(at::kBFloat16));
  check_rc(tao_fp8_dequant_bf16(cptr<uint8_t>(qc), cptr<float>(s), mptr<uint16_t>(w), N, K,
                                stream_of(q)),
           "tao_fp8_dequant_bf16");
  return w;
}

// ---- float8 dynamic activation x float8 weight (ops.py _fp8_scaled_mm_cuda & co) ---------------
Tensor fp8_scaled_mm(const Tensor& xq, const Tensor& x_scale, const Tensor& w_fp8,
                     const Tensor& w_scale, const std::optional<Tensor>& bias) {
  check_fp8_weight(w_fp8, w_scale);
  const int64_t N = w_fp8.size(0), K = w_fp8.size(1);
  TORCH_CHECK(xq.scalar_type() == at::kFloat8_e4m3fn, "xq must be float8_e4m3fn");
  TORCH_CHECK(xq.size(-1) == K, "x last dim ", xq.size(-1), " != K ", K);
  TORCH_CHECK(K % 16 == 0, "K (", K, ") must be a multiple of 16");
  check_device(xq, x_scale, "x_scale");
  check_device(xq, w_fp8, "w_fp8");
  check_device(xq, w_scale, "w_scale");
  check_device(xq, bias, "bias");
  const Tensor x2 = xq.reshape({-1, K}).contiguous();
  const int64_t M = x2.size(0);
  const Tensor xs = x_scale.reshape({-1}).to(at::kFloat).contiguous();
  TORCH_CHECK(xs.numel() == M, "x_scale must have one entry per row");
  const Tensor ws = w_scale.reshape({-1}).to(at::kFloat).contiguous();
  const Tensor w = w_fp8.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(xq.device());
  Tensor y = at::empty({M, N}, xq.options().dtype(at::kBFloat16));
  check_rc(tao_fp8_scaled_mm_bf16(cptr<uint8_t>(x2), cptr<float>(xs), cptr<uint8_t>(w),
                                  cptr<float>(ws), b ? cptr<uint16_t>(*b) : nullptr,
                                  mptr<uint16_t>(y), M, N, K, stream_of(xq)),
           "tao_fp8_scaled_mm_bf16");
  return y.reshape(out_shape(xq, N));
}

Tensor fp8_dyn_linear(const Tensor& x, const Tensor& w_fp8, const Tensor& w_scale,
                      const std::optional<Tensor>& bias) {
  check_fp8_weight(w_fp8, w_scale);
  const int64_t N = w_fp8.size(0), K = w_fp8.size(1);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "fp8_dyn_linear (HIP) needs bf16 x");
  TORCH_CHECK(x.size(-1) == K, "x last dim ", x.size(-1), " != K ", K);
  TORCH_CHECK(K % 16 == 0, "K (", K, ") must be a multiple of 16");
  check_device(x, w_fp8, "w_fp8");
  check_device(x, w_scale, "w_scale");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const Tensor ws = w_scale.reshape({-1}).to(at::kFloat).contiguous();
  const Tensor w = w_fp8.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  const uint16_t* bp = b ? cptr<uint16_t>(*b) : nullptr;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  if (M == 1 && K <= 65536) {
    check_rc(tao_fp8_dyn_linear_bf16(cptr<uint16_t>(x2), cptr<uint8_t>(w), cptr<float>(ws), bp,
                                     mptr<uint16_t>(y), 1, N, K, stream_of(x)),
             "tao_fp8_dyn_linear_bf16");
  } else if (M > 0) {
    // the codes live in a buffer of the caching allocator between the two launches
    Tensor q = at::empty({M, K}, x.options().dtype(at::kFloat8_e4m3fn));
    Tensor s = at::empty({M}, x.options().dtype(at::kFloat));
    check_rc(tao_fp8_quantize_rows_bf16(cptr<uint16_t>(x2), mptr<uint8_t>(q), mptr<float>(s), M, K,
                                        stream_of(x)),
             "tao_fp8_quantize_rows_bf16");
    check_rc(tao_fp8_scaled_mm_bf16(cptr<uint8_t>(q), cptr<float>(s), cptr<uint8_t>(w),
                                    cptr<float>(ws), bp, mptr<uint16_t>(y), M, N, K, stream_of(x)),
             "tao_fp8_scaled_mm_bf16");
  }
  return y.reshape(out_shape(x, N));
}

// ---- MXFP8: e4m3fn codes, one E8M0 byte per 32-k block (ops.py _mx_scaled_mm_cuda & co) ---------
// Scale bytes cross the op boundary as uint8 (MXTensor views its float8_e8m0fnu storage).
void check_mx_operand(const Tensor& q, const Tensor& scale, const char* qn, const char* sn) {
  TORCH_CHECK(q.scalar_type() == at::kFloat8_e4m3fn, qn, " must be float8_e4m3fn");
  TORCH_CHECK(scale.scalar_type() == at::kByte, sn, " must be uint8 (E8M0 bytes)");
  const int64_t K = q.size(-1);
  TORCH_CHECK(K % 32 == 0, "K (", K, ") must be a multiple of 32");
  TORCH_CHECK(scale.numel() * 32 == q.numel() && (scale.dim() == 0 || scale.size(-1) == K / 32),
              sn, " must hold one byte per 32-element block: [..., K/32] = [..., ", K / 32,
              "], got ", scale.sizes());
}

// scale bytes as [rows, K/32], contiguous and 8-B aligned (the MFMA route's 8-B scale loads)
Tensor mx_scale_rows(const Tensor& s, int64_t K) {
  Tensor s2 = s.reshape({-1, K / 32});
  if (!s2.is_contiguous() || reinterpret_cast<uintptr_t>(s2.data_ptr()) % 8) s2 = s2.clone();
  return s2;
}

std::tuple<Tensor, Tensor> mx_quantize_rows(const Tensor& x) {
  TORCH_CHECK(x.is_cuda(), "expected x on a HIP device, got ", x.device());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "mx quantize (HIP) needs bf16 x");
  TORCH_CHECK(x.dim() >= 1, "mx quantize: x must have at least one dimension");
  const int64_t K = x.size(-1);
  TORCH_CHECK(K % 32 == 0, "K (", K, ") must be a multiple of 32");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor q = at::empty({M, K}, x.options().dtype(at::kFloat8_e4m3fn));
  Tensor s = at::empty({M, K / 32}, x.options().dtype(at::kByte));
  check_rc(tao_mx_quantize_rows_bf16(cptr<uint16_t>(x2), mptr<uint8_t>(q), mptr<uint8_t>(s), M, K,
                                     stream_of(x)),
           "tao_mx_quantize_rows_bf16");
  std::vector<int64_t> ss(x.sizes().begin(), x.sizes().end() - 1);
  ss.push_back(K / 32);
  return {q.reshape(x.sizes()), s.reshape(ss)};
}

Tensor mx_scaled_mm(const Tensor& xq, const Tensor& x_scale, const Tensor& wq,
                    const Tensor& w_scale, const std::optional<Tensor>& bias) {
  TORCH_CHECK(wq.dim() == 2, "wq must be a 2D float8_e4m3fn tensor");
  check_mx_operand(wq, w_scale, "wq", "w_scale");
  const int64_t N = wq.size(0), K = wq.size(1);
  TORCH_CHECK(xq.dim() >= 1 && xq.size(-1) == K, "x last dim ", xq.dim() ? xq.size(-1) : 0,
              " != K ", K);
  check_mx_operand(xq, x_scale, "xq", "x_scale");
  check_device(xq, x_scale, "x_scale");
  check_device(xq, wq, "wq");
  check_device(xq, w_scale, "w_scale");
  check_device(xq, bias, "bias");
  const Tensor x2 = xq.reshape({-1, K}).contiguous();
  const int64_t M = x2.size(0);
  const Tensor xs = mx_scale_rows(x_scale, K);
  const Tensor ws = mx_scale_rows(w_scale, K);
  const Tensor w = wq.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(xq.device());
  Tensor y = at::empty({M, N}, xq.options().dtype(at::kBFloat16));
  check_rc(tao_mx_scaled_mm_bf16(cptr<uint8_t>(x2), cptr<uint8_t>(xs), cptr<uint8_t>(w),
                                 cptr<uint8_t>(ws), b ? cptr<uint16_t>(*b) : nullptr,
                                 mptr<uint16_t>(y), M, N, K, stream_of(xq)),
           "tao_mx_scaled_mm_bf16");
  return y.reshape(out_shape(xq, N));
}

Tensor mx_dyn_linear(const Tensor& x, const Tensor& wq, const Tensor& w_scale,
                     const std::optional<Tensor>& bias) {
  TORCH_CHECK(wq.dim() == 2, "wq must be a 2D float8_e4m3fn tensor");
  check_mx_operand(wq, w_scale, "wq", "w_scale");
  const int64_t N = wq.size(0), K = wq.size(1);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "mx_dyn_linear (HIP) needs bf16 x");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == K, "x last dim ", x.dim() ? x.size(-1) : 0, " != K ",
              K);
  check_device(x, wq, "wq");
  check_device(x, w_scale, "w_scale");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const Tensor ws = mx_scale_rows(w_scale, K);
  const Tensor w = wq.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  const uint16_t* bp = b ? cptr<uint16_t>(*b) : nullptr;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  if (M == 1 && K <= 65536) {
    check_rc(tao_mx_dyn_linear_bf16(cptr<uint16_t>(x2), cptr<uint8_t>(w), cptr<uint8_t>(ws), bp,
                                    mptr<uint16_t>(y), 1, N, K, stream_of(x)),
             "tao_mx_dyn_linear_bf16");
  } else if (M > 0) {
    // codes and scale bytes live in buffers of the caching allocator between the two launches
    Tensor q = at::empty({M, K}, x.options().dtype(at::kFloat8_e4m3fn));
    Tensor s = at::empty({M, K / 32}, x.options().dtype(at::kByte));
    check_rc(tao_mx_quantize_rows_bf16(cptr<uint16_t>(x2), mptr<uint8_t>(q), mptr<uint8_t>(s), M, K,
                                       stream_of(x)),
             "tao_mx_quantize_rows_bf16");
    check_rc(tao_mx_scaled_mm_bf16(cptr<uint8_t>(q), cptr<uint8_t>(s), cptr<uint8_t>(w),
                                   cptr<uint8_t>(ws), bp, mptr<uint16_t>(y), M, N, K, stream_of(x)),
             "tao_mx_scaled_mm_bf16");
  }
  return y.reshape(out_shape(x, N));
}

// ---- MXFP4 weights under MXFP8 activations (ops.py _mxfp4w_scaled_mm_cuda & co) --------------------
// wq: uint8 [N, K/2], two e2m1 codes per byte (element 2 j in the high nibble); scales as above.
int64_t check_mxfp4_weight(const Tensor& wq, const Tensor& w_scale) {
  TORCH_CHECK(wq.dim() == 2 && wq.scalar_type() == at::kByte,
              "wq must be a 2D uint8 tensor of packed e2m1 codes [N, K/2]");
  TORCH_CHECK(w_scale.scalar_type() == at::kByte, "w_scale must be uint8 (E8M0 bytes)");
  const int64_t K = 2 * wq.size(1);
  TORCH_CHECK(K % 32 == 0, "K (", K, ") must be a multiple of 32");
  TORCH_CHECK(w_scale.numel() * 32 == 2 * wq.numel() &&
                  (w_scale.dim() == 0 || w_scale.size(-1) == K / 32),
              "w_scale must hold one byte per 32-element block: [..., K/32] = [..., ", K / 32,
              "], got ", w_scale.sizes());
  return K;
}

std::tuple<Tensor, Tensor> mxfp4_quantize_rows(const Tensor& x) {
  TORCH_CHECK(x.is_cuda(), "expected x on a HIP device, got ", x.device());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "mxfp4 quantize (HIP) needs bf16 x");
  TORCH_CHECK(x.dim() >= 1, "mxfp4 quantize: x must have at least one dimension");
  const int64_t K = x.size(-1);
  TORCH_CHECK(K % 32 == 0, "K (", K, ") must be a multiple of 32");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor q = at::empty({M, K / 2}, x.options().dtype(at::kByte));
  Tensor s = at::empty({M, K / 32}, x.options().dtype(at::kByte));
  check_rc(tao_mxfp4_quantize_rows_bf16(cptr<uint16_t>(x2), mptr<uint8_t>(q), mptr<uint8_t>(s), M,
                                        K, stream_of(x)),
           "tao_mxfp4_quantize_rows_bf16");
  std::vector<int64_t> qs(x.sizes().begin(), x.sizes().end() - 1), ss = qs;
  qs.push_back(K / 2);
  ss.push_back(K / 32);
  return {q.reshape(qs), s.reshape(ss)};
}

Tensor mxfp4w_scaled_mm(const Tensor& xq, const Tensor& x_scale, const Tensor& wq,
                        const Tensor& w_scale, const std::optional<Tensor>& bias) {
  const int64_t K = check_mxfp4_weight(wq, w_scale), N = wq.size(0);
  TORCH_CHECK(xq.dim() >= 1 && xq.size(-1) == K, "x last dim ", xq.dim() ? xq.size(-1) : 0,
              " != K ", K);
  check_mx_operand(xq, x_scale, "xq", "x_scale");
  check_device(xq, x_scale, "x_scale");
  check_device(xq, wq, "wq");
  check_device(xq, w_scale, "w_scale");
  check_device(xq, bias, "bias");
  const Tensor x2 = xq.reshape({-1, K}).contiguous();
  const int64_t M = x2.size(0);
  const Tensor xs = mx_scale_rows(x_scale, K);
  const Tensor ws = mx_scale_rows(w_scale, K);
  const Tensor w = wq.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(xq.device());
  Tensor y = at::empty({M, N}, xq.options().dtype(at::kBFloat16));
  check_rc(tao_mxfp4w_scaled_mm_bf16(cptr<uint8_t>(x2), cptr<uint8_t>(xs), cptr<uint8_t>(w),
                                     cptr<uint8_t>(ws), b ? cptr<uint16_t>(*b) : nullptr,
                                     mptr<uint16_t>(y), M, N, K, stream_of(xq)),
           "tao_mxfp4w_scaled_mm_bf16");
  return y.reshape(out_shape(xq, N));
}

Tensor mxfp4w_dyn_linear(const Tensor& x, const Tensor& wq, const Tensor& w_scale,
                         const std::optional<Tensor>& bias) {
  const int64_t K = check_mxfp4_weight(wq, w_scale), N = wq.size(0);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "mxfp4w_dyn_linear (HIP) needs bf16 x");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == K, "x last dim ", x.dim() ? x.size(-1) : 0, " != K ",
              K);
  check_device(x, wq, "wq");
  check_device(x, w_scale, "w_scale");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const Tensor ws = mx_scale_rows(w_scale, K);
  const Tensor w = wq.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  const uint16_t* bp = b ? cptr<uint16_t>(*b) : nullptr;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  if (M == 1 && K <= 65536) {
    check_rc(tao_mxfp4w_dyn_linear_bf16(cptr<uint16_t>(x2), cptr<uint8_t>(w), cptr<uint8_t>(ws),
                                        bp, mptr<uint16_t>(y), 1, N, K, stream_of(x)),
             "tao_mxfp4w_dyn_linear_bf16");
  } else if (M > 0) {
    // the activation's e4m3fn codes and scale bytes live in buffers of the caching allocator
    // between the two launches
    Tensor q = at::empty({M, K}, x.options().dtype(at::kFloat8_e4m3fn));
    Tensor s = at::empty({M, K / 32}, x.options().dtype(at::kByte));
    check_rc(tao_mx_quantize_rows_bf16(cptr<uint16_t>(x2), mptr<uint8_t>(q), mptr<uint8_t>(s), M, K,
                                       stream_of(x)),
             "tao_mx_quantize_rows_bf16");
    check_rc(tao_mxfp4w_scaled_mm_bf16(cptr<uint8_t>(q), cptr<uint8_t>(s), cptr<uint8_t>(w),
                                       cptr<uint8_t>(ws), bp, mptr<uint16_t>(y), M, N, K,
                                       stream_of(x)),
             "tao_mxfp4w_scaled_mm_bf16");
  }
  return y.reshape(out_shape(x, N));
}

// ---- Blockwise float8: e4m3fn codes, fp32 scales per 1 x 128 (activation) and 128 x 128 (weight)
// block (ops.py _blockfp8_scaled_mm_cuda & co) ---------------------------------------------------
int64_t check_blockfp8_k(const Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() >= 1, name, " must have at least one dimension");
  const int64_t K = t.size(-1);
  TORCH_CHECK(K % 128 == 0, "K (", K, ") must be a multiple of 128 (blockwise float8 serves block ",
              "size 128 only)");
  return K;
}

void check_blockfp8_act(const Tensor& xq, const Tensor& x_scale) {
  TORCH_CHECK(xq.scalar_type() == at::kFloat8_e4m3fn, "xq must be float8_e4m3fn");
  TORCH_CHECK(x_scale.scalar_type() == at::kFloat, "x_scale must be float32");
  const int64_t K = check_blockfp8_k(xq, "xq");
  TORCH_CHECK(x_scale.numel() * 128 == xq.numel() &&
                  (x_scale.dim() == 0 || x_scale.size(-1) == K / 128),
              "x_scale must hold one float32 per 1x128 block: [..., K/128] = [..., ", K / 128,
              "], got ", x_scale.sizes());
}

std::pair<int64_t, int64_t> check_blockfp8_weight(const Tensor& wq, const Tensor& w_scale) {
  TORCH_CHECK(wq.dim() == 2 && wq.scalar_type() == at::kFloat8_e4m3fn,
              "wq must be a 2D float8_e4m3fn tensor");
  TORCH_CHECK(w_scale.scalar_type() == at::kFloat, "w_scale must be float32");
  const int64_t N = wq.size(0), K = check_blockfp8_k(wq, "wq");
  TORCH_CHECK(w_scale.dim() == 2 && w_scale.size(0) == (N + 127) / 128 &&
                  w_scale.size(1) == K / 128,
              "w_scale must hold one float32 per 128x128 block: [ceil(N/128), K/128] = [",
              (N + 127) / 128, ", ", K / 128, "], got ", w_scale.sizes());
  return {N, K};
}

std::tuple<Tensor, Tensor> blockfp8_quantize_act(const Tensor& x) {
  TORCH_CHECK(x.is_cuda(), "expected x on a HIP device, got ", x.device());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "blockfp8 quantize act (HIP) needs bf16 x");
  const int64_t K = check_blockfp8_k(x, "x");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor q = at::empty({M, K}, x.options().dtype(at::kFloat8_e4m3fn));
  Tensor s = at::empty({M, K / 128}, x.options().dtype(at::kFloat));
  check_rc(tao_blockfp8_quantize_act_bf16(cptr<uint16_t>(x2), mptr<uint8_t>(q), mptr<float>(s), M,
                                          K, stream_of(x)),
           "tao_blockfp8_quantize_act_bf16");
  std::vector<int64_t> ss(x.sizes().begin(), x.sizes().end() - 1);
  ss.push_back(K / 128);
  return {q.reshape(x.sizes()), s.reshape(ss)};
}

std::tuple<Tensor, Tensor> blockfp8_quantize_weight(const Tensor& w) {
  TORCH_CHECK(w.is_cuda(), "expected w on a HIP device, got ", w.device());
  TORCH_CHECK(w.scalar_type() == at::kBFloat16, "blockfp8 quantize weight (HIP) needs bf16 w");
  TORCH_CHECK(w.dim() == 2, "blockfp8 quantize weight: w must be 2D [N, K]");
  const int64_t N = w.size(0), K = check_blockfp8_k(w, "w");
  const Tensor w2 = rows_of(w, K);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  Tensor q = at::empty({N, K}, w.options().dtype(at::kFloat8_e4m3fn));
  Tensor s = at::empty({(N + 127) / 128, K / 128}, w.options().dtype(at::kFloat));
  check_rc(tao_blockfp8_quantize_weight_bf16(cptr<uint16_t>(w2), mptr<uint8_t>(q), mptr<float>(s),
                                             N, K, stream_of(w)),
           "tao_blockfp8_quantize_weight_bf16");
  return {q, s};
}

Tensor blockfp8_dequantize_weight(const Tensor& wq, const Tensor& w_scale, bool out_bf16) {
  TORCH_CHECK(wq.is_cuda(), "expected wq on a HIP device, got ", wq.device());
  const auto [N, K] = check_blockfp8_weight(wq, w_scale);
  check_device(wq, w_scale, "w_scale");
  const Tensor q = wq.contiguous();
  const Tensor s = w_scale.contiguous();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(wq.device());
  Tensor out = at::empty({N, K}, wq.options().dtype(out_bf16 ? at::kBFloat16 : at::kFloat));
  check_rc(tao_blockfp8_dequant_weight(cptr<uint8_t>(q), cptr<float>(s), out.data_ptr(), N, K,
                                       out_bf16 ? 1 : 0, stream_of(wq)),
           "tao_blockfp8_dequant_weight");
  return out;
}

Tensor blockfp8_scaled_mm(const Tensor& xq, const Tensor& x_scale, const Tensor& wq,
                          const Tensor& w_scale, const std::optional<Tensor>& bias) {
  const auto [N, K] = check_blockfp8_weight(wq, w_scale);
  TORCH_CHECK(xq.dim() >= 1 && xq.size(-1) == K, "x last dim ", xq.dim() ? xq.size(-1) : 0,
              " != K ", K);
  check_blockfp8_act(xq, x_scale);
  TORCH_CHECK(!bias.has_value() || (bias->scalar_type() == at::kBFloat16 && bias->numel() == N),
              "bias must be bfloat16 with N elements");
  check_device(xq, x_scale, "x_scale");
  check_device(xq, wq, "wq");
  check_device(xq, w_scale, "w_scale");
  check_device(xq, bias, "bias");
  const Tensor x2 = xq.reshape({-1, K}).contiguous();
  const int64_t M = x2.size(0);
  const Tensor xs = x_scale.reshape({-1, K / 128}).contiguous();
  const Tensor ws = w_scale.contiguous();
  const Tensor w = wq.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(xq.device());
  Tensor y = at::empty({M, N}, xq.options().dtype(at::kBFloat16));
  check_rc(tao_blockfp8_scaled_mm_bf16(cptr<uint8_t>(x2), cptr<float>(xs), cptr<uint8_t>(w),
                                       cptr<float>(ws), b ? cptr<uint16_t>(*b) : nullptr,
                                       mptr<uint16_t>(y), M, N, K, stream_of(xq)),
           "tao_blockfp8_scaled_mm_bf16");
  return y.reshape(out_shape(xq, N));
}

Tensor blockfp8_dyn_linear(const Tensor& x, const Tensor& wq, const Tensor& w_scale,
                           const std::optional<Tensor>& bias) {
  const auto [N, K] = check_blockfp8_weight(wq, w_scale);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "blockfp8_dyn_linear (HIP) needs bf16 x");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == K, "x last dim ", x.dim() ? x.size(-1) : 0, " != K ",
              K);
  TORCH_CHECK(!bias.has_value() || (bias->scalar_type() == at::kBFloat16 && bias->numel() == N),
              "bias must be bfloat16 with N elements");
  check_device(x, wq, "wq");
  check_device(x, w_scale, "w_scale");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const Tensor ws = w_scale.contiguous();
  const Tensor w = wq.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  const uint16_t* bp = b ? cptr<uint16_t>(*b) : nullptr;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  if (M == 1 && K <= 65536) {
    check_rc(tao_blockfp8_dyn_linear_bf16(cptr<uint16_t>(x2), cptr<uint8_t>(w), cptr<float>(ws),
                                          bp, mptr<uint16_t>(y), 1, N, K, stream_of(x)),
             "tao_blockfp8_dyn_linear_bf16");
  } else if (M > 0) {
    // codes and scales live in buffers of the caching allocator between the two launches
    Tensor q = at::empty({M, K}, x.options().dtype(at::kFloat8_e4m3fn));
    Tensor s = at::empty({M, K / 128}, x.options().dtype(at::kFloat));
    check_rc(tao_blockfp8_quantize_act_bf16(cptr<uint16_t>(x2), mptr<uint8_t>(q), mptr<float>(s),
                                            M, K, stream_of(x)),
             "tao_blockfp8_quantize_act_bf16");
    check_rc(tao_blockfp8_scaled_mm_bf16(cptr<uint8_t>(q), cptr<float>(s), cptr<uint8_t>(w),
                                         cptr<float>(ws), bp, mptr<uint16_t>(y), M, N, K,
                                         stream_of(x)),
             "tao_blockfp8_scaled_mm_bf16");
  }
  return y.reshape(out_shape(x, N));
}

// ---- W4A8: int8 dynamic activation x packed int4 weight (ops.py _w4a8_scaled_mm_cuda & co) ------
void check_w4a8_weight(const Tensor& w, const Tensor& w_scale) {
  TORCH_CHECK(w.dim() == 2 && (w.scalar_type() == at::kChar || w.scalar_type() == at::kByte),
              "weight must be a 2D int8 [N, K/2] tensor of packed int4 codes");
  TORCH_CHECK(w_scale.scalar_type() == at::kFloat, "weight_scale must be float32");
  TORCH_CHECK(w_scale.dim() == 1 && w_scale.numel() == w.size(0),
              "weight_scale must be [N] = (", w.size(0), "), got ", w_scale.sizes());
  TORCH_CHECK((w.size(1) * 2) % 32 == 0, "K (", w.size(1) * 2, ") must be a multiple of 32");
}

Tensor rowwise_scaled_linear_cutlass_s8s4(const Tensor& input, const Tensor& input_scale,
                                          const Tensor& weight, const Tensor& weight_scale,
                                          const std::optional<Tensor>& bias,
                                          std::optional<at::ScalarType> out_dtype) {
  check_w4a8_weight(weight, weight_scale);
  const int64_t N = weight.size(0), K = weight.size(1) * 2;
  TORCH_CHECK(input.scalar_type() == at::kChar, "input must be int8");
  TORCH_CHECK(input_scale.scalar_type() == at::kFloat, "input_scale must be float32");
  TORCH_CHECK(input.dim() >= 1 && input.size(-1) == K, "input last dim ",
              input.dim() ? input.size(-1) : 0, " != K ", K);
  TORCH_CHECK(!out_dtype.has_value() || *out_dtype == at::kBFloat16,
              "rowwise_scaled_linear_cutlass_s8s4 (HIP) gives bfloat16 output only");
  TORCH_CHECK(!bias.has_value() || (bias->dim() == 1 && bias->numel() == N),
              "bias must be [N] = (", N, ")");
  check_device(input, input_scale, "input_scale");
  check_device(input, weight, "weight");
  check_device(input, weight_scale, "weight_scale");
  check_device(input, bias, "bias");
  const Tensor x2 = rows_of(input, K);
  const int64_t M = x2.size(0);
  const Tensor xs = input_scale.reshape({-1}).contiguous();
  TORCH_CHECK(xs.numel() == M, "input_scale must have one entry per row");
  const Tensor w = weight.contiguous();
  const Tensor ws = weight_scale.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(input.device());
  Tensor y = at::empty({M, N}, input.options().dtype(at::kBFloat16));
  check_rc(tao_w4a8_scaled_mm_bf16(cptr<int8_t>(x2), cptr<float>(xs), cptr<uint8_t>(w),
                                   cptr<float>(ws), b ? cptr<uint16_t>(*b) : nullptr,
                                   mptr<uint16_t>(y), M, N, K, stream_of(input)),
           "tao_w4a8_scaled_mm_bf16");
  return y.reshape(out_shape(input, N));
}

std::tuple<Tensor, Tensor> int8_quantize_per_token_f32(const Tensor& x) {
  TORCH_CHECK(x.is_cuda(), "expected x on a HIP device, got ", x.device());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "int8_quantize_per_token_f32 (HIP) needs bf16 x");
  TORCH_CHECK(x.dim() >= 1, "int8_quantize_per_token_f32: x must have at least one dimension");
  const int64_t K = x.size(-1);
  TORCH_CHECK(K % 8 == 0, "K (", K, ") must be a multiple of 8");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor q = at::empty({M, K}, x.options().dtype(at::kChar));
  Tensor s = at::empty({M}, x.options().dtype(at::kFloat));
  check_rc(tao_int8_quant_per_token_f32(cptr<uint16_t>(x2), mptr<int8_t>(q), mptr<float>(s), M, K,
                                        stream_of(x)),
           "tao_int8_quant_per_token_f32");
  std::vector<int64_t> ss(x.sizes().begin(), x.sizes().end() - 1);
  return {q.reshape(x.sizes()), s.reshape(ss)};
}

std::tuple<Tensor, Tensor> int4_quantize_rows_packed(const Tensor& w) {
  TORCH_CHECK(w.is_cuda(), "expected w on a HIP device, got ", w.device());
  TORCH_CHECK(w.scalar_type() == at::kBFloat16, "int4_quantize_rows_packed (HIP) needs a bf16 weight");
  TORCH_CHECK(w.dim() == 2, "int4_quantize_rows_packed: w must be [N, K]");
  const int64_t R = w.size(0), K = w.size(1);
  TORCH_CHECK(K % 8 == 0, "K (", K, ") must be a multiple of 8");
  const Tensor w2 = rows_of(w, K);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  Tensor q = at::empty({R, K / 2}, w.options().dtype(at::kChar));
  Tensor s = at::empty({R}, w.options().dtype(at::kFloat));
  check_rc(tao_int4_quantize_rows_packed_bf16(cptr<uint16_t>(w2), mptr<uint8_t>(q), mptr<float>(s),
                                              R, K, stream_of(w)),
           "tao_int4_quantize_rows_packed_bf16");
  return {q, s};
}

Tensor w4a8_dyn_linear(const Tensor& x, const Tensor& weight, const Tensor& weight_scale,
                       const std::optional<Tensor>& bias) {
  check_w4a8_weight(weight, weight_scale);
  const int64_t N = weight.size(0), K = weight.size(1) * 2;
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "w4a8_dyn_linear (HIP) needs bf16 x");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == K, "x last dim ", x.dim() ? x.size(-1) : 0, " != K ",
              K);
  TORCH_CHECK(!bias.has_value() || (bias->dim() == 1 && bias->numel() == N),
              "bias must be [N] = (", N, ")");
  check_device(x, weight, "weight");
  check_device(x, weight_scale, "weight_scale");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const Tensor w = weight.contiguous();
  const Tensor ws = weight_scale.contiguous();
  const std::optional<Tensor> b = bf16_bias(bias);
  const uint16_t* bp = b ? cptr<uint16_t>(*b) : nullptr;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  if (M == 1 && K <= 65536) {
    check_rc(tao_w4a8_dyn_linear_bf16(cptr<uint16_t>(x2), cptr<uint8_t>(w), cptr<float>(ws), bp,
                                      mptr<uint16_t>(y), 1, N, K, stream_of(x)),
             "tao_w4a8_dyn_linear_bf16");
  } else if (M > 0) {
    // the codes live in a buffer of the caching allocator between the two launches
    Tensor q = at::empty({M, K}, x.options().dtype(at::kChar));
    Tensor s = at::empty({M}, x.options().dtype(at::kFloat));
    check_rc(tao_int8_quant_per_token_f32(cptr<uint16_t>(x2), mptr<int8_t>(q), mptr<float>(s), M,
                                          K, stream_of(x)),
             "tao_int8_quant_per_token_f32");
    check_rc(tao_w4a8_scaled_mm_bf16(cptr<int8_t>(q), cptr<float>(s), cptr<uint8_t>(w),
                                     cptr<float>(ws), bp, mptr<uint16_t>(y), M, N, K,
                                     stream_of(x)),
             "tao_w4a8_scaled_mm_bf16");
  }
  return y.reshape(out_shape(x, N));
}

// ---- NF4 (QLoRA) weight-only (torchao/dtypes/nf4tensor.py; csrc/nf4.hip) ------------------------
// The five stored tensors of an NF4Tensor: codes uint8 [numel / 2], qscalers int8 [numel / 64],
// qfactor bf16 [numel / 16384], mean bf16 0-dim, levels bf16 [16]
struct Nf4Parts {
  Tensor codes, qs, qf, mean, levels;
};
Nf4Parts check_nf4(const Tensor& codes, const Tensor& qscalers, const Tensor& qfactor,
                   const Tensor& mean, const Tensor& levels, int64_t numel, const char* op) {
  TORCH_CHECK(codes.is_cuda(), op, ": expected codes on a HIP device, got ", codes.device());
  TORCH_CHECK(codes.scalar_type() == at::kByte, op, ": codes must be uint8, got ",
              codes.scalar_type());
  TORCH_CHECK(qscalers.scalar_type() == at::kChar, op, ": qscalers must be int8, got ",
              qscalers.scalar_type());
  TORCH_CHECK(qfactor.scalar_type() == at::kBFloat16 && mean.scalar_type() == at::kBFloat16 &&
                  levels.scalar_type() == at::kBFloat16,
              op, " (HIP) needs bf16 qfactor, mean and levels");
  TORCH_CHECK(numel % 64 == 0, op, ": numel (", numel, ") must be a multiple of the block size 64");
  TORCH_CHECK(codes.numel() == numel / 2, op, ": codes must have numel / 2 = ", numel / 2,
              " bytes, got ", codes.numel());
  TORCH_CHECK(qscalers.numel() == numel / 64, op, ": qscalers must have numel / 64 = ", numel / 64,
              " elements, got ", qscalers.numel());
  TORCH_CHECK(qfactor.numel() == (numel + 16383) / 16384, op,
              ": qfactor must have ceil(numel / 16384) = ", (numel + 16383) / 16384,
              " elements, got ", qfactor.numel());
  TORCH_CHECK(mean.numel() == 1, op, ": mean must have one element, got ", mean.numel());
  TORCH_CHECK(levels.numel() == 16, op, ": levels must have 16 elements, got ", levels.numel());
  check_device(codes, qscalers, "qscalers");
  check_device(codes, qfactor, "qfactor");
  check_device(codes, mean, "mean");
  check_device(codes, levels, "levels");
  auto flat = [](const Tensor& t, uintptr_t align) {
    Tensor f = t.reshape({-1});
    if (!f.is_contiguous() || reinterpret_cast<uintptr_t>(f.data_ptr()) % align) f = f.clone();
    return f;
  };
  return {flat(codes, 16), flat(qscalers, 1), flat(qfactor, 2), flat(mean, 2), flat(levels, 4)};
}

std::tuple<Tensor, Tensor> nf4_quantize_blocks(const Tensor& w, const Tensor& levels) {
  TORCH_CHECK(w.is_cuda(), "nf4_quantize_blocks: expected w on a HIP device, got ", w.device());
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && levels.scalar_type() == at::kBFloat16,
              "nf4_quantize_blocks (HIP) needs a bf16 weight and bf16 levels");
  TORCH_CHECK(levels.numel() == 16, "nf4_quantize_blocks: levels must have 16 elements, got ",
              levels.numel());
  check_device(w, levels, "levels");
  const int64_t numel = w.numel();
  TORCH_CHECK(numel % 64 == 0, "nf4_quantize_blocks: numel (", numel,
              ") must be a multiple of the block size 64");
  Tensor wf = w.reshape({-1});
  if (!wf.is_contiguous() || reinterpret_cast<uintptr_t>(wf.data_ptr()) % 16) wf = wf.clone();
  const Tensor lv = levels.reshape({-1}).contiguous();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  Tensor codes = at::empty({numel / 2}, w.options().dtype(at::kByte));
  Tensor absmax = at::empty({numel / 64}, w.options());
  check_rc(tao_nf4_quantize_blocks_bf16(cptr<uint16_t>(wf), cptr<uint16_t>(lv),
                                        mptr<uint8_t>(codes), mptr<uint16_t>(absmax), numel,
                                        stream_of(w)),
           "tao_nf4_quantize_blocks_bf16");
  return {codes, absmax};
}

Tensor nf4_dequantize_flat(const Nf4Parts& p, int64_t numel) {
  Tensor w = at::empty({numel}, p.codes.options().dtype(at::kBFloat16));
  check_rc(tao_nf4_dequant_bf16(cptr<uint8_t>(p.codes), cptr<int8_t>(p.qs), cptr<uint16_t>(p.qf),
                                cptr<uint16_t>(p.mean), cptr<uint16_t>(p.levels),
                                mptr<uint16_t>(w), numel, stream_of(p.codes)),
           "tao_nf4_dequant_bf16");
  return w;
}

Tensor nf4_dequantize(const Tensor& codes, const Tensor& qscalers, const Tensor& qfactor,
                      const Tensor& mean, const Tensor& levels, at::IntArrayRef shape) {
  int64_t numel = 1;
  for (const int64_t d : shape) {
    TORCH_CHECK(d >= 0, "nf4_dequantize: shape must be non-negative, got ", shape);
    numel *= d;
  }
  const Nf4Parts p = check_nf4(codes, qscalers, qfactor, mean, levels, numel, "nf4_dequantize");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(codes.device());
  return nf4_dequantize_flat(p, numel).reshape(shape);
}

Tensor nf4_linear(const Tensor& x, const Tensor& codes, const Tensor& qscalers,
                  const Tensor& qfactor, const Tensor& mean, const Tensor& levels, int64_t N,
                  const std::optional<Tensor>& bias) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "nf4_linear (HIP) needs bf16 x, got ",
              x.scalar_type());
  TORCH_CHECK(x.dim() >= 1, "nf4_linear: x must have at least one dimension");
  TORCH_CHECK(N >= 0, "nf4_linear: N must be non-negative, got ", N);
  const int64_t K = x.size(-1);
  TORCH_CHECK(K > 0 && K % 64 == 0, "nf4_linear: K (", K,
              ") must be a positive multiple of the block size 64");
  check_device(x, codes, "codes");
  const Nf4Parts p = check_nf4(codes, qscalers, qfactor, mean, levels, N * K, "nf4_linear");
  TORCH_CHECK(!bias.has_value() || bias->numel() == N, "nf4_linear: bias must have N = ", N,
              " elements");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  if (M > 0 && N > 0 && tao_nf4_linear_route(M, N, K) == 2) {
    // the reference's own form with a fast dequantizer: W^ into a temporary of the caching
    // allocator, then the bf16 matmul; the bias is a second rounding, as on the other route
    const Tensor w = nf4_dequantize_flat(p, N * K).reshape({N, K});
    Tensor y = at::linear(x2, w);
    if (b) y = y + *b;
    return y.reshape(out_shape(x, N));
  }
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  check_rc(tao_nf4_linear_bf16(cptr<uint16_t>(x2), cptr<uint8_t>(p.codes), cptr<int8_t>(p.qs),
                               cptr<uint16_t>(p.qf), cptr<uint16_t>(p.mean),
                               cptr<uint16_t>(p.levels), b ? cptr<uint16_t>(*b) : nullptr,
                               mptr<uint16_t>(y), M, N, K, stream_of(x)),
           "tao_nf4_linear_bf16");
  return y.reshape(out_shape(x, N));
}

// ---- FP6 weight-only (torchao/dtypes/floatx/floatx_tensor_core_layout.py; csrc/fp6.hip) ---------
// codes int32 [N, K * 6 / 32] (native storage), scale bf16 [N]
void check_fp6_format(int64_t ebits, int64_t mbits, const char* op) {
  TORCH_CHECK(tao::fp6_format_of(ebits, mbits) >= 0, op, ": (ebits, mbits) = (", ebits, ", ",
              mbits, ") is not served; served: (3, 2) and (2, 3)");
}

struct Fp6Weight {
  Tensor codes, scale;
  int64_t N, K;
};
Fp6Weight check_fp6_weight(const Tensor& codes, const Tensor& scale, const char* op) {
  TORCH_CHECK(codes.is_cuda(), op, ": expected codes on a HIP device, got ", codes.device());
  TORCH_CHECK(codes.dim() == 2 && codes.scalar_type() == at::kInt, op,
              ": codes must be a 2D int32 [N, K * 6 / 32] tensor, got ", codes.scalar_type(), " ",
              codes.sizes());
  TORCH_CHECK(codes.size(1) % 6 == 0, op,
              ": codes must hold whole 32-code groups of 6 dwords, got ", codes.size(1),
              " dwords per row");
  const int64_t N = codes.size(0), K = codes.size(1) / 6 * 32;
  TORCH_CHECK(scale.scalar_type() == at::kBFloat16, op, " (HIP) needs a bf16 scale, got ",
              scale.scalar_type());
  TORCH_CHECK(scale.numel() == N, op, ": scale must have N = ", N, " elements, got ",
              scale.numel());
  check_device(codes, scale, "scale");
  Tensor c = codes;
  if (!c.is_contiguous() || reinterpret_cast<uintptr_t>(c.data_ptr()) % 16) c = c.clone();
  return {c, scale.reshape({-1}).contiguous(), N, K};
}

std::tuple<Tensor, Tensor> fp6_quantize_rows(const Tensor& w, int64_t ebits, int64_t mbits) {
  check_fp6_format(ebits, mbits, "fp6_quantize_rows");
  TORCH_CHECK(w.is_cuda(), "fp6_quantize_rows: expected w on a HIP device, got ", w.device());
  TORCH_CHECK(w.scalar_type() == at::kBFloat16, "fp6_quantize_rows (HIP) needs a bf16 weight, got ",
              w.scalar_type());
  TORCH_CHECK(w.dim() == 2, "fp6_quantize_rows: w must be 2D, got ", w.dim(), "D");
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(K % 32 == 0, "fp6_quantize_rows: K (", K, ") must be a multiple of 32");
  Tensor wc = w;
  if (!wc.is_contiguous() || reinterpret_cast<uintptr_t>(wc.data_ptr()) % 16) wc = wc.clone();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  Tensor codes = at::empty({N, tao::fp6_row_dwords(K)}, w.options().dtype(at::kInt));
  Tensor scale = at::empty({N}, w.options());
  check_rc(tao_fp6_quantize_rows_bf16(cptr<uint16_t>(wc), mptr<uint32_t>(codes),
                                      mptr<uint16_t>(scale), N, K, (int)ebits, (int)mbits,
                                      stream_of(w)),
           "tao_fp6_quantize_rows_bf16");
  return {codes, scale};
}

Tensor fp6_dequantize_checked(const Fp6Weight& p, int64_t ebits, int64_t mbits) {
  Tensor w = at::empty({p.N, p.K}, p.codes.options().dtype(at::kBFloat16));
  check_rc(tao_fp6_dequant_bf16(cptr<uint32_t>(p.codes), cptr<uint16_t>(p.scale),
                                mptr<uint16_t>(w), p.N, p.K, (int)ebits, (int)mbits,
                                stream_of(p.codes)),
           "tao_fp6_dequant_bf16");
  return w;
}

Tensor fp6_dequantize(const Tensor& codes, const Tensor& scale, int64_t ebits, int64_t mbits) {
  check_fp6_format(ebits, mbits, "fp6_dequantize");
  const Fp6Weight p = check_fp6_weight(codes, scale, "fp6_dequantize");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(codes.device());
  return fp6_dequantize_checked(p, ebits, mbits);
}

Tensor fp6_weight_only_linear(const Tensor& x, const Tensor& codes, const Tensor& scale,
                              int64_t ebits, int64_t mbits, const std::optional<Tensor>& bias) {
  check_fp6_format(ebits, mbits, "fp6_weight_only_linear");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "fp6_weight_only_linear (HIP) needs bf16 x, got ",
              x.scalar_type());
  TORCH_CHECK(x.dim() >= 1, "fp6_weight_only_linear: x must have at least one dimension");
  check_device(x, codes, "codes");
  const Fp6Weight p = check_fp6_weight(codes, scale, "fp6_weight_only_linear");
  const int64_t N = p.N, K = p.K;
  TORCH_CHECK(K > 0 && K % 64 == 0, "fp6_weight_only_linear: K (", K,
              ") must be a positive multiple of 64");
  TORCH_CHECK(x.size(-1) == K, "x last dim ", x.size(-1), " != K ", K);
  TORCH_CHECK(!bias.has_value() || bias->numel() == N, "fp6_weight_only_linear: bias must have N = ",
              N, " elements");
  check_device(x, bias, "bias");
  const Tensor x2 = rows_of(x, K);
  const int64_t M = x2.size(0);
  const std::optional<Tensor> b = bf16_bias(bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  if (M > 0 && N > 0 && tao_fp6_linear_route(M, N, K) == 2) {
    // W^ into a temporary of the caching allocator, then the bf16 matmul; the bias is a second
    // rounding, as on the other route
    const Tensor w = fp6_dequantize_checked(p, ebits, mbits);
    Tensor y = at::linear(x2, w);
    if (b) y = y + *b;
    return y.reshape(out_shape(x, N));
  }
  Tensor y = at::empty({M, N}, x.options().dtype(at::kBFloat16));
  check_rc(tao_fp6_linear_bf16(cptr<uint16_t>(x2), cptr<uint32_t>(p.codes),
                               cptr<uint16_t>(p.scale), b ? cptr<uint16_t>(*b) : nullptr,
                               mptr<uint16_t>(y), M, N, K, (int)ebits, (int)mbits, stream_of(x)),
           "tao_fp6_linear_bf16");
  return y.reshape(out_shape(x, N));
}

// ---- MoE expert FFN over many tokens (torchao/prototype/moe_quant; csrc/moe_gemm.hip) -----------
std::tuple<Tensor, Tensor, Tensor> moe_route(const Tensor& expert_indices, int64_t num_experts,
                                             int64_t top_k) {
  TORCH_CHECK(expert_indices.is_cuda(), "moe_route: expected expert_indices on a HIP device, got ",
              expert_indices.device());
  TORCH_CHECK(expert_indices.scalar_type() == at::kLong, "moe_route: expert_indices must be int64, got ",
              expert_indices.scalar_type());
  TORCH_CHECK(num_experts >= 1 && num_experts <= tao::kMoeMaxExperts, "moe_route: num_experts (",
              num_experts, ") is not served; served: 1 to ", tao::kMoeMaxExperts);
  TORCH_CHECK(top_k >= 1 && top_k <= tao::kMoeMaxTopK, "moe_route: top_k (", top_k,
              ") is not served; served: 1 to ", tao::kMoeMaxTopK);
  const Tensor idx = expert_indices.reshape({-1}).contiguous();
  const int64_t R = idx.numel();
  TORCH_CHECK(R % top_k == 0, "moe_route: expert_indices has ", R,
              " elements, not a multiple of top_k = ", top_k);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(idx.device());
  const auto opt = idx.options().dtype(at::kInt);
  Tensor offsets = at::empty({num_experts + 1}, opt);
  Tensor order = at::empty({R}, opt), inverse = at::empty({R}, opt);
  check_rc(tao_moe_route(cptr<int64_t>(idx), R, top_k, num_experts, mptr<int32_t>(offsets),
                         mptr<int32_t>(order), mptr<int32_t>(inverse), stream_of(idx)),
           "tao_moe_route");
  return {offsets, order, inverse};
}

void check_int4_stack(const Tensor& x, const Tensor& packed, const Tensor& sz, int64_t group_size,
                      const char* name) {
  TORCH_CHECK(packed.dim() == 3 && packed.scalar_type() == at::kInt, "int4_grouped_linear: ", name,
              " must be a 3D int32 [E, N, K/8] tensor");
  const int64_t E = packed.size(0), N = packed.size(1), K = packed.size(2) * 8;
  TORCH_CHECK(sz.scalar_type() == at::kBFloat16 && sz.dim() == 4 && sz.size(0) == E &&
                  sz.size(1) == N && sz.size(2) == K / group_size && sz.size(3) == 2,
              "int4_grouped_linear: scales_and_zeros of ", name, " must be bfloat16 [E, N, K/g, 2] = (",
              E, ", ", N, ", ", K / group_size, ", 2), got ", sz.sizes());
  TORCH_CHECK(packed.is_contiguous() && sz.is_contiguous(), "int4_grouped_linear: ", name,
              " and its scales_and_zeros must be contiguous");
  check_device(x, packed, name);
  check_device(x, sz, "scales_and_zeros");
}

Tensor int4_grouped_linear(const Tensor& x, const std::optional<Tensor>& src_row, int64_t row_div,
                           const Tensor& packed, const Tensor& sz,
                           const std::optional<Tensor>& packed_b,
                           const std::optional<Tensor>& sz_b, const Tensor& offsets,
                           int64_t group_size) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 2,
              "int4_grouped_linear (HIP) needs a 2D bf16 x, got ", x.scalar_type(), " ", x.dim(), "D");
  TORCH_CHECK(group_size == 32 || group_size == 64 || group_size == 128 || group_size == 256,
              "qGroupSize must be 32, 64, 128, or 256");
  TORCH_CHECK(packed.dim() == 3 && packed.size(2) * 8 % group_size == 0,
              "int4_grouped_linear: packed must be [E, N, K/8] with K divisible by qGroupSize");
  check_int4_stack(x, packed, sz, group_size, "packed");
  const int64_t E = packed.size(0), N = packed.size(1), K = packed.size(2) * 8;
  TORCH_CHECK(E <= tao::kMoeMaxExperts, "int4_grouped_linear: E (", E, ") is not served; served: 1 to ",
              tao::kMoeMaxExperts);
  TORCH_CHECK(packed_b.has_value() == sz_b.has_value(),
              "int4_grouped_linear: the second stack needs both packed_b and scales_and_zeros_b");
  if (packed_b.has_value()) {
    check_int4_stack(x, *packed_b, *sz_b, group_size, "packed_b");
    TORCH_CHECK(packed_b->sizes() == packed.sizes(), "int4_grouped_linear: packed_b ",
                packed_b->sizes(), " must have packed's shape ", packed.sizes());
  }
  TORCH_CHECK(x.size(1) == K, "x last dim ", x.size(1), " != K ", K);
  TORCH_CHECK(offsets.scalar_type() == at::kInt && offsets.dim() == 1 && offsets.size(0) == E + 1 &&
                  offsets.is_contiguous(),
              "int4_grouped_linear: offsets must be a contiguous int32 [E + 1] tensor");
  check_device(x, offsets, "offsets");
  TORCH_CHECK(row_div >= 1, "int4_grouped_linear: row_div must be >= 1");
  int64_t R = x.size(0);
  if (src_row.has_value()) {
    TORCH_CHECK(src_row->scalar_type() == at::kInt && src_row->dim() == 1 && src_row->is_contiguous(),
                "int4_grouped_linear: src_row must be a contiguous 1D int32 tensor");
    check_device(x, *src_row, "src_row");
    R = src_row->numel();
  }
  const Tensor x2 = rows_of(x, K);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({R, N}, x.options());
  check_rc(tao_int4wo_grouped_linear_bf16(
               cptr<uint16_t>(x2), x2.size(0), src_row ? cptr<int32_t>(*src_row) : nullptr, row_div,
               cptr<uint32_t>(packed), cptr<uint16_t>(sz),
               packed_b ? cptr<uint32_t>(*packed_b) : nullptr, sz_b ? cptr<uint16_t>(*sz_b) : nullptr,
               cptr<int32_t>(offsets), R, E, mptr<uint16_t>(y), N, K, group_size, stream_of(x)),
           "tao_int4wo_grouped_linear_bf16");
  return y;
}

Tensor moe_combine(const Tensor& y2, const Tensor& expert_weights, const Tensor& inverse,
                   int64_t top_k) {
  TORCH_CHECK(y2.is_cuda(), "moe_combine: expected y2 on a HIP device, got ", y2.device());
  TORCH_CHECK(y2.scalar_type() == at::kBFloat16 && y2.dim() == 2 && y2.is_contiguous(),
              "moe_combine (HIP) needs a contiguous 2D bf16 y2");
  TORCH_CHECK(top_k >= 1 && top_k <= tao::kMoeMaxTopK, "moe_combine: top_k (", top_k,
              ") is not served; served: 1 to ", tao::kMoeMaxTopK);
  const int64_t R = y2.size(0), D = y2.size(1);
  TORCH_CHECK(R % top_k == 0, "moe_combine: y2 has ", R, " rows, not a multiple of top_k = ", top_k);
  TORCH_CHECK(D % 8 == 0, "moe_combine: D (", D, ") must be a multiple of 8");
  TORCH_CHECK(expert_weights.scalar_type() == at::kBFloat16 && expert_weights.numel() == R,
              "moe_combine: expert_weights must be bf16 with R = ", R, " elements");
  TORCH_CHECK(inverse.scalar_type() == at::kInt && inverse.numel() == R && inverse.is_contiguous(),
              "moe_combine: inverse must be a contiguous int32 tensor of R = ", R, " elements");
  check_device(y2, expert_weights, "expert_weights");
  check_device(y2, inverse, "inverse");
  const Tensor w = expert_weights.reshape({-1}).contiguous();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(y2.device());
  Tensor out = at::empty({R / top_k, D}, y2.options());
  check_rc(tao_moe_combine_bf16(cptr<uint16_t>(y2), cptr<uint16_t>(w), cptr<int32_t>(inverse),
                                mptr<uint16_t>(out), R / top_k, top_k, D, stream_of(y2)),
           "tao_moe_combine_bf16");
  return out;
}

}  // namespace

TORCH_LIBRARY_IMPL(torchao, CUDA, m) {
  m.impl("moe_route", &moe_route);
  m.impl("int4_grouped_linear", &int4_grouped_linear);
  m.impl("moe_combine", &moe_combine);
  m.impl("fp6_quantize_rows", &fp6_quantize_rows);
  m.impl("fp6_dequantize", &fp6_dequantize);
  m.impl("fp6_weight_only_linear", &fp6_weight_only_linear);
  m.impl("nf4_quantize_blocks", &nf4_quantize_blocks);
  m.impl("nf4_dequantize", &nf4_dequantize);
  m.impl("nf4_linear", &nf4_linear);
  m.impl("rowwise_scaled_linear_cutlass_s8s4", &rowwise_scaled_linear_cutlass_s8s4);
  m.impl("int8_quantize_per_token_f32", &int8_quantize_per_token_f32);
  m.impl("int4_quantize_rows_packed", &int4_quantize_rows_packed);
  m.impl("w4a8_dyn_linear", &w4a8_dyn_linear);
  m.impl("blockfp8_quantize_act", &blockfp8_quantize_act);
  m.impl("blockfp8_quantize_weight", &blockfp8_quantize_weight);
  m.impl("blockfp8_dequantize_weight", &blockfp8_dequantize_weight);
  m.impl("blockfp8_scaled_mm", &blockfp8_scaled_mm);
  m.impl("blockfp8_dyn_linear", &blockfp8_dyn_linear);
  m.impl("int4_weight_only_linear", &int4_weight_only_linear);
  m.impl("act_prescale", &act_prescale);
  m.impl("int4_prescaled_linear", &int4_prescaled_linear);
  m.impl("int8_weight_only_linear", &int8_weight_only_linear);
  m.impl("int8_quantize_per_token", &int8_quantize_per_token);
  m.impl("int8_scaled_mm", &int8_scaled_mm);
  m.impl("int8_dyn_linear", &int8_dyn_linear);
  m.impl("int8_smooth_quantize_per_token", &int8_smooth_quantize_per_token);
  m.impl("int8_smooth_quantize_static", &int8_smooth_quantize_static);
  m.impl("int8_smooth_dyn_linear", &int8_smooth_dyn_linear);
  m.impl("int8_smooth_static_linear", &int8_smooth_static_linear);
  m.impl("fp8_weight_only_linear", &fp8_weight_only_linear);
  m.impl("fp8_quantize_rows", &fp8_quantize_rows);
  m.impl("fp8_dequantize", &fp8_dequantize);
  m.impl("fp8_scaled_mm", &fp8_scaled_mm);
  m.impl("fp8_dyn_linear", &fp8_dyn_linear);
  m.impl("mx_quantize_rows", &mx_quantize_rows);
  m.impl("mx_scaled_mm", &mx_scaled_mm);
  m.impl("mx_dyn_linear", &mx_dyn_linear);
  m.impl("mxfp4_quantize_rows", &mxfp4_quantize_rows);
  m.impl("mxfp4w_scaled_mm", &mxfp4w_scaled_mm);
  m.impl("mxfp4w_dyn_linear", &mxfp4w_dyn_linear);
}

// Probe for torchao.ops (which ops this library serves).
extern "C" const char* tao_torch_ops_served(void) {
  return "int4_weight_only_linear,int8_weight_only_linear,int8_quantize_per_token,"
         "int8_scaled_mm,int8_dyn_linear";
}

// The float8 weight-only ops served here, listed apart from the integer per-linear set above.
extern "C" const char* tao_torch_ops_served_float8(void) {
  return "fp8_weight_only_linear,fp8_quantize_rows,fp8_dequantize";
}

// The float8 dynamic-activation ops served here, a set of their own for the same reason.
extern "C" const char* tao_torch_ops_served_float8_dyn(void) {
  return "fp8_scaled_mm,fp8_dyn_linear";
}

// The MXFP8 ops served here, again a set of their own.
extern "C" const char* tao_torch_ops_served_mx(void) {
  return "mx_quantize_rows,mx_scaled_mm,mx_dyn_linear";
}

// The blockwise float8 ops served here, a set of their own too.
extern "C" const char* tao_torch_ops_served_blockfp8(void) {
  return "blockfp8_quantize_act,blockfp8_quantize_weight,blockfp8_dequantize_weight,"
         "blockfp8_scaled_mm,blockfp8_dyn_linear";
}

// The NF4 ops served here; they have no Python kernels, so torchao.ops requires them.
extern "C" const char* tao_torch_ops_served_nf4(void) {
  return "nf4_quantize_blocks,nf4_dequantize,nf4_linear";
}

// The FP6 ops served here; they have no Python kernels either.
extern "C" const char* tao_torch_ops_served_fp6(void) {
  return "fp6_quantize_rows,fp6_dequantize,fp6_weight_only_linear";
}

// The MoE ops served here; they have no Python kernels either.
extern "C" const char* tao_torch_ops_served_moe(void) {
  return "moe_route,int4_grouped_linear,moe_combine";
}

// The activation pre-scale ops (AWQ) served here, a set of their own as well.
extern "C" const char* tao_torch_ops_served_awq(void) {
  return "act_prescale,int4_prescaled_linear";
}

// The SmoothQuant ops served here, a set of their own as well.
extern "C" const char* tao_torch_ops_served_smoothquant(void) {
  return "int8_smooth_quantize_per_token,int8_smooth_quantize_static,int8_smooth_dyn_linear,"
         "int8_smooth_static_linear";
}

// The W4A8 ops served here, a set of their own as well.
extern "C" const char* tao_torch_ops_served_w4a8(void) {
  return "rowwise_scaled_linear_cutlass_s8s4,int8_quantize_per_token_f32,"
         "int4_quantize_rows_packed,w4a8_dyn_linear";
}

// The MXFP4-weight ops served here, a set of their own as well.
extern "C" const char* tao_torch_ops_served_mxfp4(void) {
  return "mxfp4_quantize_rows,mxfp4w_scaled_mm,mxfp4w_dyn_linear";
}
