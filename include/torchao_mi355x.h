/*
 * torchao_mi355x.h — C-ABI of the MI355X (gfx950) weight-only quantized linear path.
 *
 * This is the drop-in boundary. Every entry point takes plain device pointers, sizes and a
 * hipStream_t passed as `void*` (NULL = the legacy default stream); no torch types appear here.
 * Each function replaces one call site of the reference (torchao 0.13.0, cited file:line) —
 * the aten/torchao op that the reference's Python layout `impl` functions invoke.
 *
 * Conventions (mirroring the reference op conventions):
 *   - inputs are borrowed, contiguous, row-major; outputs are caller-allocated;
 *   - no entry point allocates, synchronises or copies host<->device, so every call is
 *     hipGraph-capturable (reference compiles decode with mode="reduce-overhead",
 *     torchao/_models/llama/generate.py:865-872);
 *   - bf16 tensors are passed as uint16_t bit patterns;
 *   - return value is TAO_OK (0) or a TAO_ERR_* code; tao_last_error() gives the message for the
 *     calling thread (the reference raises RuntimeError via TORCH_CHECK with the same meaning).
 *
 * int4 weight layout ("gfx950 row-stream layout"):
 *   packed : uint32 [N][K/8]; dword d of row n holds k = 8d..8d+7 with
 *            bits 4i..4i+3 = q[n][8d+2i], bits 16+4i..16+4i+3 = q[n][8d+2i+1]   (i = 0..3)
 *   sz     : bf16 [N][K/group][2] = (scale, zero) interleaved per (row, group)
 *   dequant: w = (q - 8) * scale + zero        (tinygemm float-zero domain)
 *
 * Companion headers of the same library: torchao_mi355x_llama.h (the fused kernels of the
 * end-to-end gpt-fast harness, BASELINE config 4) and torchao_mi355x_tune.h (internal: launch-shape
 * overrides, profiling and diagnostics for bench.py / tests / experiments; not a boundary).
 */
#ifndef TORCHAO_MI355X_H_
#define TORCHAO_MI355X_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  TAO_OK = 0,
  TAO_ERR_INVALID_ARGUMENT = 1, /* shape / alignment / group-size check failed   */
  TAO_ERR_UNSUPPORTED = 2,      /* valid request this build does not implement     */
  TAO_ERR_HIP = 3               /* a HIP runtime call or kernel launch failed      */
};

/* ---- library ------------------------------------------------------------------------------ */

/* Version string of this library ("torchao-mi355x <ver> gfx950"). */
const char* tao_version(void);
/* Message describing the last failed call on this thread ("" if none). */
const char* tao_last_error(void);
/* Number of hipDevices visible (0 if no GPU / runtime unavailable). Never fails. */
int tao_device_count(void);

/* ---- int4 weight-only (tinygemm-equivalent) ----------------------------------------------- */

/* y[M][N] = x[M][K] @ dequant(packed, sz)^T (+ bias[N]), bf16 in/out, fp32 accumulate.
 * Replaces aten._weight_int4pack_mm(x, packed, qGroupSize, qScaleAndZeros) called at
 * torchao/dtypes/uintx/tensor_core_tiled_layout.py:104 (plus the bias add at :112-113).
 * group_size in {32,64,128,256}; K % group_size == 0; M >= 0 (M == 0 is a no-op).
 * x, y: 16-B aligned rows. bias may be NULL. */
int tao_int4wo_linear_bf16(const uint16_t* x, const uint32_t* packed, const uint16_t* sz,
                           const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                           int64_t group_size, void* stream);

/* y[m][k] = bf16( float(x[m][k]) / float(scale[k]) ): the IEEE fp32 quotient (no reciprocal, no
 * fast-math) rounded once to nearest-even; zero, inf, NaN and bf16-subnormal operands and results
 * behave as IEEE division does (a NaN stays a quiet NaN). x, y bf16 [M][K], scale bf16 [K].
 * Replaces `scaled_input_act = input_tensor / scale` of
 * WeightTensorWithLinearActivationScaleMetadata._quantized_linear_op at
 * torchao/quantization/linear_activation_scale.py:61-70 (the AWQ / SmoothQuant equalization
 * scale). K % 8 == 0; x, scale, y 16-B aligned; M >= 0 (M == 0 is a no-op). */
int tao_act_prescale_bf16(const uint16_t* x, const uint16_t* scale, uint16_t* y, int64_t M,
                          int64_t K, void* stream);

/* One token (M <= 1): tao_act_prescale_bf16 of the bf16 token x [K] by act_scale [K] and
 * tao_int4wo_linear_bf16 in one launch: the quotient is formed while the workgroup stages x in
 * LDS. Replaces the division and the F.linear of linear_activation_scale.py:61-70 over an int4
 * TensorCoreTiledLayout weight. Bit-identical to the two calls with the second under
 * the x-in-LDS tuning mode (the same launch shape and summation order). Returns
 * TAO_ERR_INVALID_ARGUMENT for M > 1, for a bias, and for K > 16384 (the prologue holds x in
 * registers): those are the two calls, the caller owning the buffer between them (as for the int8
 * and float8 dynamic paths). act_scale 16-B aligned. */
int tao_int4wo_prescaled_linear_bf16(const uint16_t* x, const uint16_t* act_scale,
                                     const uint32_t* packed, const uint16_t* sz,
                                     const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                                     int64_t K, int64_t group_size, void* stream);

/* 1 when a caller replacing linear_activation_scale.py:61-70 should take
 * tao_int4wo_prescaled_linear_bf16 for this call, 0 when it should take the two calls: one token
 * without a bias at K <= 4096 and N * K <= 2^24 weights. Past those the plain linear's own
 * launch shapes outrun the prologue's shape by more than the saved launch (measured:
 * experiments/bench_awq.py). Never fails. */
int tao_int4wo_prescaled_linear_fused(int64_t M, int64_t N, int64_t K, int has_bias);

/* packed[N][K/8] <- q[N][K] (int32 values 0..15).
 * Replaces aten._convert_weight_to_int4pack(u8, inner_k_tiles) at
 * torchao/dtypes/uintx/tensor_core_tiled_layout.py:279 (device kernel). K % 8 == 0. */
int tao_int4_pack(const int32_t* q, uint32_t* packed, int64_t N, int64_t K, void* stream);

/* packed[N][K/8] <- u8[N][K/2] where u8 = q[:, 0::2] << 4 | q[:, 1::2]
 * (the operand the reference builds at tensor_core_tiled_layout.py:276). */
int tao_int4_pack_u8(const uint8_t* q_u8, uint32_t* packed, int64_t N, int64_t K,
                     void* stream);

/* q[N][K] (int32 0..15) <- packed. Exact inverse of tao_int4_pack.
 * Replaces the identity-matmul recovery in get_plain (tensor_core_tiled_layout.py:465-517). */
int tao_int4_unpack(const uint32_t* packed, int32_t* q, int64_t N, int64_t K, void* stream);

/* w[N][K] bf16 <- dequant(packed, sz).
 * mode 0: bf16((q-8)*s) then bf16(+z) — the two roundings of _dequantize_affine_tinygemm
 *         (torchao/quantization/quant_primitives.py:1019-1023), bit-exact to AQT.dequantize();
 * mode 1: one rounding of fma(q-8, s, z) — the semantics of the reference dequant kernel
 *         (torchao/csrc/cuda/tensor_core_tiled_layout/tensor_core_tiled_layout.cu:184-190). */
int tao_int4_dequant(const uint32_t* packed, const uint16_t* sz, uint16_t* w, int64_t N,
                     int64_t K, int64_t group_size, int mode, void* stream);

/* Host (CPU) versions of pack / unpack for weights that are quantized on the CPU before being
 * moved to the GPU (quantize_ on a CPU model). Plain C++; identical bytes to the device kernels. */
int tao_int4_pack_host(const int32_t* q, uint32_t* packed, int64_t N, int64_t K);
int tao_int4_unpack_host(const uint32_t* packed, int32_t* q, int64_t N, int64_t K);

/* ---- reference tile-format compat (torchao::*_tensor_core_tiled_layout) ------------------- */

/* The reference tile format: int32 [N/8][K/(ikt*16)][32][ikt/2], inner_k_tiles (ikt) in {2,4,8}.
 * Two nibble maps share that shape (tile_format):
 *   0 = CUDA: the semantics of the reference's own kernels (tensor_core_tiled_layout.cu:131-215),
 *       i.e. what aten._convert_weight_to_int4pack writes on CUDA builds of PyTorch;
 *   1 = ROCm: what aten._convert_weight_to_int4pack writes on PyTorch-ROCm (gfx950, measured:
 *       experiments/probe_aten_tile_map.py, tests/golden/aten_tile_map_rocm.npz), the bytes seen
 *       flat as [N/16][K/(ikt*16)][64][ikt/2] for wave64 lanes; needs N % 16 == 0.
 * A checkpoint saved by torchao holds whichever format its producing build wrote. */

/* out[N][K] int32 <- tile-format packed_w.
 * Replaces torchao::unpack_tensor_core_tiled_layout (torchao/ops.py:255-296,
 * tensor_core_tiled_layout.cu:320-368). */
int tao_unpack_tensor_core_tiled_layout(const int32_t* packed_w, int32_t* out, int64_t N,
                                        int64_t K, int64_t inner_k_tiles, int tile_format,
                                        void* stream);

/* The same on the host (checkpoint conversion of CPU-resident state dicts). */
int tao_unpack_tensor_core_tiled_layout_host(const int32_t* packed_w, int32_t* out, int64_t N,
                                             int64_t K, int64_t inner_k_tiles, int tile_format);

/* out[N][K] bf16 <- fma(q-8, s, z) with scales_and_zeros [K/g][N][2] bf16 (tinygemm packing,
 * torchao/quantization/utils.py:395-409). Replaces torchao::dequantize_tensor_core_tiled_layout
 * (torchao/ops.py:299-377, tensor_core_tiled_layout.cu:223-316). */
int tao_dequantize_tensor_core_tiled_layout(const int32_t* packed_w,
                                            const uint16_t* scales_and_zeros, uint16_t* out,
                                            int64_t N, int64_t K, int64_t group_size,
                                            int64_t inner_k_tiles, int tile_format,
                                            void* stream);

/* Tile-format packer (the inverse of the unpack above): packed_w <- q[N][K] int32; with
 * tile_format 1 bit-identical to PyTorch-ROCm's aten._convert_weight_to_int4pack (the call at
 * torchao/dtypes/uintx/tensor_core_tiled_layout.py:279). K % (ikt*16) == 0. */
int tao_pack_tensor_core_tiled_layout(const int32_t* q, int32_t* packed_w, int64_t N, int64_t K,
                                      int64_t inner_k_tiles, int tile_format, void* stream);

/* ---- int8 weight-only ---------------------------------------------------------------------- */

/* y[M][N] = bf16( bf16(x @ w^T) * scale[n] ) (+ bias), w int8 [N][K], scale bf16 [N].
 * Replaces torch.mm(x, w.t().to(bf16)) * scale at torchao/dtypes/uintx/plain_layout.py:256-266. */
int tao_int8wo_linear_bf16(const uint16_t* x, const int8_t* w, const uint16_t* scale,
                           const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                           void* stream);

/* ---- float8 (e4m3fn) weight-only ------------------------------------------------------------ */

/* y[M][N] = bf16( (sum_k x[m][k] * f(w[n][k])) * scale[n] ) (+ bias[n], rounded to bf16 again),
 * w uint8 [N][K] = OCP e4m3fn codes (torch.float8_e4m3fn), f their exact decode, scale f32 [N]
 * per output row; the sum and the scale product are formed in fp32. The scale is applied once
 * per output; the reference rounds bf16(f(w) * scale) per weight, which is the same number
 * whenever that product is a bf16 number (e.g. power-of-two scales) and has more roundings
 * otherwise. A NaN code (0x7F / 0xFF) makes its output column NaN.
 * Replaces F.linear(x, weight.dequantize(), bias) in _linear_fp_act_fp8_weight_impl at
 * torchao/dtypes/floatx/float8_layout.py:391-396, which rebuilds a bf16 copy of W on every call.
 * K % 32 == 0; M >= 0 (M == 0 is a no-op). x, w: 16-B aligned. bias may be NULL. */
int tao_fp8wo_linear_bf16(const uint16_t* x, const uint8_t* w, const float* scale,
                          const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                          void* stream);

/* Fused per-row e4m3fn weight quantizer (Float8WeightOnlyConfig version 1 on bf16 weights), one
 * pass per row of w [rows][K] bf16: scale[r] = float(bf16(amax|w[r]| / 448)) (the bf16 rounding is
 * the one the reference's division of the bf16 amax tensor makes; the value is kept in fp32),
 * q = e4m3fn_rne(clamp(float(w) / scale[r], -448, 448)), both true divisions. No eps, as in the
 * reference: an all-zero row gets scale 0.0 and NaN codes. K % 8 == 0. Replaces
 * _choose_scale_float8 + _quantize_affine_float8 (torchao/quantization/quant_primitives.py:2175-2221,
 * 2274-2293) behind to_affine_quantized_floatx, byte for byte. */
int tao_fp8_quantize_rows_bf16(const uint16_t* w, uint8_t* q, float* scale, int64_t rows,
                               int64_t K, void* stream);

/* w[N][K] bf16 <- bf16(f(q[n][k]) * scale[n]) (product in fp32; NaN codes give NaN). K % 8 == 0.
 * Replaces _dequantize_affine_float8 (torchao/quantization/quant_primitives.py:2298-2312), bit-exact
 * to AffineQuantizedTensor.dequantize() of a Float8Layout weight. */
int tao_fp8_dequant_bf16(const uint8_t* q, const float* scale, uint16_t* w, int64_t N, int64_t K,
                         void* stream);

/* ---- float8 (e4m3fn) dynamic activation x float8 weight, per-row scales --------------------- */

/* y[m][n] = bf16( fp32(fp32(acc * xs[m]) * ws[n]) + fp32(bias[n]) ),
 * acc[m][n] = sum_k f(xq[m][k]) * f(wq[n][k]) in fp32 (every product of two e4m3fn values is an
 * fp32 number): one rounding to bf16, with or without bias, as a row-wise _scaled_mm epilogue is
 * specified. xq uint8 [M][K] and wq uint8 [N][K] are OCP e4m3fn codes, xs f32 [M] the per-token
 * and ws f32 [N] the per-row scales, bias bf16 [N] or NULL. A NaN code (an all-zero token or
 * weight row quantises to scale 0.0 and NaN codes) makes its output row / column NaN.
 * Replaces the torch._scaled_mm call of _linear_fp8_act_fp8_weight_impl at
 * torchao/dtypes/floatx/float8_layout.py:329-367. K % 16 == 0 (the reference's _fp8_mm_compat),
 * any N, M >= 0 (M == 0 is a no-op); xq, wq: 16-B aligned, each operand below 4 GiB. */
int tao_fp8_scaled_mm_bf16(const uint8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                           const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                           void* stream);

/* One token (M <= 1): tao_fp8_quantize_rows_bf16 of the bf16 token x [K] and the product above in
 * one launch, bit-identical to the two calls. Replaces _input_activation_quant_func_fp8
 * (torchao/quantization/quant_api.py:1533-1571) followed by _linear_fp8_act_fp8_weight_impl
 * (torchao/dtypes/floatx/float8_layout.py:329-367). More tokens are the two calls, the caller
 * owning the code buffer between them (as for the int8 dynamic path). K % 16 == 0, K <= 65536. */
int tao_fp8_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const float* ws,
                            const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                            void* stream);

/* ---- MXFP8: e4m3fn codes with one E8M0 scale byte per 32-element block (csrc/mx_fp8.hip) ------ */

/* Block quantizer of x [M][K] bf16, FLOOR mode: per block of 32 consecutive k,
 *   byte = clamp((biased fp32 exponent field of amax|x|) - 8, 0, ..), 255 if the amax is NaN,
 *   q    = e4m3fn_rne(clamp(float(x) / d, -448, 448)), d the fp32 number with `byte` as exponent
 *          field, at least 2^-126 (an all-zero block: byte 0, codes 0).
 * q uint8 [M][K] codes, scale uint8 [M][K/32] E8M0 bytes. Replaces to_mx
 * (torchao/prototype/mx_formats/mx_tensor.py:133-326, elem_dtype float8_e4m3fn, block_size 32,
 * ScaleCalculationMode.FLOOR), byte for byte. K % 32 == 0; M == 0 is a no-op; x, q 16-B aligned,
 * M * K below 4 Gi. */
int tao_mx_quantize_rows_bf16(const uint16_t* x, uint8_t* q, uint8_t* scale, int64_t M, int64_t K,
                              void* stream);

/* y[m][n] = bf16( acc[m][n] + fp32(bias[n]) ),
 * acc[m][n] = sum_b 2^(xs[m][b]-127) 2^(ws[n][b]-127) sum_{k in block b} f(xq[m][k]) f(wq[n][k])
 * in fp32: one rounding to bf16. xq uint8 [M][K], wq uint8 [N][K] e4m3fn codes; xs uint8 [M][K/32],
 * ws uint8 [N][K/32] E8M0 bytes (255 is NaN); bias bf16 [N] or NULL. Replaces the block-scaled
 * torch._scaled_mm call of _addmm_mx_dispatch (torchao/prototype/mx_formats/mx_ops.py), which the
 * reference has for sm100 only. K % 32 == 0, any N, M >= 0 (M == 0 is a no-op); xq, wq: 16-B
 * aligned, and xs, ws 8-B aligned where K % 256 == 0; each operand below 4 GiB. */
int tao_mx_scaled_mm_bf16(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq,
                          const uint8_t* ws, const uint16_t* bias, uint16_t* y, int64_t M,
                          int64_t N, int64_t K, void* stream);

/* One token (M <= 1): tao_mx_quantize_rows_bf16 of the bf16 token x [K] and the product above in
 * one launch, bit-identical to the two calls. Replaces MXTensor.to_mx on the activation followed by
 * _addmm_mx_dispatch (torchao/prototype/mx_formats/mx_ops.py). More tokens are the two calls, the
 * caller owning the code and scale buffers between them. K % 32 == 0, K <= 65536. */
int tao_mx_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const uint8_t* ws,
                           const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                           void* stream);

/* ---- MXFP4 weights under MXFP8 activations: e2m1 codes, two per byte, one E8M0 scale byte per
 * 32-element block (csrc/mx_fp4.hip). Storage is the reference's: element 2 j of a row in the HIGH
 * nibble of byte j, element 2 j + 1 in the low nibble. ------------------------------------------ */

/* Block quantizer of x [M][K] bf16 to e2m1, FLOOR mode: per block of 32 consecutive k,
 *   byte = max((biased fp32 exponent field of amax|x|) - 2, 0), 255 if the amax is NaN,
 *   q    = e2m1_rne(float(x) / d) saturating at +-6 (no clamp before the cast: +-inf -> +-6), d the
 *          fp32 number with `byte` as exponent field, at least 2^-126.
 * q uint8 [M][K/2] packed codes, scale uint8 [M][K/32] E8M0 bytes. Replaces to_mx
 * (torchao/prototype/mx_formats/mx_tensor.py:133-326, elem_dtype float4_e2m1fn_x2, block_size 32,
 * ScaleCalculationMode.FLOOR) with f32_to_f4_unpacked and pack_uint4, byte for byte (the sign bit
 * of the nibble written for a NaN input is the input's). K % 32 == 0; M == 0 is a no-op; x, q 16-B
 * aligned, M * K below 2^32. */
int tao_mxfp4_quantize_rows_bf16(const uint16_t* x, uint8_t* q, uint8_t* scale, int64_t M,
                                 int64_t K, void* stream);

/* y[m][n] = bf16( acc[m][n] + fp32(bias[n]) ),
 * acc[m][n] = sum_b 2^(xs[m][b]-127) 2^(ws[n][b]-127) sum_{k in block b} e4m3(xq[m][k]) e2m1(wq[n][k])
 * in fp32: one rounding to bf16. xq uint8 [M][K] e4m3fn codes, wq uint8 [N][K/2] packed e2m1 codes;
 * xs uint8 [M][K/32], ws uint8 [N][K/32] E8M0 bytes (255 is NaN); bias bf16 [N] or NULL. Replaces
 * the emulated branch of _addmm_mx_dispatch (torchao/prototype/mx_formats/mx_ops.py:144-156:
 * to_dtype of both operands and a bf16 addmm) for an e4m3fn activation and an e2m1 weight.
 * K % 32 == 0, any N, M >= 0 (M == 0 is a no-op); xq, wq 16-B aligned, and xs, ws 8-B aligned where
 * K % 256 == 0; M * K and N * K below 2^32. */
int tao_mxfp4w_scaled_mm_bf16(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq,
                              const uint8_t* ws, const uint16_t* bias, uint16_t* y, int64_t M,
                              int64_t N, int64_t K, void* stream);

/* One token (M <= 1): tao_mx_quantize_rows_bf16 of the bf16 token x [K] (e4m3fn blocks) and the
 * product above in one launch, bit-identical to the two calls. Replaces MXTensor.to_mx on the
 * activation followed by _addmm_mx_dispatch (torchao/prototype/mx_formats/mx_ops.py). More tokens
 * are the two calls. K % 32 == 0, K <= 65536. */
int tao_mxfp4w_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const uint8_t* ws,
                               const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                               void* stream);

/* ---- Blockwise float8 (torchao.prototype.blockwise_fp8_inference): e4m3fn codes, one fp32 scale
 * per 1 x 128 block of the activation and per 128 x 128 block of the weight (csrc/block_fp8.hip).
 * K % 128 == 0 throughout; NB = ceil(N / 128). -------------------------------------------------- */

/* Activation quantizer of x [M][K] bf16, per block of 128 consecutive k of one row:
 *   amax = max |x| (a NaN element ignored, 0 if there is no number), s = amax / 448 (correctly
 *   rounded fp32, subnormals kept), q = e4m3fn_rne(float(x) / s), and q = e4m3fn_rne(float(x))
 *   where amax == 0 (an all-zero block: zero codes, scale 0; the reference stores NaN codes).
 * q uint8 [M][K] codes, scale fp32 [M][K/128]. Replaces fp8_blockwise_act_quant
 * (torchao/prototype/blockwise_fp8_inference/blockwise_quantization.py), byte for byte but for the
 * all-zero block. M == 0 is a no-op; x 16-B, q 8-B aligned, M * K below 2^32. */
int tao_blockfp8_quantize_act_bf16(const uint16_t* x, uint8_t* q, float* scale, int64_t M,
                                   int64_t K, void* stream);

/* Weight quantizer of w [N][K] bf16: the same arithmetic per block of up to 128 rows x 128 k (the
 * last row block takes its amax over the rows that exist). q uint8 [N][K], scale fp32 [NB][K/128].
 * Replaces fp8_blockwise_weight_quant, which needs N % 128 == 0. */
int tao_blockfp8_quantize_weight_bf16(const uint16_t* w, uint8_t* q, float* scale, int64_t N,
                                      int64_t K, void* stream);

/* out[n][k] = float(q[n][k]) * scale[n / 128][k / 128] in fp32, stored as fp32 (out_bf16 == 0) or
 * rounded once to bf16 (out_bf16 == 1). Replaces fp8_blockwise_weight_dequant. q, out 16-B
 * aligned. */
int tao_blockfp8_dequant_weight(const uint8_t* q, const float* scale, void* out, int64_t N,
                                int64_t K, int out_bf16, void* stream);

/* y[m][n] = bf16( sum_b P[m][n][b] * (xs[m][b] * ws[n / 128][b]) + fp32(bias[n]) ), P the fp32 dot
 * product of the 128 code pairs of block b; fp32 throughout (each term one fma on the rounded
 * factor), one rounding to bf16, the bias a separate add. xq uint8 [M][K], wq uint8 [N][K] e4m3fn
 * codes; xs fp32 [M][K/128], ws fp32 [NB][K/128]; bias bf16 [N] or NULL. Replaces
 * blockwise_fp8_gemm. Any N, M >= 0 (M == 0 is a no-op); xq, wq 16-B aligned; each operand below
 * 4 GiB. No scale outside the two arrays is read. */
int tao_blockfp8_scaled_mm_bf16(const uint8_t* xq, const float* xs, const uint8_t* wq,
                                const float* ws, const uint16_t* bias, uint16_t* y, int64_t M,
                                int64_t N, int64_t K, void* stream);

/* One token (M <= 1): tao_blockfp8_quantize_act_bf16 of the bf16 token x [K] and the product above
 * in one launch, bit-identical to the two calls. Replaces BlockwiseQuantLinear.forward at one
 * token. More tokens are the two calls. K <= 65536. */
int tao_blockfp8_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const float* ws,
                                 const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                                 int64_t K, void* stream);

/* ---- int8 dynamic activation x int8 weight -------------------------------------------------- */

/* Per-token symmetric reduced-range int8 quantization of x [M][K] bf16:
 *   s[m] = max(bf16(amax(|x[m]|) / 127), bf16(1e-5)); q = clamp(rne(bf16(x * bf16(1/s))), -127, 127)
 * Replaces _int8_symm_per_token_reduced_range_quant (torchao/quantization/quant_api.py:1258-1273). */
int tao_int8_quant_per_token(const uint16_t* x, int8_t* q, uint16_t* scale, int64_t M,
                             int64_t K, void* stream);

/* y[M][N] = bf16( bf16( bf16(xq @ wq^T) * xs[m] ) * ws[n] ) (+ bias), exact int32 accumulation.
 * Replaces int_scaled_matmul + the weight-scale epilogue at
 * torchao/dtypes/uintx/plain_layout.py:294-315 and torchao/kernel/intmm.py:108-143. */
int tao_int8_scaled_mm_bf16(const int8_t* xq, const uint16_t* xs, const int8_t* wq,
                            const uint16_t* ws, const uint16_t* bias, uint16_t* y, int64_t M,
                            int64_t N, int64_t K, void* stream);

/* One token (M <= 1) through both steps above in ONE launch: every workgroup quantises x [K]
 * bf16 per token into LDS (tao_int8_quant_per_token's arithmetic) and runs the int8 x int8 GEMV
 * on it. Bit-identical to tao_int8_quant_per_token + tao_int8_scaled_mm_bf16 (K % 16 == 0,
 * K <= 65536). Replaces LinearActivationQuantizedTensor's quantize-then-F.linear for the default
 * Int8DynamicActivationInt8WeightConfig recipe at decode (linear_activation_quantized_tensor.py
 * _quantized_linear_op; quant_api.py:1258-1273 + plain_layout.py:294-315). */
int tao_int8_dyn_linear_bf16(const uint16_t* x, const int8_t* wq, const uint16_t* ws,
                             const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                             void* stream);

/* SmoothQuant activation quantization of x [M][K] bf16 in one launch: t = bf16(x / smooth)
 * (tao_act_prescale_bf16's bits; smooth bf16 [K]; t is never written), then
 *   act_scale == NULL (dynamic): s[m] = max(bf16(amax(|t[m]|) / 127), 2^-7), the default eps of
 *     choose_qparams_affine for bf16, NOT the 1e-5 of tao_int8_quant_per_token;
 *   act_scale != NULL (static): s[m] = act_scale[0], a per-tensor bf16 scale in device memory,
 *     written to every row of scale so tao_int8_scaled_mm_bf16 takes it as it is;
 *   q = clamp(rne(bf16(t * bf16(1/s))), -127, 127) (values past the calibrated range saturate).
 * Replaces the division of linear_activation_scale.py:61-70 followed by
 * _ActQuantizer.dynamic_quantize / .static_quantize (torchao/prototype/smoothquant/api.py:133-155:
 * to_affine_quantized_intx / to_affine_quantized_intx_static, ~8 eager kernels).
 * K % 16 == 0, K <= 65536; x, smooth 16-B aligned, q 8-B aligned; q int8 [M][K], scale bf16 [M]. */
int tao_int8_smooth_quant_bf16(const uint16_t* x, const uint16_t* smooth,
                               const uint16_t* act_scale, int8_t* q, uint16_t* scale, int64_t M,
                               int64_t K, void* stream);

/* One token (M <= 1): tao_int8_smooth_quant_bf16 and tao_int8_scaled_mm_bf16 in ONE launch (the
 * division and the quantisation in the GEMV's prologue, under its first weight loads), bit-identical
 * to the two calls. act_scale as above (NULL = dynamic). Replaces F.linear on SmoothQuant's
 * converted weight at decode (torchao/prototype/smoothquant/api.py:176-231,
 * linear_activation_scale.py:61-70). Served up to K = 16384 on the default launch shapes (the
 * token and the factor fit the prologue's registers); a longer K returns the argument error and
 * is the two calls, the caller owning q and scale between them. */
int tao_int8_smooth_linear_bf16(const uint16_t* x, const uint16_t* smooth,
                                const uint16_t* act_scale, const int8_t* wq, const uint16_t* ws,
                                const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                                int64_t K, void* stream);

/* 1 when a caller replacing the SmoothQuant linear (api.py:176-231) should take
 * tao_int8_smooth_linear_bf16 for this call, 0 when it should take the two calls: one token whose
 * K the one launch serves, and for the static recipe (is_static != 0) K <= 8192, past which the
 * two calls are faster (measured: experiments/bench_smoothquant.py). Never
 * fails. */
int tao_int8_smooth_linear_fused(int64_t M, int64_t N, int64_t K, int is_static);

/* Device-side faults of the decode kernels since the last call, read and cleared (synchronous:
 * call outside graph capture). bits & 1: a KV-cache position outside [0, T) reached
 * tao_rope_kv_bf16 / tao_int4wo_decode_bf16's rope_kv epilogue; those launches wrote no cache
 * row and tao_attn_decode_bf16 clamped its key count to T. (The reference's index_put KV cache
 * device-asserts in this case, torchao/_models/llama/model.py KVCache.update.) bits & 2: a split-K
 * reducer of the prefill GEMMs timed out waiting for its publishers; that output tile was not
 * written (never expected; the ticket is left consistent for later launches). */
int tao_decode_status(int* bits);

/* Fused int4 weight quantizer (Int4WeightOnlyConfig's from_hp_to_intx in one pass):
 * w [rows][K] bf16 -> packed [rows][K/8] (row-stream nibbles, as tao_int4_pack) and
 * scales_and_zeros [rows][K/g][2] bf16, per group of g: s = clamp(bf16(bf16(max-min)/15), eps),
 * z = bf16(min + 8 s), q = clamp(rint(bf16(bf16(w - bf16(z - 8 s)) / s)), 0, 15), each step
 * rounded to bf16 as the reference's torch ops do (_choose_qparams_affine_tinygemm
 * quant_primitives.py:1238-1307, _quantize_affine_tinygemm :461-573). g in {32,64,128,256}. */
int tao_int4_quantize_bf16(const uint16_t* w, uint32_t* packed, uint16_t* scales_and_zeros,
                           int64_t rows, int64_t K, int64_t group_size, float eps, void* stream);

/* Fused HQQ int4 weight quantizer (Int4WeightOnlyConfig(use_hqq=True)): replaces
 * _choose_qparams_and_quantize_affine_hqq with optimize_weights_proximal_legacy and
 * _convert_to_affinequantized_format (quant_primitives.py:1901-2111, called from
 * affine_quantized_tensor.py:252-288) and the layout's pack. In fp32, the reference's CPU
 * arithmetic (its GPU path iterates in fp16). Per group of g:
 * scale = min((1 / (max - min)) * 15, 2e4) (torch's scalar / tensor is reciprocal * scalar),
 * zero = rint(-min * scale), then at most 20 proximal updates of zero alone (lp 0.7, beta 10,
 * kappa 1.01) with the reference's early stop on the mean |W - Wr| of the whole tensor, decided
 * on the device: three launches on `stream`, no host copy or synchronisation (capturable).
 * w [rows][K] bf16 -> packed [rows][K/8] and scales_and_zeros [rows][K/g][2] bf16 as
 * tao_int4_quantize_bf16 writes them: q = clamp(rint(w * scale + zero), 0, 15),
 * s = bf16(1 / scale), z = bf16((8 - zero) * (1 / scale)), so w ~= (q - 8) s + z.
 * iters_run: one int32 on the device, the iterations run (1..20; 0 for an empty tensor).
 * scratch: device memory owned by the caller, 8-B aligned, tao_int4_hqq_scratch_bytes(rows, K)
 * bytes; contents are overwritten, nothing is kept between calls. g in {32,64,128,256},
 * K % g == 0; w 16-B aligned. Results are bit-equal from run to run. */
int tao_int4_hqq_quantize_bf16(const uint16_t* w, uint32_t* packed, uint16_t* scales_and_zeros,
                               int32_t* iters_run, void* scratch, int64_t rows, int64_t K,
                               int64_t group_size, void* stream);

/* Scratch of tao_int4_hqq_quantize_bf16 (the per-workgroup error sums that stand in for the
 * reference's float(torch.abs(W_f - W_r).mean()), quant_primitives.py:1957):
 * ceil(rows * (K / 8) / 256) * 20 * 8 bytes; 0 for an empty tensor. Never fails. */
int64_t tao_int4_hqq_scratch_bytes(int64_t rows, int64_t K);

/* Fused symmetric per-row int8 weight quantizer (Int8WeightOnlyConfig /
 * Int8DynamicActivationInt8WeightConfig weights; choose_qparams_affine SYMMETRIC +
 * quantize_affine, quant_primitives.py): s[r] = bf16(max(bf16(max|w[r]| / 127.5), eps)),
 * q = clamp(rint(bf16(w * bf16(1 / s))), -128, 127). K % 8 == 0. Replaces the torch-op
 * quantisation behind to_affine_quantized_intx in _int8_weight_only_quantize_tensor
 * (torchao/quantization/quant_api.py:1223-1240) for bf16 GPU weights. */
int tao_int8_quantize_rows_bf16(const uint16_t* w, int8_t* q, uint16_t* scale, int64_t rows,
                                int64_t K, float eps, void* stream);

/* ---- W4A8: int8 dynamic activation x int4 weight packed two per byte (csrc/w4a8.hip) ----------
 * Int8DynamicActivationInt4WeightConfig(layout=CutlassInt4PackedLayout()): per-token symmetric
 * int8 activations, per-output-channel symmetric int4 weights, both with fp32 scales and no zero
 * point. Weight storage is the reference's: byte j of a row holds element 2 j in its low nibble
 * and element 2 j + 1 in its high nibble, two's complement. */

/* Per-token quantizer of x [M][K] bf16: s[m] = max(fp32(bf16(amax|x[m]| / 127.5)), 2^-23),
 * q = clamp(rne(fp32(x) * (1 / s[m])), -128, 127), the reciprocal and the product in fp32. An
 * all-zero token gets codes 0. q int8 [M][K], scale fp32 [M]. Replaces _int8_symm_cutlass_quant
 * (torchao/quantization/quant_api.py:1299-1308: to_affine_quantized_intx, ~8 eager kernels), byte
 * for byte. K % 8 == 0; x 16-B aligned, q 8-B aligned. */
int tao_int8_quant_per_token_f32(const uint16_t* x, int8_t* q, float* scale, int64_t M, int64_t K,
                                 void* stream);

/* Per-row weight quantizer of w [rows][K] bf16 with packed output:
 * s[r] = max(fp32(bf16(amax|w[r]| / 7.5)), 2^-23), q = clamp(rne(fp32(w) * (1 / s[r])), -8, 7),
 * two codes per byte as above. An all-zero row gets zero bytes. q uint8 [rows][K/2], scale fp32
 * [rows]. Replaces _int4_symm_cutlass_quant (torchao/quantization/quant_api.py:1311-1323) and
 * Int4PackedTensorImpl.from_plain (torchao/dtypes/uintx/cutlass_int4_packed_layout.py:131-144),
 * byte for byte. K % 8 == 0; w 16-B aligned, q 4-B aligned. */
int tao_int4_quantize_rows_packed_bf16(const uint16_t* w, uint8_t* q, float* scale, int64_t rows,
                                       int64_t K, void* stream);

/* y[m][n] = bf16( fp32(fp32(fp32(acc) * xs[m]) * ws[n]) + fp32(bias[n]) ),
 * acc[m][n] = sum_k xq[m][k] * wq[n][k] in exact int32: one rounding to bf16, with or without
 * bias. xq int8 [M][K], xs f32 [M], wq uint8 [N][K/2] packed int4 codes, ws f32 [N], bias bf16 [N]
 * or NULL. The result does not depend on the route (GEMV up to M = 2, and up to M = 4 for weights
 * of at most 32 Mi elements; int8 MFMA above) or on any launch shape: every partial sum is an
 * integer. Replaces
 * torchao::rowwise_scaled_linear_cutlass_s8s4 behind _linear_int8_act_int4_weight_cutlass_impl
 * (torchao/dtypes/uintx/cutlass_int4_packed_layout.py:176-189), a CUTLASS kernel the reference
 * builds for sm80 only. K % 32 == 0, K < 131072 (the weights enter the dot products as int8 x 16;
 * the factor leaves the int32 sum exactly), any N, M >= 0 (M == 0 is a no-op); xq, wq 16-B aligned,
 * each operand below 4 GiB. */
int tao_w4a8_scaled_mm_bf16(const int8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                            const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                            void* stream);

/* One token (M <= 1): tao_int8_quant_per_token_f32 of the bf16 token x [K] and the product above
 * in one launch, bit-identical to the two calls. Replaces LinearActivationQuantizedTensor's
 * quantize-then-F.linear for this recipe at decode (_int8_symm_cutlass_quant,
 * torchao/quantization/quant_api.py:1299-1308, then cutlass_int4_packed_layout.py:176-189). More
 * tokens are the two calls, the caller owning the code buffer between them. K % 32 == 0,
 * K <= 65536. */
int tao_w4a8_dyn_linear_bf16(const uint16_t* x, const uint8_t* wq, const float* ws,
                             const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                             void* stream);

/* ---- NF4 (QLoRA) weight-only (csrc/nf4.hip; torchao/dtypes/nf4tensor.py NF4Tensor) -------------
 * The flattened weight is cut into blocks of 64; block b has a double-quantized scaler
 *   s[b] = bf16( bf16( float(qscalers[b]) / qfactor[b / 256] ) + mean ),
 * qscalers int8 [numel / 64], qfactor bf16 [ceil(numel / 16384)], mean one bf16, and a weight is
 *   w^ = bf16( levels[code] * s[b] ),
 * levels the tensor's own 16 bf16 values (never a compiled-in table), codes uint8 [numel / 2] with
 * element 2 j in the HIGH nibble of byte j. Every operation is the eager torch op on bf16 tensors:
 * evaluated in fp32, rounded to bf16 once. */

/* First stage of NF4Tensor.from_tensor for w bf16 [numel], numel % 64 == 0, in one read:
 * absmax[b] = max |w| over block b (bf16; a NaN in the block gives NaN) and the packed codes,
 *   v = bf16(w / absmax[b]), code = first j minimising bf16(|bf16(v - levels[j])|),
 * a NaN v (an all-zero block: 0 / 0) taking code 0 as torch.min returns the first NaN. Replaces
 * get_block_absmax and convert_to_norm_float_weight (torchao/dtypes/nf4tensor.py:544-561, 790-827),
 * whose quantize_tensor_nearest materialises a numel x 16 difference tensor in chunks; the
 * double quantization of absmax (n_blocks values) stays torch ops on the device. w 16-B aligned,
 * codes 4-B aligned. */
int tao_nf4_quantize_blocks_bf16(const uint16_t* w, const uint16_t* levels, uint8_t* codes,
                                 uint16_t* absmax, int64_t numel, void* stream);

/* w[i] = w^ of element i for a flat tensor of numel weights (numel % 64 == 0; blocks may straddle
 * the rows of a 2-D weight), bit-exact to NF4Tensor.get_original_weight (nf4tensor.py:829-855).
 * codes and levels 4-B aligned, w 16-B aligned. */
int tao_nf4_dequant_bf16(const uint8_t* codes, const int8_t* qscalers, const uint16_t* qfactor,
                         const uint16_t* mean, const uint16_t* levels, uint16_t* w, int64_t numel,
                         void* stream);

/* y[m][n] = bf16( sum_k x[m][k] * w^[n][k] ), the sum in fp32 over the bf16-rounded w^; with a
 * bias a second rounding, bf16(y + bias[n]) (the reference's out + bias). x bf16 [M][K], the
 * weight [N][K] row-major in the flat layout above, y bf16 [M][N]. The decode GEMV
 * (nf4_gemv_kernel): one launch up to 8 tokens, a sequence of 8-token launches beyond. The op
 * torchao::nf4_linear calls it up to M = 4 and dequantizes + matmuls above
 * (tao_nf4_linear_route, torchao_mi355x_tune.h). K % 64 == 0 (a row is whole blocks); any N, with
 * ceil(N K / 16384) factors; M >= 0 (M == 0 is a no-op); x and codes 16-B aligned. Replaces
 * F.linear(x, weight.to(x.dtype)) of LinearNF4.forward (nf4tensor.py:1037-1042), which rebuilds and
 * re-reads a bf16 copy of W on every call. */
int tao_nf4_linear_bf16(const uint16_t* x, const uint8_t* codes, const int8_t* qscalers,
                        const uint16_t* qfactor, const uint16_t* mean, const uint16_t* levels,
                        const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                        void* stream);

/* ---- FP6 weight-only (csrc/fp6.hip; FPXWeightOnlyConfig, torchao/dtypes/floatx) ---------------
 * (ebits, mbits) = (3, 2) or (2, 3), the OCP FP6 formats (no inf, no NaN; max 28 / 7.5); any other
 * pair is refused. A weight [N][K] is codes uint32 [N][K * 6 / 32], code k of a row at bits
 * 6 k .. 6 k + 5 of the row's little-endian bit stream (32 codes = 6 dwords), and one bf16 scale
 * per row. */

/* Per row, in one read of w bf16 [rows][K], K % 32 == 0:
 *   scale = bf16( max(amax|w|, 1e-12) / max_normal )          the IEEE fp32 quotient
 *   code  = round-to-nearest-even of float(w) / float(scale), saturated at +-max_normal,
 *           subnormals and the sign of zero kept
 * (the reference's _choose_qparams_affine_floatx + _quantize_affine_floatx,
 * torchao/quantization/quant_primitives.py:2114-2158, bit for bit on finite rows, straight into
 * the native storage: replaces them and pack_tc_floatx of floatx_tensor_core_layout.py:210-213).
 * A NaN weight does not enter amax and takes an unspecified code; an inf gives scale = inf
 * and unspecified codes. w 16-B aligned, codes 8-B aligned. */
int tao_fp6_quantize_rows_bf16(const uint16_t* w, uint32_t* codes, uint16_t* scale, int64_t rows,
                               int64_t K, int ebits, int mbits, void* stream);

/* w[n][k] = bf16( float(value(code[n][k])) * float(scale[n]) ), the reference's
 * _dequantize_affine_floatx (quant_primitives.py:2161-2171) to bf16 bit for bit. K % 32 == 0; codes 8-B aligned, w 16-B aligned. */
int tao_fp6_dequant_bf16(const uint32_t* codes, const uint16_t* scale, uint16_t* w, int64_t N,
                         int64_t K, int ebits, int mbits, void* stream);

/* y[m][n] = bf16( float(sum_k x[m][k] * value(code[n][k])) * float(scale[n]) ), the sum in fp32;
 * with a bias a second rounding, bf16(y + bias[n]). x bf16 [M][K], y bf16 [M][N]. The decode GEMV
 * (fp6wo_gemv_kernel): one launch up to 8 tokens, a sequence of 8-token launches beyond. The op
 * torchao::fp6_weight_only_linear calls it up to the boundary of tao_fp6_linear_route
 * (torchao_mi355x_tune.h) and dequantizes + matmuls above. K % 64 == 0; any N >= 0; M >= 0 (M == 0
 * is a no-op); x and codes 16-B aligned. Replaces quant_llm_linear of
 * _linear_f16_bf16_act_floatx_weight_impl (torchao/dtypes/floatx/floatx_tensor_core_layout.py:
 * 641-666), a CUDA kernel the reference's ROCm build does not compile. */
int tao_fp6_linear_bf16(const uint16_t* x, const uint32_t* codes, const uint16_t* scale,
                        const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                        int ebits, int mbits, void* stream);

/* ---- MoE expert FFN over many tokens (csrc/moe_gemm.hip; torchao/prototype/moe_quant) ----------
 * T tokens, A = top-k, R = T * A token activations, E experts. E <= 256, A <= 8. None of the three
 * kernels waits on another workgroup; each result is a pure function of its inputs. */

/* Stable counting sort of expert_indices int64 [R] (flat index = token * A + slot): offsets int32
 * [E + 1], offsets[e] = number of activations whose expert is < e, offsets[E] = R; order int32 [R],
 * order[p] = the flat index at sorted position p, ascending within an expert (argsort(stable=True));
 * inverse int32 [R], inverse[order[p]] = p. An index outside [0, E) is clamped and reported by
 * tao_decode_status (bits & 4). One launch, no global atomics. R % A == 0, R < 2^24. Replaces the
 * argsort / div / floor / histc / cumsum of ConditionalFeedForwardAOQuantizable's many-token branch
 * (prototype/moe_quant/quantizable_moe_modules.py:117-136) and its per-expert host-side slices. */
int tao_moe_route(const int64_t* expert_indices, int64_t R, int64_t A, int64_t E,
                  int32_t* offsets, int32_t* order, int32_t* inverse, void* stream);

/* y[p][n] = bf16( sum_k x[row(p)][k] * W_e[n][k] ) for every sorted row p, e the expert with
 * offsets[e] <= p < offsets[e + 1] and row(p) = src_row[p] / row_div (p itself when src_row is
 * null): every expert's int4 linear (tao_int4wo_linear_bf16's weight format per expert: packed
 * [E][N][K/8], scales_and_zeros [E][N][K/g][2]) over its own rows in one launch, the token gather
 * x[indices] folded into the x load. x bf16 [x_rows][K], y bf16 [R][N]; the sum in fp32 in a fixed
 * order. With packed_b / scales_and_zeros_b (a second stack of the same shape: gate and up in one
 * launch) y[p][n] = bf16( bf16(silu(bf16 a)) * bf16 b ), a and b the two stacks' sums: the roundings
 * of F.silu(F.linear(x, w1)) * F.linear(x, w3) on bf16 tensors. K % 32 == 0, K % group_size == 0,
 * N * K / 2 a multiple of 16 and below 4 GiB; x, packed 16-B aligned. Rows per tile: csrc/moe_host.h
 * (tao_moe_row_tile, tao_tune_moe). Replaces the per-expert x[indices], F.linear x 3, silu and mul
 * of ConditionalFeedForwardAOQuantizable's many-token branch. */
int tao_int4wo_grouped_linear_bf16(const uint16_t* x, int64_t x_rows, const int32_t* src_row,
                                   int64_t row_div, const uint32_t* packed,
                                   const uint16_t* scales_and_zeros, const uint32_t* packed_b,
                                   const uint16_t* scales_and_zeros_b, const int32_t* offsets,
                                   int64_t R, int64_t E, uint16_t* y, int64_t N, int64_t K,
                                   int64_t group_size, void* stream);

/* out[t] = the expert-weighted sum of token t's A rows of y2 bf16 [R][D], taken in ascending
 * sorted position p = inverse[t * A + a]: acc = +0, then acc = bf16(acc + bf16(y2[p] * w[t * A + a])),
 * the reference's mul and scatter_add as the CPU executes them, for any A. expert_weights bf16 [R]
 * (token order), out bf16 [T][D]. D % 8 == 0, T <= 65535; y2 and out 16-B aligned. Replaces the
 * weight gather, mul, zeros_like and scatter_add of quantizable_moe_modules.py:173-190. */
int tao_moe_combine_bf16(const uint16_t* y2, const uint16_t* expert_weights,
                         const int32_t* inverse, uint16_t* out, int64_t T, int64_t A, int64_t D,
                         void* stream);

/* ---- int8 KV cache (AffineQuantizedKVCache, torchao/_models/llama/model.py:198-240) -----------
 * k_cache / v_cache [B][Hkv][T][128] int8 codes, k_scale / v_scale [B][Hkv][T] bf16, one scale per
 * row: symmetric, [-127, 127], eps 1e-5, the arithmetic of _quantize_activation_per_token_absmax in
 * bf16 (quantization/utils.py:152-182): s = max(bf16(amax / 127), bf16(1e-5)),
 * q = clamp(rint(bf16(x * bf16(1 / s))), -127, 127). */

/* tao_rope_kv_bf16 (torchao_mi355x_llama.h) with the cache write quantized: qkv
 * [B*S][(H + 2 Hkv) * 128] bf16 -> q_out [B][H][S][128] rotated; the rotated k and the raw v rows
 * of the S tokens exact in k_cur / v_cur [B][Hkv][S][128] bf16, and their codes and scales written
 * to the caches at pos[s] (a position outside [0, T) writes no cache row and sets
 * tao_decode_status bit 1). head_dim == 128. Replaces apply_rotary_emb and the quantize-and-store
 * half of AffineQuantizedKVCache.update (model.py:219-233). */
int tao_rope_kv_q8_bf16(const uint16_t* qkv, const float* freqs, const int64_t* pos,
                        uint16_t* q_out, int8_t* k_cache, int8_t* v_cache, uint16_t* k_scale,
                        uint16_t* v_scale, uint16_t* k_cur, uint16_t* v_cur, int64_t B, int64_t S,
                        int64_t H, int64_t Hkv, int64_t D, int64_t T, void* stream);

/* One-query attention of a decode step over the int8 caches: q [B][H][1][128] bf16 against keys
 * 0..pos[0] (pos read on the device), keys 0..pos[0]-1 from the codes and scales, the key at pos[0]
 * exact from k_cur / v_cur [B][Hkv][1][128] (the rows tao_rope_kv_q8_bf16 left there). In fp32:
 * score_t = k_scale[t] * (q . k8[t]) * scale, o = sum_t p_t * v_scale[t] * v8[t], online softmax.
 * Any T. splits 1: out [B][1][H*128] bf16. splits 2 or 4: the cached keys split into that many
 * ranges per head, the unnormalised partials written to partial [B * H][splits][132] fp32 in the
 * record of tao_attn_decode_split_bf16 (the current key in split 0) for tao_attn_merge_bf16.
 * H / Hkv in {1, 2, 4, 8}; caches, q, k_cur, v_cur and partial 16-B aligned. Replaces the
 * dequantize-everything half of AffineQuantizedKVCache.update and the F.scaled_dot_product_attention
 * after it (model.py:219-233, 441-476) without forming the bf16 cache. */
int tao_attn_decode_q8_bf16(const uint16_t* q, const int8_t* k_cache, const int8_t* v_cache,
                            const uint16_t* k_scale, const uint16_t* v_scale,
                            const uint16_t* k_cur, const uint16_t* v_cur, const int64_t* pos,
                            float* partial, uint16_t* out, int64_t B, int64_t H, int64_t Hkv,
                            int64_t D, int64_t T, float scale, int64_t splits, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TORCHAO_MI355X_H_ */
