"""``torch.ops.torchao`` operators of the MI355X weight-only quantized linear path.

Follows the reference's registration pattern (torchao/ops.py:12-21 ``Library("torchao",
"FRAGMENT")`` + ``lib.define`` schemas, :73-77 ``register_fake`` meta impls using
``torch._check``). The device impls are registered for the ``CUDA`` dispatch key (which is HIP
on ROCm, as in tensor_core_tiled_layout.cu:370-374) and call the gfx950 C-ABI library
(``include/torchao_mi355x.h``) on the current stream: no allocation besides the output (caching
allocator), no host synchronisation, so every op is hipGraph-capturable.

Operators:
  * ``unpack_tensor_core_tiled_layout`` / ``dequantize_tensor_core_tiled_layout`` — the
    reference schemas (ops.py:16-21) on the reference tile format, with an optional
    ``tile_format``: the CUDA nibble map of the reference's .cu kernels, or the one PyTorch-ROCm's
    ``aten._convert_weight_to_int4pack`` writes (the default on ROCm builds).
  * ``pack_tensor_core_tiled_layout`` — inverse of the unpack (bit-identical to
    ``aten._convert_weight_to_int4pack`` in the ROCm map), for checkpoint interchange.
  * ``int4_pack`` / ``int4_unpack`` / ``int4_dequantize`` / ``int4_weight_only_linear`` — the
    gfx950 row-stream int4 layout; ``int4_weight_only_linear`` replaces
    ``aten._weight_int4pack_mm`` (tensor_core_tiled_layout.py:104).
  * ``int8_weight_only_linear`` — replaces mm + scale (plain_layout.py:256-266).
  * ``int8_quantize_per_token`` / ``int8_scaled_mm`` — replace the activation quant
    (quant_api.py:1258-1273) and ``int_scaled_matmul`` + weight scale (plain_layout.py:294-315).
  * ``int8_dyn_linear`` — one token through both in one launch (decode), bit-identical.
  * ``int4_quantize_pack`` / ``int8_quantize_rows`` — the weight quantizers of
    ``from_hp_to_intx`` in one pass each (tinygemm qparams + quantize + row-stream pack;
    symmetric per-row int8), bit-exact to the bf16 torch-op formulation.
  * ``int4_hqq_quantize_pack`` — ``from_hp_to_intx(use_hqq=True)`` on a bf16 GPU weight: the HQQ
    iteration (quant_primitives.py:1901-2111) in registers, its global stop on the device.
  * ``fp8_weight_only_linear`` — e4m3fn per-row-scaled weight-only linear; replaces
    ``F.linear(x, weight.dequantize(), bias)`` (floatx/float8_layout.py:391-396).
  * ``fp8_quantize_rows`` / ``fp8_dequantize`` — the per-row e4m3fn quantizer of
    ``from_hp_to_floatx`` and its dequant (quant_primitives.py:2175-2312), byte for byte.
  * ``fp8_scaled_mm`` — e4m3fn x e4m3fn product with per-row scales on both operands; replaces
    the ``torch._scaled_mm`` call of ``_linear_fp8_act_fp8_weight_impl``
    (floatx/float8_layout.py:329-367).
  * ``fp8_dyn_linear`` — the activation quantisation and that product from a bf16 input (one
    token: one launch), bit-identical to ``fp8_quantize_rows`` -> ``fp8_scaled_mm``.
  * ``mx_quantize_rows`` — the MXFP8 block quantizer (e4m3fn codes, one E8M0 byte per 32
    elements); replaces ``to_mx`` (prototype/mx_formats/mx_tensor.py:133-326), byte for byte.
  * ``mx_scaled_mm`` — the block-scaled e4m3fn x e4m3fn product; replaces the ``torch._scaled_mm``
    call of ``_addmm_mx_dispatch`` (prototype/mx_formats/mx_ops.py).
  * ``mx_dyn_linear`` — both from a bf16 input (one token: one launch), bit-identical to
    ``mx_quantize_rows`` -> ``mx_scaled_mm``.
  * ``mxfp4_quantize_rows`` / ``mxfp4w_scaled_mm`` / ``mxfp4w_dyn_linear`` — the same three for
    e2m1 weights (two codes per byte) under e4m3fn activations (csrc/mx_fp4.hip).
  * ``blockfp8_quantize_act`` / ``blockfp8_quantize_weight`` / ``blockfp8_dequantize_weight`` /
    ``blockfp8_scaled_mm`` / ``blockfp8_dyn_linear`` — the blockwise float8 recipe (e4m3fn codes,
    fp32 scales per 1 x 128 activation block and 128 x 128 weight block, csrc/block_fp8.hip);
    replace the Triton kernels of prototype/blockwise_fp8_inference/blockwise_quantization.py.
  * ``act_prescale`` — ``bf16(x / scale)`` over the input channels (IEEE fp32 division, one
    rounding); replaces the division of ``WeightTensorWithLinearActivationScaleMetadata``
    (quantization/linear_activation_scale.py:61-70), the AWQ / SmoothQuant equalization scale.
  * ``int4_prescaled_linear`` — that division and ``int4_weight_only_linear`` from a bf16 input
    (one token without a bias at K <= 4096 and N * K <= 2^24: one launch, the quotient formed
    while the GEMV stages x in LDS), bit-identical to ``act_prescale`` ->
    ``int4_weight_only_linear``.
  * ``int8_smooth_quantize_per_token`` / ``int8_smooth_quantize_static`` — SmoothQuant's
    activation side in one launch: ``bf16(x / smooth)``, then the per-token int8 codes of
    ``to_affine_quantized_intx`` with its default eps (2^-7 for bf16) or the static codes of
    ``to_affine_quantized_intx_static`` with one calibrated scale; replace the division above and
    ``_ActQuantizer`` (prototype/smoothquant/api.py:133-155). The scale comes back as ``[M]``.
  * ``int8_smooth_dyn_linear`` / ``int8_smooth_static_linear`` — those and ``int8_scaled_mm``
    from a bf16 input at any M (one token up to K = 16384, static 8192: one launch, the division
    and the quantisation in the GEMV's prologue), bit-identical to the two ops.
  * ``rowwise_scaled_linear_cutlass_s8s4`` — the reference's op name and schema (ops.py:28-30) for
    int8 activations x packed int4 weights with fp32 row scales, on the int8 matrix cores
    (csrc/w4a8.hip); the reference builds it for sm80 only.
  * ``int8_quantize_per_token_f32`` / ``int4_quantize_rows_packed`` — its two quantizers,
    ``_int8_symm_cutlass_quant`` and ``_int4_symm_cutlass_quant`` (quant_api.py:1299-1323), one
    launch each, byte for byte.
  * ``w4a8_dyn_linear`` — the activation quantisation and the product from a bf16 input (one
    token: one launch), bit-identical to the two ops.
"""

import ctypes
import os
from typing import Optional, Tuple

import torch
from torch import Tensor

from torchao import _lib

lib = torch.library.Library("torchao", "FRAGMENT")
# The reference schemas (ops.py:16-21) plus an optional trailing tile_format (-1 = this
# platform's aten format, see default_tile_format), so the reference's positional calls bind.
lib.define(
    "unpack_tensor_core_tiled_layout(Tensor packed_w, int inner_k_tiles, int tile_format=-1) "
    "-> Tensor"
)
lib.define(
    "dequantize_tensor_core_tiled_layout(Tensor packed_w, Tensor scales_and_zeros, "
    "int group_size, int inner_k_tiles, int tile_format=-1) -> Tensor"
)
lib.define(
    "pack_tensor_core_tiled_layout(Tensor int_data, int inner_k_tiles, int tile_format=-1) "
    "-> Tensor"
)
lib.define("int4_pack(Tensor int_data) -> Tensor")
lib.define("int4_pack_u8(Tensor int_data_u8) -> Tensor")
lib.define("int4_unpack(Tensor packed_w) -> Tensor")
lib.define(
    "int4_dequantize(Tensor packed_w, Tensor scales_and_zeros, int group_size, int mode=0) "
    "-> Tensor"
)
lib.define(
    "int4_weight_only_linear(Tensor x, Tensor packed_w, Tensor scales_and_zeros, "
    "int group_size, Tensor? bias=None) -> Tensor"
)
lib.define(
    "int8_weight_only_linear(Tensor x, Tensor w_int8, Tensor scale, Tensor? bias=None) -> Tensor"
)
lib.define("int8_quantize_per_token(Tensor x) -> (Tensor, Tensor)")
lib.define("int4_quantize_pack(Tensor w, int group_size, float eps) -> (Tensor, Tensor)")
lib.define("int8_quantize_rows(Tensor w, float eps) -> (Tensor, Tensor)")
lib.define(
    "int8_scaled_mm(Tensor x_int8, Tensor x_scale, Tensor w_int8, Tensor w_scale, "
    "Tensor? bias=None) -> Tensor"
)
lib.define(
    "int8_dyn_linear(Tensor x, Tensor w_int8, Tensor w_scale, Tensor? bias=None) -> Tensor"
)
# The float8 weight-only ops live in a fragment of their own: ``lib`` keeps exactly the integer
# op set that tests/test_gpu_opcheck.py enumerates from it; these three are opchecked in
# tests/test_gpu_float8.py.
lib_float8 = torch.library.Library("torchao", "FRAGMENT")
lib_float8.define(
    "fp8_weight_only_linear(Tensor x, Tensor w_fp8, Tensor scale, Tensor? bias=None) -> Tensor"
)
lib_float8.define("fp8_quantize_rows(Tensor w) -> (Tensor, Tensor)")
lib_float8.define("fp8_dequantize(Tensor q, Tensor scale) -> Tensor")

# The float8 dynamic-activation ops, again on a fragment of their own (the two sets above are
# enumerated by existing tests); opchecked in tests/test_gpu_float8_dyn.py.
lib_float8_dyn = torch.library.Library("torchao", "FRAGMENT")
lib_float8_dyn.define(
    "fp8_scaled_mm(Tensor xq, Tensor x_scale, Tensor w_fp8, Tensor w_scale, "
    "Tensor? bias=None) -> Tensor"
)
lib_float8_dyn.define(
    "fp8_dyn_linear(Tensor x, Tensor w_fp8, Tensor w_scale, Tensor? bias=None) -> Tensor"
)

# The MXFP8 ops (torchao.prototype.mx_formats), on a fragment of their own for the same reason;
# opchecked in tests/test_gpu_mx.py. Codes cross as float8_e4m3fn, scale bytes as uint8.
lib_mx = torch.library.Library("torchao", "FRAGMENT")
lib_mx.define("mx_quantize_rows(Tensor x) -> (Tensor, Tensor)")
lib_mx.define(
    "mx_scaled_mm(Tensor xq, Tensor x_scale, Tensor wq, Tensor w_scale, Tensor? bias=None) "
    "-> Tensor"
)
lib_mx.define("mx_dyn_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias=None) -> Tensor")
# The MXFP4-weight ops (e4m3fn activation x e2m1 weight), again on a fragment of their own; opchecked
# in tests/test_gpu_mxfp4.py. Weight codes cross as uint8 [N, K/2], two per byte.
lib_mxfp4 = torch.library.Library("torchao", "FRAGMENT")
lib_mxfp4.define("mxfp4_quantize_rows(Tensor x) -> (Tensor, Tensor)")
lib_mxfp4.define(
    "mxfp4w_scaled_mm(Tensor xq, Tensor x_scale, Tensor wq, Tensor w_scale, Tensor? bias=None) "
    "-> Tensor")
lib_mxfp4.define(
    "mxfp4w_dyn_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias=None) -> Tensor")
# The blockwise float8 ops (torchao.prototype.blockwise_fp8_inference), on a fragment of their own;
# opchecked in tests/test_gpu_blockfp8.py. Codes cross as float8_e4m3fn, scales as float32:
# [..., K/128] for the activation, [ceil(N/128), K/128] for the weight.
lib_blockfp8 = torch.library.Library("torchao", "FRAGMENT")
lib_blockfp8.define("blockfp8_quantize_act(Tensor x) -> (Tensor, Tensor)")
lib_blockfp8.define("blockfp8_quantize_weight(Tensor w) -> (Tensor, Tensor)")
lib_blockfp8.define(
    "blockfp8_dequantize_weight(Tensor wq, Tensor w_scale, bool out_bf16=False) -> Tensor")
lib_blockfp8.define(
    "blockfp8_scaled_mm(Tensor xq, Tensor x_scale, Tensor wq, Tensor w_scale, Tensor? bias=None) "
    "-> Tensor")
lib_blockfp8.define(
    "blockfp8_dyn_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias=None) -> Tensor")
# The activation pre-scale ops (AWQ: torchao.prototype.awq, quantization/linear_activation_scale.py),
# on a fragment of their own; opchecked in tests/test_gpu_awq.py. bf16 only.
lib_awq = torch.library.Library("torchao", "FRAGMENT")
lib_awq.define("act_prescale(Tensor x, Tensor scale) -> Tensor")
lib_awq.define(
    "int4_prescaled_linear(Tensor x, Tensor act_scale, Tensor packed_w, Tensor scales_and_zeros, "
    "int group_size, Tensor? bias=None) -> Tensor")
# The SmoothQuant ops (torchao.prototype.smoothquant over the int8 dynamic / static linear), on a
# fragment of their own; opchecked in tests/test_gpu_smoothquant.py. bf16 only; ``smooth`` is the
# per-input-channel factor [K], ``act_scale`` the per-tensor scale of the static recipe (one bf16).
lib_smoothquant = torch.library.Library("torchao", "FRAGMENT")
lib_smoothquant.define(
    "int8_smooth_quantize_per_token(Tensor x, Tensor smooth) -> (Tensor, Tensor)")
lib_smoothquant.define(
    "int8_smooth_quantize_static(Tensor x, Tensor smooth, Tensor act_scale) -> (Tensor, Tensor)")
lib_smoothquant.define(
    "int8_smooth_dyn_linear(Tensor x, Tensor smooth, Tensor w_int8, Tensor w_scale, "
    "Tensor? bias=None) -> Tensor")
lib_smoothquant.define(
    "int8_smooth_static_linear(Tensor x, Tensor smooth, Tensor act_scale, Tensor w_int8, "
    "Tensor w_scale, Tensor? bias=None) -> Tensor")
# The W4A8 ops (Int8DynamicActivationInt4WeightConfig with CutlassInt4PackedLayout; csrc/w4a8.hip),
# on a fragment of their own; opchecked in tests/test_gpu_w4a8.py. The first is the reference's
# schema and name (torchao/ops.py:28-30, 666-695), served here on gfx950. Weight codes cross as int8
# [N, K/2], two int4 per byte; all scales are float32.
lib_w4a8 = torch.library.Library("torchao", "FRAGMENT")
lib_w4a8.define(
    "rowwise_scaled_linear_cutlass_s8s4(Tensor input, Tensor input_scale, Tensor weight, "
    "Tensor weight_scale, Tensor? bias=None, ScalarType? out_dtype=None) -> Tensor")
lib_w4a8.define("int8_quantize_per_token_f32(Tensor x) -> (Tensor, Tensor)")
lib_w4a8.define("int4_quantize_rows_packed(Tensor w) -> (Tensor, Tensor)")
lib_w4a8.define(
    "w4a8_dyn_linear(Tensor x, Tensor weight, Tensor weight_scale, Tensor? bias=None) -> Tensor")
# The NF4 ops (NF4Tensor / NF4WeightOnlyConfig, torchao/dtypes/nf4tensor.py; csrc/nf4.hip), on a
# fragment of their own; opchecked in tests/test_gpu_nf4.py. bf16 HIP tensors only: everything else
# runs the plain-torch formulation in nf4tensor.py. Their CUDA kernels exist in C++ only
# (csrc/torch_ops.cpp), so without libtorchao_ops.so a call raises instead of falling back.
lib_nf4 = torch.library.Library("torchao", "FRAGMENT")
lib_nf4.define("nf4_quantize_blocks(Tensor w, Tensor levels) -> (Tensor, Tensor)")
lib_nf4.define(
    "nf4_dequantize(Tensor codes, Tensor qscalers, Tensor qfactor, Tensor mean, Tensor levels, "
    "int[] shape) -> Tensor")
lib_nf4.define(
    "nf4_linear(Tensor x, Tensor codes, Tensor qscalers, Tensor qfactor, Tensor mean, "
    "Tensor levels, int N, Tensor? bias=None) -> Tensor")
# The FP6 ops (FPXWeightOnlyConfig, torchao/dtypes/floatx/floatx_tensor_core_layout.py;
# csrc/fp6.hip), on a fragment of their own; opchecked in tests/test_gpu_fp6.py. (ebits, mbits) is
# (3, 2) or (2, 3); codes are the native storage, int32 [N, K * 6 / 32]; scale is bf16 [N]. bf16
# HIP tensors only. Their CUDA kernels exist in C++ only (csrc/torch_ops.cpp), so without
# libtorchao_ops.so a call raises instead of falling back.
lib_fp6 = torch.library.Library("torchao", "FRAGMENT")
lib_fp6.define("fp6_quantize_rows(Tensor w, int ebits, int mbits) -> (Tensor, Tensor)")
lib_fp6.define("fp6_dequantize(Tensor codes, Tensor scale, int ebits, int mbits) -> Tensor")
lib_fp6.define(
    "fp6_weight_only_linear(Tensor x, Tensor codes, Tensor scale, int ebits, int mbits, "
    "Tensor? bias=None) -> Tensor")
# The MoE ops (MoEQuantConfig, torchao/prototype/moe_quant; csrc/moe_gemm.hip), on a fragment of
# their own; opchecked in tests/test_gpu_moe.py: the stable sort of the token activations by expert,
# every expert's int4 linear over its own sorted rows in one launch (a second stack: gate and up
# with SwiGLU in the epilogue), and the expert-weighted sum back to token order. bf16 HIP tensors
# only. Their CUDA kernels exist in C++ only (csrc/torch_ops.cpp), so without libtorchao_ops.so a
# call raises instead of falling back.
lib_moe = torch.library.Library("torchao", "FRAGMENT")
lib_moe.define("moe_route(Tensor expert_indices, int num_experts, int top_k) -> "
               "(Tensor, Tensor, Tensor)")
lib_moe.define(
    "int4_grouped_linear(Tensor x, Tensor? src_row, int row_div, Tensor packed, "
    "Tensor scales_and_zeros, Tensor? packed_b, Tensor? scales_and_zeros_b, Tensor offsets, "
    "int group_size) -> Tensor")
lib_moe.define(
    "moe_combine(Tensor y2, Tensor expert_weights, Tensor inverse, int top_k) -> Tensor")
# The HQQ int4 quantizer (Int4WeightOnlyConfig(use_hqq=True); csrc/hqq.hip), on a fragment of its
# own; opchecked in tests/test_gpu_hqq.py. bf16 HIP weight [N, K] or [E, N, K] (one stop decision
# for the whole tensor) -> the operands of int4_weight_only_linear and the iterations run (int32
# [1], on the device: the op never synchronises).
lib_hqq = torch.library.Library("torchao", "FRAGMENT")
lib_hqq.define("int4_hqq_quantize_pack(Tensor w, int group_size) -> (Tensor, Tensor, Tensor)")

_GROUP_SIZES = (32, 64, 128, 256)


def _ptr(t: Optional[Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(t: Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _require_contig(t: Tensor, name: str):
    torch._check(t.is_contiguous(), lambda: f"{name} must be contiguous")


def _same_device(x: Tensor, **operands):
    """Every operand on x's device (the kernels take raw device pointers; a tensor on another
    GPU or the host would reach the launch as a foreign pointer). RuntimeError otherwise, like
    the C++ op kernels (csrc/torch_ops.cpp check_device)."""
    for name, t in operands.items():
        if t is not None and t.device != x.device:
            raise RuntimeError(f"{name} is on {t.device} but x is on {x.device}: all operands "
                               "must be on the same device")


# ---------------------------------------------------------------------------------------------
# reference tile format (torchao/ops.py:255-377)
# ---------------------------------------------------------------------------------------------
TILE_FORMAT_CUDA = 0  # tensor_core_tiled_layout.cu:131-215 (aten on CUDA builds)
TILE_FORMAT_ROCM = 1  # aten._convert_weight_to_int4pack on PyTorch-ROCm (wave64 lanes)
_default_tile_format = TILE_FORMAT_ROCM if torch.version.hip else TILE_FORMAT_CUDA


def default_tile_format() -> int:
    """The nibble map ``aten._convert_weight_to_int4pack`` writes on this PyTorch build (both
    share the tile tensor's shape; include/torchao_mi355x.h documents the two maps)."""
    return _default_tile_format


def set_default_tile_format(fmt) -> None:
    """Select the map that tile_format=-1 means: "cuda" / 0 to read a TensorCoreTiledLayout
    checkpoint written by a CUDA build of torchao, "rocm" / 1 for one written on ROCm. This is
    also the explicit choice that lets reference checkpoints load (``checkpoint_tile_format``)."""
    global _default_tile_format, _chosen_tile_format
    _default_tile_format = _tile_format(fmt)
    _chosen_tile_format = _default_tile_format


# The map a reference checkpoint's tile storage is read with. The two maps share the tile
# tensor's shape and cannot be told apart from the bytes, and CUDA builds write most
# checkpoints, so loading never guesses: None until set_default_tile_format() or the
# checkpoint_tile_format() context chooses one.
_chosen_tile_format = None


class checkpoint_tile_format:
    """``with torchao.ops.checkpoint_tile_format("cuda"): torch.load(...)`` — the nibble map of
    the reference TensorCoreTiledLayout storage being loaded, for the duration of the block."""

    def __init__(self, fmt):
        self.fmt = _tile_format(fmt) if fmt != -1 else -1
        torch._check(self.fmt != -1, lambda: "checkpoint_tile_format needs 'cuda' or 'rocm'")

    def __enter__(self):
        global _chosen_tile_format
        self._prev = _chosen_tile_format
        _chosen_tile_format = self.fmt
        return self

    def __exit__(self, *exc):
        global _chosen_tile_format
        _chosen_tile_format = self._prev
        return False


def chosen_checkpoint_tile_format() -> int:
    """The explicitly chosen map for reference tile storage; raises if none was chosen."""
    if _chosen_tile_format is None:
        raise RuntimeError(
            "this checkpoint holds int4 weights in the reference's TensorCoreTiledLayout tile "
            "format, whose nibble map depends on the PyTorch build that wrote it (CUDA or ROCm) "
            "and cannot be detected from the bytes. Choose it before loading: "
            "torchao.ops.set_default_tile_format('cuda' | 'rocm'), or "
            "`with torchao.ops.checkpoint_tile_format('cuda' | 'rocm'): torch.load(...)`")
    return _chosen_tile_format


def _tile_format(fmt) -> int:
    if isinstance(fmt, str):
        fmt = {"cuda": TILE_FORMAT_CUDA, "rocm": TILE_FORMAT_ROCM}.get(fmt.lower(), -2)
    if fmt == -1:
        return _default_tile_format
    torch._check(fmt in (TILE_FORMAT_CUDA, TILE_FORMAT_ROCM),
                 lambda: f"tile_format must be 'cuda' (0), 'rocm' (1) or -1, got {fmt}")
    return int(fmt)


def _check_tile_n(N: int, fmt: int):
    if fmt == TILE_FORMAT_ROCM:
        torch._check(N % 16 == 0, lambda: f"ROCm tile format needs N % 16 == 0, got N={N}")


def _check_tile(packed_w: Tensor, inner_k_tiles: int):
    torch._check(
        packed_w.dim() == 4, lambda: f"packed weight should be a 4d tensor, got {packed_w.dim()}D"
    )
    torch._check(
        packed_w.dtype is torch.int32, lambda: f"weight must be INT32, got {packed_w.dtype}"
    )
    torch._check(inner_k_tiles in (2, 4, 8), lambda: "inner_k_tiles must be 2, 4, or 8")
    torch._check(packed_w.size(2) == 32, lambda: "packed weight must have 32 at dim 2")
    torch._check(
        packed_w.size(3) == inner_k_tiles // 2,
        lambda: "packed weight must have inner_k_tiles/2 at dim 3",
    )
    return packed_w.size(0) * 8, packed_w.size(1) * inner_k_tiles * 16


def _check_tile_sz(sz: Tensor, group_size: int, N: int, K: int):
    torch._check(sz.dtype is torch.bfloat16, lambda: "scales_and_zeros must be bfloat16")
    torch._check(sz.dim() == 3, lambda: f"scales_and_zeros must be 3D, got {sz.dim()}")
    torch._check(group_size in _GROUP_SIZES, lambda: "qGroupSize must be 32, 64, 128, or 256")
    torch._check(
        sz.size(0) == K // group_size, lambda: "scales_and_zeros must have K // qGroupSize at dim 0"
    )
    torch._check(sz.size(1) == N, lambda: "scales_and_zeros must have N at dim 1")
    torch._check(sz.size(2) == 2, lambda: "scales_and_zeros must have 2 at dim 2")


@torch.library.register_fake("torchao::unpack_tensor_core_tiled_layout")
def _(packed_w: Tensor, inner_k_tiles: int, tile_format: int = -1) -> Tensor:
    N, K = _check_tile(packed_w, inner_k_tiles)
    _check_tile_n(N, _tile_format(tile_format))
    return packed_w.new_empty((N, K), dtype=torch.int32)


def _unpack_tile_cuda(packed_w: Tensor, inner_k_tiles: int, tile_format: int = -1) -> Tensor:
    N, K = _check_tile(packed_w, inner_k_tiles)
    fmt = _tile_format(tile_format)
    _check_tile_n(N, fmt)
    _require_contig(packed_w, "packed_w")
    out = torch.empty((N, K), dtype=torch.int32, device=packed_w.device)
    with torch.cuda.device(packed_w.device):
        _lib.call("tao_unpack_tensor_core_tiled_layout", _ptr(packed_w), _ptr(out), N, K,
                  inner_k_tiles, fmt, _stream(packed_w))
    return out


def _unpack_tile_cpu(packed_w: Tensor, inner_k_tiles: int, tile_format: int = -1) -> Tensor:
    """Host C++ unpack (tao_unpack_tensor_core_tiled_layout_host) for CPU-resident checkpoints."""
    N, K = _check_tile(packed_w, inner_k_tiles)
    fmt = _tile_format(tile_format)
    _check_tile_n(N, fmt)
    packed_w = packed_w.contiguous()
    out = torch.empty((N, K), dtype=torch.int32)
    _lib.call("tao_unpack_tensor_core_tiled_layout_host", _ptr(packed_w), _ptr(out), N, K,
              inner_k_tiles, fmt)
    return out


@torch.library.register_fake("torchao::dequantize_tensor_core_tiled_layout")
def _(packed_w: Tensor, scales_and_zeros: Tensor, group_size: int, inner_k_tiles: int,
      tile_format: int = -1) -> Tensor:
    N, K = _check_tile(packed_w, inner_k_tiles)
    _check_tile_n(N, _tile_format(tile_format))
    _check_tile_sz(scales_and_zeros, group_size, N, K)
    return packed_w.new_empty((N, K), dtype=torch.bfloat16)


def _dequant_tile_cuda(packed_w, scales_and_zeros, group_size, inner_k_tiles, tile_format=-1):
    N, K = _check_tile(packed_w, inner_k_tiles)
    fmt = _tile_format(tile_format)
    _check_tile_n(N, fmt)
    _check_tile_sz(scales_and_zeros, group_size, N, K)
    _same_device(packed_w, scales_and_zeros=scales_and_zeros)
    _require_contig(packed_w, "packed_w")
    _require_contig(scales_and_zeros, "scales_and_zeros")
    out = torch.empty((N, K), dtype=torch.bfloat16, device=packed_w.device)
    with torch.cuda.device(packed_w.device):
        _lib.call("tao_dequantize_tensor_core_tiled_layout", _ptr(packed_w),
                  _ptr(scales_and_zeros), _ptr(out), N, K, group_size, inner_k_tiles, fmt,
                  _stream(packed_w))
    return out


def _check_pack_tile(int_data: Tensor, inner_k_tiles: int):
    torch._check(int_data.dim() == 2 and int_data.dtype is torch.int32,
                 lambda: "int_data must be a 2D int32 tensor")
    torch._check(inner_k_tiles in (2, 4, 8), lambda: "inner_k_tiles must be 2, 4, or 8")
    N, K = int_data.shape
    torch._check(N % 8 == 0, lambda: f"N ({N}) must be a multiple of 8")
    torch._check(K % (inner_k_tiles * 16) == 0,
                 lambda: f"K ({K}) must be a multiple of {inner_k_tiles * 16}")
    return N, K


@torch.library.register_fake("torchao::pack_tensor_core_tiled_layout")
def _(int_data: Tensor, inner_k_tiles: int, tile_format: int = -1) -> Tensor:
    N, K = _check_pack_tile(int_data, inner_k_tiles)
    _check_tile_n(N, _tile_format(tile_format))
    return int_data.new_empty(
        (N // 8, K // (inner_k_tiles * 16), 32, inner_k_tiles // 2), dtype=torch.int32
    )


def _pack_tile_cuda(int_data: Tensor, inner_k_tiles: int, tile_format: int = -1) -> Tensor:
    N, K = _check_pack_tile(int_data, inner_k_tiles)
    fmt = _tile_format(tile_format)
    _check_tile_n(N, fmt)
    _require_contig(int_data, "int_data")
    out = torch.empty((N // 8, K // (inner_k_tiles * 16), 32, inner_k_tiles // 2),
                      dtype=torch.int32, device=int_data.device)
    with torch.cuda.device(int_data.device):
        _lib.call("tao_pack_tensor_core_tiled_layout", _ptr(int_data), _ptr(out), N, K,
                  inner_k_tiles, fmt, _stream(int_data))
    return out


# ---------------------------------------------------------------------------------------------
# gfx950 row-stream int4 layout
# ---------------------------------------------------------------------------------------------
def _check_int4_plain(int_data: Tensor):
    torch._check(int_data.dim() == 2, lambda: "int4_pack expects a 2D [N, K] tensor")
    torch._check(int_data.dtype is torch.int32, lambda: "int4_pack expects int32 values 0..15")
    torch._check(int_data.size(1) % 8 == 0, lambda: "int4_pack: K must be a multiple of 8")


@torch.library.register_fake("torchao::int4_pack")
def _(int_data: Tensor) -> Tensor:
    _check_int4_plain(int_data)
    return int_data.new_empty((int_data.size(0), int_data.size(1) // 8), dtype=torch.int32)


def _int4_pack_cuda(int_data: Tensor) -> Tensor:
    _check_int4_plain(int_data)
    int_data = int_data.contiguous()
    N, K = int_data.shape
    out = torch.empty((N, K // 8), dtype=torch.int32, device=int_data.device)
    with torch.cuda.device(int_data.device):
        _lib.call("tao_int4_pack", _ptr(int_data), _ptr(out), N, K, _stream(int_data))
    return out


def _int4_pack_cpu(int_data: Tensor) -> Tensor:
    _check_int4_plain(int_data)
    int_data = int_data.contiguous()
    N, K = int_data.shape
    out = torch.empty((N, K // 8), dtype=torch.int32)
    _lib.call("tao_int4_pack_host", _ptr(int_data), _ptr(out), N, K)
    return out


@torch.library.register_fake("torchao::int4_pack_u8")
def _(int_data_u8: Tensor) -> Tensor:
    torch._check(int_data_u8.dim() == 2 and int_data_u8.dtype is torch.uint8,
                 lambda: "int4_pack_u8 expects a 2D uint8 [N, K/2] tensor")
    return int_data_u8.new_empty((int_data_u8.size(0), int_data_u8.size(1) // 4), dtype=torch.int32)


def _int4_pack_u8_cuda(int_data_u8: Tensor) -> Tensor:
    torch._check(int_data_u8.dim() == 2 and int_data_u8.dtype is torch.uint8,
                 lambda: "int4_pack_u8 expects a 2D uint8 [N, K/2] tensor")
    int_data_u8 = int_data_u8.contiguous()
    N, K = int_data_u8.size(0), int_data_u8.size(1) * 2
    out = torch.empty((N, K // 8), dtype=torch.int32, device=int_data_u8.device)
    with torch.cuda.device(int_data_u8.device):
        _lib.call("tao_int4_pack_u8", _ptr(int_data_u8), _ptr(out), N, K, _stream(int_data_u8))
    return out


@torch.library.register_fake("torchao::int4_unpack")
def _(packed_w: Tensor) -> Tensor:
    torch._check(packed_w.dim() == 2 and packed_w.dtype is torch.int32,
                 lambda: "int4_unpack expects a 2D int32 [N, K/8] tensor")
    return packed_w.new_empty((packed_w.size(0), packed_w.size(1) * 8), dtype=torch.int32)


def _int4_unpack_cuda(packed_w: Tensor) -> Tensor:
    _require_contig(packed_w, "packed_w")
    N, K = packed_w.size(0), packed_w.size(1) * 8
    out = torch.empty((N, K), dtype=torch.int32, device=packed_w.device)
    with torch.cuda.device(packed_w.device):
        _lib.call("tao_int4_unpack", _ptr(packed_w), _ptr(out), N, K, _stream(packed_w))
    return out


def _int4_unpack_cpu(packed_w: Tensor) -> Tensor:
    packed_w = packed_w.contiguous()
    N, K = packed_w.size(0), packed_w.size(1) * 8
    out = torch.empty((N, K), dtype=torch.int32)
    _lib.call("tao_int4_unpack_host", _ptr(packed_w), _ptr(out), N, K)
    return out


def _check_int4_weight(packed_w: Tensor, sz: Tensor, group_size: int):
    torch._check(packed_w.dim() == 2 and packed_w.dtype is torch.int32,
                 lambda: "packed weight must be a 2D int32 [N, K/8] tensor")
    N, K = packed_w.size(0), packed_w.size(1) * 8
    torch._check(group_size in _GROUP_SIZES, lambda: "qGroupSize must be 32, 64, 128, or 256")
    torch._check(K % group_size == 0, lambda: f"K ({K}) must be divisible by qGroupSize")
    torch._check(sz.dtype is torch.bfloat16, lambda: "scales_and_zeros must be bfloat16")
    torch._check(
        tuple(sz.shape) == (N, K // group_size, 2),
        lambda: f"scales_and_zeros must be [N, K/g, 2] = {(N, K // group_size, 2)}, got {tuple(sz.shape)}",
    )
    return N, K


@torch.library.register_fake("torchao::int4_dequantize")
def _(packed_w: Tensor, scales_and_zeros: Tensor, group_size: int, mode: int = 0) -> Tensor:
    N, K = _check_int4_weight(packed_w, scales_and_zeros, group_size)
    return packed_w.new_empty((N, K), dtype=torch.bfloat16)


def _int4_dequant_cuda(packed_w, scales_and_zeros, group_size, mode=0):
    N, K = _check_int4_weight(packed_w, scales_and_zeros, group_size)
    _same_device(packed_w, scales_and_zeros=scales_and_zeros)
    _require_contig(packed_w, "packed_w")
    _require_contig(scales_and_zeros, "scales_and_zeros")
    out = torch.empty((N, K), dtype=torch.bfloat16, device=packed_w.device)
    with torch.cuda.device(packed_w.device):
        _lib.call("tao_int4_dequant", _ptr(packed_w), _ptr(scales_and_zeros), _ptr(out), N, K,
                  group_size, int(mode), _stream(packed_w))
    return out


def _linear_out_shape(x: Tensor, N: int):
    return (*x.shape[:-1], N)


@torch.library.register_fake("torchao::int4_weight_only_linear")
def _(x, packed_w, scales_and_zeros, group_size, bias=None):
    N, K = _check_int4_weight(packed_w, scales_and_zeros, group_size)
    torch._check(x.dtype is torch.bfloat16, lambda: "int4 weight-only linear needs bf16 input")
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    return x.new_empty(_linear_out_shape(x, N))


def _int4_linear_cuda(x, packed_w, scales_and_zeros, group_size, bias=None):
    N, K = _check_int4_weight(packed_w, scales_and_zeros, group_size)
    torch._check(x.dtype is torch.bfloat16, lambda: "int4 weight-only linear needs bf16 input")
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    _same_device(x, packed_w=packed_w, scales_and_zeros=scales_and_zeros, bias=bias)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    _require_contig(packed_w, "packed_w")
    _require_contig(scales_and_zeros, "scales_and_zeros")
    with torch.cuda.device(x.device):
        _lib.call("tao_int4wo_linear_bf16", _ptr(x2), _ptr(packed_w), _ptr(scales_and_zeros),
                  _ptr(bias), _ptr(y), M, N, K, group_size, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


# ---------------------------------------------------------------------------------------------
# activation pre-scale (AWQ / SmoothQuant equalization scale)
# ---------------------------------------------------------------------------------------------
def _check_act_scale(x: Tensor, scale: Tensor, K: int, op: str):
    torch._check(x.dtype is torch.bfloat16, lambda: f"{op} (HIP) needs bf16 x, got {x.dtype}")
    torch._check(scale.dtype is torch.bfloat16,
                 lambda: f"{op} (HIP) needs a bf16 scale, got {scale.dtype}")
    torch._check(x.dim() >= 1 and x.size(-1) == K,
                 lambda: f"x last dim {x.size(-1) if x.dim() else 0} != K {K}")
    torch._check(scale.numel() == K,
                 lambda: f"scale must have K = {K} elements, got {scale.numel()}")


def _scale_row(scale: Tensor) -> Tensor:
    s = scale.reshape(-1)
    if not s.is_contiguous() or s.data_ptr() % 16:
        s = s.contiguous()
    return s


@torch.library.register_fake("torchao::act_prescale")
def _(x, scale):
    K = scale.numel()
    _check_act_scale(x, scale, K, "act_prescale")
    torch._check(K % 8 == 0, lambda: f"act_prescale needs K % 8 == 0, got K = {K}")
    return x.new_empty(x.shape)


def _act_prescale_cuda(x, scale):
    """bf16(x / scale) over the last dimension: IEEE fp32 division, one rounding (what
    ``input_tensor / scale`` gives for bf16 operands, linear_activation_scale.py:61-70)."""
    K = scale.numel()
    _check_act_scale(x, scale, K, "act_prescale")
    torch._check(K % 8 == 0, lambda: f"act_prescale needs K % 8 == 0, got K = {K}")
    _same_device(x, scale=scale)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    s = _scale_row(scale)
    y = torch.empty_like(x2)
    with torch.cuda.device(x.device):
        _lib.call("tao_act_prescale_bf16", _ptr(x2), _ptr(s), _ptr(y), x2.size(0), K, _stream(x))
    return y.reshape(x.shape)


@torch.library.register_fake("torchao::int4_prescaled_linear")
def _(x, act_scale, packed_w, scales_and_zeros, group_size, bias=None):
    N, K = _check_int4_weight(packed_w, scales_and_zeros, group_size)
    _check_act_scale(x, act_scale, K, "int4_prescaled_linear")
    return x.new_empty(_linear_out_shape(x, N))


def _int4_prescaled_linear_cuda(x, act_scale, packed_w, scales_and_zeros, group_size, bias=None):
    """The AWQ int4 linear from a bf16 activation. One token without a bias at K <= 4096 and
    N * K <= 2^24 (tao_int4wo_prescaled_linear_fused): the division and the GEMV in one launch.
    Otherwise act_prescale into a buffer of the caching allocator, then int4_weight_only_linear;
    bit-identical to calling the two ops."""
    N, K = _check_int4_weight(packed_w, scales_and_zeros, group_size)
    _check_act_scale(x, act_scale, K, "int4_prescaled_linear")
    _same_device(x, act_scale=act_scale, packed_w=packed_w, scales_and_zeros=scales_and_zeros,
                 bias=bias)
    _require_contig(packed_w, "packed_w")
    _require_contig(scales_and_zeros, "scales_and_zeros")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    s = _scale_row(act_scale)
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        if _lib.lib().tao_int4wo_prescaled_linear_fused(M, N, K, int(bias is not None)):
            _lib.call("tao_int4wo_prescaled_linear_bf16", _ptr(x2), _ptr(s), _ptr(packed_w),
                      _ptr(scales_and_zeros), _ptr(None), _ptr(y), 1, N, K, group_size, _stream(x))
        elif M > 0:
            xs = torch.empty_like(x2)
            _lib.call("tao_act_prescale_bf16", _ptr(x2), _ptr(s), _ptr(xs), M, K, _stream(x))
            _lib.call("tao_int4wo_linear_bf16", _ptr(xs), _ptr(packed_w), _ptr(scales_and_zeros),
                      _ptr(bias), _ptr(y), M, N, K, group_size, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


# ---------------------------------------------------------------------------------------------
# int8 weight-only and dynamic activation
# ---------------------------------------------------------------------------------------------
def _check_int8_weight(w: Tensor, scale: Tensor):
    torch._check(w.dim() == 2 and w.dtype is torch.int8, lambda: "w must be a 2D int8 tensor")
    torch._check(scale.numel() == w.size(0), lambda: "scale must have N elements")
    return w.shape


@torch.library.register_fake("torchao::int8_weight_only_linear")
def _(x, w_int8, scale, bias=None):
    N, K = _check_int8_weight(w_int8, scale)
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    return x.new_empty(_linear_out_shape(x, N))


def _int8wo_linear_cuda(x, w_int8, scale, bias=None):
    N, K = _check_int8_weight(w_int8, scale)
    torch._check(x.dtype is torch.bfloat16, lambda: "int8 weight-only linear (HIP) needs bf16 x")
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    _same_device(x, w_int8=w_int8, scale=scale, bias=bias)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    w_int8 = w_int8.contiguous()
    scale = scale.reshape(-1).to(torch.bfloat16).contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    with torch.cuda.device(x.device):
        _lib.call("tao_int8wo_linear_bf16", _ptr(x2), _ptr(w_int8), _ptr(scale), _ptr(bias),
                  _ptr(y), M, N, K, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


@torch.library.register_fake("torchao::int8_quantize_per_token")
def _(x):
    return (
        x.new_empty(x.shape, dtype=torch.int8),
        x.new_empty((*x.shape[:-1], 1), dtype=torch.bfloat16),
    )


def _int8_quant_cuda(x: Tensor) -> Tuple[Tensor, Tensor]:
    torch._check(x.dtype is torch.bfloat16, lambda: "int8 per-token quant (HIP) needs bf16 x")
    K = x.size(-1)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    q = torch.empty((M, K), dtype=torch.int8, device=x.device)
    s = torch.empty((M, 1), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("tao_int8_quant_per_token", _ptr(x2), _ptr(q), _ptr(s), M, K, _stream(x))
    return q.reshape(x.shape), s.reshape(*x.shape[:-1], 1)


@torch.library.register_fake("torchao::int8_scaled_mm")
def _(x_int8, x_scale, w_int8, w_scale, bias=None):
    N, K = _check_int8_weight(w_int8, w_scale)
    return x_int8.new_empty(_linear_out_shape(x_int8, N), dtype=torch.bfloat16)


def _int8_scaled_mm_cuda(x_int8, x_scale, w_int8, w_scale, bias=None):
    N, K = _check_int8_weight(w_int8, w_scale)
    torch._check(x_int8.dtype is torch.int8, lambda: "x_int8 must be int8")
    torch._check(x_int8.size(-1) == K, lambda: f"x last dim {x_int8.size(-1)} != K {K}")
    _same_device(x_int8, x_scale=x_scale, w_int8=w_int8, w_scale=w_scale, bias=bias)
    x2 = x_int8.reshape(-1, K).contiguous()
    M = x2.size(0)
    xs = x_scale.reshape(-1).to(torch.bfloat16).contiguous()
    torch._check(xs.numel() == M, lambda: "x_scale must have one entry per row")
    ws = w_scale.reshape(-1).to(torch.bfloat16).contiguous()
    w_int8 = w_int8.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x_int8.device)
    with torch.cuda.device(x_int8.device):
        _lib.call("tao_int8_scaled_mm_bf16", _ptr(x2), _ptr(xs), _ptr(w_int8), _ptr(ws),
                  _ptr(bias), _ptr(y), M, N, K, _stream(x_int8))
    return y.reshape(_linear_out_shape(x_int8, N))


@torch.library.register_fake("torchao::int8_dyn_linear")
def _(x, w_int8, w_scale, bias=None):
    N, K = _check_int8_weight(w_int8, w_scale)
    torch._check(x.numel() == K, lambda: "int8_dyn_linear is one token (x.numel() == K)")
    return x.new_empty(_linear_out_shape(x, N), dtype=torch.bfloat16)


def _int8_dyn_linear_cuda(x, w_int8, w_scale, bias=None):
    """One token: per-token int8 quant + int8 x int8 GEMV in one launch, bit-identical to
    int8_quantize_per_token -> int8_scaled_mm."""
    N, K = _check_int8_weight(w_int8, w_scale)
    torch._check(x.dtype is torch.bfloat16, lambda: "int8_dyn_linear (HIP) needs bf16 x")
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    torch._check(x.numel() == K, lambda: "int8_dyn_linear is one token (x.numel() == K)")
    _same_device(x, w_int8=w_int8, w_scale=w_scale, bias=bias)
    x2 = x.reshape(1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    ws = w_scale.reshape(-1).to(torch.bfloat16).contiguous()
    w_int8 = w_int8.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((1, N), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("tao_int8_dyn_linear_bf16", _ptr(x2), _ptr(w_int8), _ptr(ws), _ptr(bias),
                  _ptr(y), 1, N, K, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


# ---------------------------------------------------------------------------------------------
# SmoothQuant: fused smooth + quantize, and the linear on top (prototype/smoothquant)
# ---------------------------------------------------------------------------------------------
def _check_smooth(x: Tensor, smooth: Tensor, act_scale: Optional[Tensor], K: int, op: str):
    _check_act_scale(x, smooth, K, op)
    torch._check(K % 16 == 0 and 0 < K <= 65536,
                 lambda: f"{op} needs K % 16 == 0 and 0 < K <= 65536, got K = {K}")
    if act_scale is not None:
        torch._check(act_scale.dtype is torch.bfloat16 and act_scale.numel() == 1,
                     lambda: f"{op} needs a bf16 act_scale of one element, got "
                             f"{act_scale.dtype} with {act_scale.numel()}")


def _smooth_quant_fake(x, smooth, act_scale, op):
    K = smooth.numel()
    _check_smooth(x, smooth, act_scale, K, op)
    return x.new_empty(x.shape, dtype=torch.int8), x.new_empty((x.numel() // K,))


@torch.library.register_fake("torchao::int8_smooth_quantize_per_token")
def _(x, smooth):
    return _smooth_quant_fake(x, smooth, None, "int8_smooth_quantize_per_token")


@torch.library.register_fake("torchao::int8_smooth_quantize_static")
def _(x, smooth, act_scale):
    return _smooth_quant_fake(x, smooth, act_scale, "int8_smooth_quantize_static")


def _smooth_linear_fake(x, smooth, act_scale, w_int8, w_scale, op):
    N, K = _check_int8_weight(w_int8, w_scale)
    _check_smooth(x, smooth, act_scale, K, op)
    return x.new_empty(_linear_out_shape(x, N))


@torch.library.register_fake("torchao::int8_smooth_dyn_linear")
def _(x, smooth, w_int8, w_scale, bias=None):
    return _smooth_linear_fake(x, smooth, None, w_int8, w_scale, "int8_smooth_dyn_linear")


@torch.library.register_fake("torchao::int8_smooth_static_linear")
def _(x, smooth, act_scale, w_int8, w_scale, bias=None):
    return _smooth_linear_fake(x, smooth, act_scale, w_int8, w_scale,
                               "int8_smooth_static_linear")


def _smooth_operands(x, smooth, act_scale, K):
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    if act_scale is not None:
        act_scale = act_scale.reshape(1).contiguous()
    return x2, _scale_row(smooth), act_scale


def _int8_smooth_quant_cuda(x, smooth, act_scale, op):
    """bf16(x / smooth), then the per-token (act_scale None; 2^-7 scale clamp) or static int8
    codes, in one launch: (q int8 like x, scale bf16 [M])."""
    K = smooth.numel()
    _check_smooth(x, smooth, act_scale, K, op)
    _same_device(x, smooth=smooth, act_scale=act_scale)
    x2, s, a = _smooth_operands(x, smooth, act_scale, K)
    M = x2.size(0)
    q = torch.empty((M, K), dtype=torch.int8, device=x.device)
    sc = torch.empty((M,), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("tao_int8_smooth_quant_bf16", _ptr(x2), _ptr(s), _ptr(a), _ptr(q), _ptr(sc), M,
                  K, _stream(x))
    return q.reshape(x.shape), sc


def _int8_smooth_quant_per_token_cuda(x, smooth):
    return _int8_smooth_quant_cuda(x, smooth, None, "int8_smooth_quantize_per_token")


def _int8_smooth_quant_static_cuda(x, smooth, act_scale):
    return _int8_smooth_quant_cuda(x, smooth, act_scale, "int8_smooth_quantize_static")


def _int8_smooth_linear_cuda(x, smooth, act_scale, w_int8, w_scale, bias, op):
    """The SmoothQuant int8 linear from a bf16 activation. One token where
    tao_int8_smooth_linear_fused says so: one launch. Otherwise the fused quantizer into buffers
    of the caching allocator, then int8_scaled_mm's entry; bit-identical."""
    N, K = _check_int8_weight(w_int8, w_scale)
    _check_smooth(x, smooth, act_scale, K, op)
    _same_device(x, smooth=smooth, act_scale=act_scale, w_int8=w_int8, w_scale=w_scale, bias=bias)
    x2, s, a = _smooth_operands(x, smooth, act_scale, K)
    M = x2.size(0)
    ws = w_scale.reshape(-1).to(torch.bfloat16).contiguous()
    w_int8 = w_int8.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        if _lib.lib().tao_int8_smooth_linear_fused(M, N, K, int(a is not None)):
            _lib.call("tao_int8_smooth_linear_bf16", _ptr(x2), _ptr(s), _ptr(a), _ptr(w_int8),
                      _ptr(ws), _ptr(bias), _ptr(y), 1, N, K, _stream(x))
        elif M > 0:
            q = torch.empty((M, K), dtype=torch.int8, device=x.device)
            sc = torch.empty((M,), dtype=torch.bfloat16, device=x.device)
            _lib.call("tao_int8_smooth_quant_bf16", _ptr(x2), _ptr(s), _ptr(a), _ptr(q), _ptr(sc),
                      M, K, _stream(x))
            _lib.call("tao_int8_scaled_mm_bf16", _ptr(q), _ptr(sc), _ptr(w_int8), _ptr(ws),
                      _ptr(bias), _ptr(y), M, N, K, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


def _int8_smooth_dyn_linear_cuda(x, smooth, w_int8, w_scale, bias=None):
    return _int8_smooth_linear_cuda(x, smooth, None, w_int8, w_scale, bias,
                                    "int8_smooth_dyn_linear")


def _int8_smooth_static_linear_cuda(x, smooth, act_scale, w_int8, w_scale, bias=None):
    return _int8_smooth_linear_cuda(x, smooth, act_scale, w_int8, w_scale, bias,
                                    "int8_smooth_static_linear")


@torch.library.register_fake("torchao::int4_quantize_pack")
def _(w, group_size, eps):
    torch._check(group_size in _GROUP_SIZES, lambda: "group_size must be 32, 64, 128, or 256")
    K = w.size(-1)
    torch._check(K % group_size == 0, lambda: f"K ({K}) must be divisible by group_size")
    lead = w.shape[:-1]
    return (w.new_empty((*lead, K // 8), dtype=torch.int32),
            w.new_empty((*lead, K // group_size, 2), dtype=torch.bfloat16))


def _int4_quantize_pack_cuda(w: Tensor, group_size: int, eps: float):
    """bf16 W [..., K] -> (packed int32 [..., K/8], scales_and_zeros bf16 [..., K/g, 2])."""
    torch._check(w.dtype is torch.bfloat16, lambda: "int4 quantize (HIP) needs a bf16 weight")
    torch._check(group_size in _GROUP_SIZES, lambda: "group_size must be 32, 64, 128, or 256")
    K = w.size(-1)
    torch._check(K % group_size == 0, lambda: f"K ({K}) must be divisible by group_size")
    w2 = w.reshape(-1, K)
    if not w2.is_contiguous() or w2.data_ptr() % 16:
        w2 = w2.contiguous()
    R = w2.size(0)
    packed = torch.empty((R, K // 8), dtype=torch.int32, device=w.device)
    sz = torch.empty((R, K // group_size, 2), dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("tao_int4_quantize_bf16", _ptr(w2), _ptr(packed), _ptr(sz), R, K, group_size,
                  ctypes.c_float(eps), _stream(w))
    lead = w.shape[:-1]
    return packed.reshape(*lead, K // 8), sz.reshape(*lead, K // group_size, 2)


@torch.library.register_fake("torchao::int4_hqq_quantize_pack")
def _(w, group_size):
    torch._check(w.dim() in (2, 3), lambda: "int4 hqq quantize: w must be [N, K] or [E, N, K]")
    torch._check(group_size in _GROUP_SIZES, lambda: "group_size must be 32, 64, 128, or 256")
    K = w.size(-1)
    torch._check(K % group_size == 0, lambda: f"K ({K}) must be divisible by group_size")
    lead = w.shape[:-1]
    return (w.new_empty((*lead, K // 8), dtype=torch.int32),
            w.new_empty((*lead, K // group_size, 2), dtype=torch.bfloat16),
            w.new_empty((1,), dtype=torch.int32))


def _int4_hqq_quantize_pack_cuda(w: Tensor, group_size: int):
    """bf16 W [(E,) N, K] -> (packed int32 [..., K/8], scales_and_zeros bf16 [..., K/g, 2],
    iterations run int32 [1]). The scratch comes from the caching allocator: stream-ordered, so a
    later call may reuse it, and a captured graph keeps its own."""
    torch._check(w.dtype is torch.bfloat16, lambda: "int4 hqq quantize (HIP) needs a bf16 weight")
    torch._check(w.dim() in (2, 3), lambda: "int4 hqq quantize: w must be [N, K] or [E, N, K]")
    torch._check(group_size in _GROUP_SIZES, lambda: "group_size must be 32, 64, 128, or 256")
    K = w.size(-1)
    torch._check(K % group_size == 0, lambda: f"K ({K}) must be divisible by group_size")
    w2 = w.reshape(-1, K)
    if not w2.is_contiguous() or w2.data_ptr() % 16:
        w2 = w2.contiguous()
    R = w2.size(0)
    packed = torch.empty((R, K // 8), dtype=torch.int32, device=w.device)
    sz = torch.empty((R, K // group_size, 2), dtype=torch.bfloat16, device=w.device)
    iters = torch.empty((1,), dtype=torch.int32, device=w.device)
    nbytes = _lib.lib().tao_int4_hqq_scratch_bytes(R, K)
    scratch = torch.empty((max(nbytes // 8, 1),), dtype=torch.float64, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("tao_int4_hqq_quantize_bf16", _ptr(w2), _ptr(packed), _ptr(sz), _ptr(iters),
                  _ptr(scratch), R, K, group_size, _stream(w))
    lead = w.shape[:-1]
    return packed.reshape(*lead, K // 8), sz.reshape(*lead, K // group_size, 2), iters


@torch.library.register_fake("torchao::int8_quantize_rows")
def _(w, eps):
    return (w.new_empty(w.shape, dtype=torch.int8),
            w.new_empty(w.shape[:-1], dtype=torch.bfloat16))


def _int8_quantize_rows_cuda(w: Tensor, eps: float):
    """bf16 W [..., K] -> (int8 [..., K], per-row scale bf16 [...]), symmetric [-128, 127]."""
    torch._check(w.dtype is torch.bfloat16, lambda: "int8 quantize (HIP) needs a bf16 weight")
    K = w.size(-1)
    torch._check(K % 8 == 0, lambda: f"K ({K}) must be a multiple of 8")
    w2 = w.reshape(-1, K)
    if not w2.is_contiguous() or w2.data_ptr() % 16:
        w2 = w2.contiguous()
    R = w2.size(0)
    q = torch.empty((R, K), dtype=torch.int8, device=w.device)
    s = torch.empty((R,), dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("tao_int8_quantize_rows_bf16", _ptr(w2), _ptr(q), _ptr(s), R, K,
                  ctypes.c_float(eps), _stream(w))
    return q.reshape(w.shape), s.reshape(w.shape[:-1])


# ---------------------------------------------------------------------------------------------
# float8 (e4m3fn) weight-only
# ---------------------------------------------------------------------------------------------
def _check_fp8_weight(w: Tensor, scale: Tensor):
    torch._check(w.dim() == 2 and w.dtype is torch.float8_e4m3fn,
                 lambda: "w must be a 2D float8_e4m3fn tensor")
    torch._check(scale.numel() == w.size(0), lambda: "scale must have N elements")
    return w.shape


@torch.library.register_fake("torchao::fp8_weight_only_linear")
def _(x, w_fp8, scale, bias=None):
    N, K = _check_fp8_weight(w_fp8, scale)
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    return x.new_empty(_linear_out_shape(x, N), dtype=torch.bfloat16)


def _fp8wo_linear_cuda(x, w_fp8, scale, bias=None):
    N, K = _check_fp8_weight(w_fp8, scale)
    torch._check(x.dtype is torch.bfloat16, lambda: "fp8 weight-only linear (HIP) needs bf16 x")
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    _same_device(x, w_fp8=w_fp8, scale=scale, bias=bias)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    w_fp8 = w_fp8.contiguous()
    scale = scale.reshape(-1).to(torch.float32).contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    with torch.cuda.device(x.device):
        _lib.call("tao_fp8wo_linear_bf16", _ptr(x2), _ptr(w_fp8), _ptr(scale), _ptr(bias),
                  _ptr(y), M, N, K, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


@torch.library.register_fake("torchao::fp8_quantize_rows")
def _(w):
    torch._check(w.size(-1) % 8 == 0, lambda: f"K ({w.size(-1)}) must be a multiple of 8")
    return (w.new_empty(w.shape, dtype=torch.float8_e4m3fn),
            w.new_empty((*w.shape[:-1], 1), dtype=torch.float32))


def _fp8_quantize_rows_cuda(w: Tensor):
    """bf16 W [..., K] -> (e4m3fn [..., K], per-row scale fp32 [..., 1]); no eps."""
    torch._check(w.dtype is torch.bfloat16, lambda: "fp8 quantize (HIP) needs a bf16 weight")
    K = w.size(-1)
    torch._check(K % 8 == 0, lambda: f"K ({K}) must be a multiple of 8")
    w2 = w.reshape(-1, K)
    if not w2.is_contiguous() or w2.data_ptr() % 16:
        w2 = w2.contiguous()
    R = w2.size(0)
    q = torch.empty((R, K), dtype=torch.float8_e4m3fn, device=w.device)
    s = torch.empty((R,), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("tao_fp8_quantize_rows_bf16", _ptr(w2), _ptr(q), _ptr(s), R, K, _stream(w))
    return q.reshape(w.shape), s.reshape(*w.shape[:-1], 1)


@torch.library.register_fake("torchao::fp8_dequantize")
def _(q, scale):
    N, K = _check_fp8_weight(q, scale)
    torch._check(K % 8 == 0, lambda: f"K ({K}) must be a multiple of 8")
    return q.new_empty((N, K), dtype=torch.bfloat16)


def _fp8_dequantize_cuda(q: Tensor, scale: Tensor):
    """e4m3fn [N, K] x per-row fp32 scale -> bf16 [N, K] = bf16(float(q) * scale)."""
    N, K = _check_fp8_weight(q, scale)
    torch._check(K % 8 == 0, lambda: f"K ({K}) must be a multiple of 8")
    _same_device(q, scale=scale)
    q = q.contiguous()
    scale = scale.reshape(-1).to(torch.float32).contiguous()
    out = torch.empty((N, K), dtype=torch.bfloat16, device=q.device)
    with torch.cuda.device(q.device):
        _lib.call("tao_fp8_dequant_bf16", _ptr(q), _ptr(scale), _ptr(out), N, K, _stream(q))
    return out


# ---------------------------------------------------------------------------------------------
# float8 (e4m3fn) dynamic activation x float8 weight, per-row scales
# ---------------------------------------------------------------------------------------------
@torch.library.register_fake("torchao::fp8_scaled_mm")
def _(xq, x_scale, w_fp8, w_scale, bias=None):
    N, K = _check_fp8_weight(w_fp8, w_scale)
    torch._check(xq.size(-1) == K, lambda: f"x last dim {xq.size(-1)} != K {K}")
    return xq.new_empty(_linear_out_shape(xq, N), dtype=torch.bfloat16)


def _fp8_scaled_mm_cuda(xq, x_scale, w_fp8, w_scale, bias=None):
    """y = bf16(((f(xq) @ f(w)^T) * x_scale[m]) * w_scale[n] + bias), fp32 up to the one
    rounding (include/torchao_mi355x.h tao_fp8_scaled_mm_bf16)."""
    N, K = _check_fp8_weight(w_fp8, w_scale)
    torch._check(xq.dtype is torch.float8_e4m3fn, lambda: "xq must be float8_e4m3fn")
    torch._check(xq.size(-1) == K, lambda: f"x last dim {xq.size(-1)} != K {K}")
    torch._check(K % 16 == 0, lambda: f"K ({K}) must be a multiple of 16")
    _same_device(xq, x_scale=x_scale, w_fp8=w_fp8, w_scale=w_scale, bias=bias)
    x2 = xq.reshape(-1, K).contiguous()
    M = x2.size(0)
    xs = x_scale.reshape(-1).to(torch.float32).contiguous()
    torch._check(xs.numel() == M, lambda: "x_scale must have one entry per row")
    ws = w_scale.reshape(-1).to(torch.float32).contiguous()
    w_fp8 = w_fp8.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=xq.device)
    with torch.cuda.device(xq.device):
        _lib.call("tao_fp8_scaled_mm_bf16", _ptr(x2), _ptr(xs), _ptr(w_fp8), _ptr(ws),
                  _ptr(bias), _ptr(y), M, N, K, _stream(xq))
    return y.reshape(_linear_out_shape(xq, N))


@torch.library.register_fake("torchao::fp8_dyn_linear")
def _(x, w_fp8, w_scale, bias=None):
    N, K = _check_fp8_weight(w_fp8, w_scale)
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    return x.new_empty(_linear_out_shape(x, N), dtype=torch.bfloat16)


def _fp8_dyn_linear_cuda(x, w_fp8, w_scale, bias=None):
    """The whole linear from a bf16 activation. One token: quantisation + GEMV in one launch.
    More: fp8_quantize_rows (rows = tokens) into a buffer of the caching allocator, then
    fp8_scaled_mm; bit-identical to calling the two ops."""
    N, K = _check_fp8_weight(w_fp8, w_scale)
    torch._check(x.dtype is torch.bfloat16, lambda: "fp8_dyn_linear (HIP) needs bf16 x")
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    torch._check(K % 16 == 0, lambda: f"K ({K}) must be a multiple of 16")
    _same_device(x, w_fp8=w_fp8, w_scale=w_scale, bias=bias)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    ws = w_scale.reshape(-1).to(torch.float32).contiguous()
    w_fp8 = w_fp8.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        if M == 1 and K <= 65536:
            _lib.call("tao_fp8_dyn_linear_bf16", _ptr(x2), _ptr(w_fp8), _ptr(ws), _ptr(bias),
                      _ptr(y), 1, N, K, _stream(x))
        elif M > 0:
            q = torch.empty((M, K), dtype=torch.float8_e4m3fn, device=x.device)
            s = torch.empty((M,), dtype=torch.float32, device=x.device)
            _lib.call("tao_fp8_quantize_rows_bf16", _ptr(x2), _ptr(q), _ptr(s), M, K, _stream(x))
            _lib.call("tao_fp8_scaled_mm_bf16", _ptr(q), _ptr(s), _ptr(w_fp8), _ptr(ws),
                      _ptr(bias), _ptr(y), M, N, K, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


# ---------------------------------------------------------------------------------------------
# MXFP8: e4m3fn codes with one E8M0 scale byte per 32-element block (csrc/mx_fp8.hip)
# ---------------------------------------------------------------------------------------------
def _check_mx_operand(q, scale, qn, sn):
    torch._check(q.dtype is torch.float8_e4m3fn, lambda: f"{qn} must be float8_e4m3fn")
    torch._check(scale.dtype is torch.uint8, lambda: f"{sn} must be uint8 (E8M0 bytes)")
    K = q.size(-1)
    torch._check(K % 32 == 0, lambda: f"K ({K}) must be a multiple of 32")
    torch._check(
        scale.numel() * 32 == q.numel() and (scale.dim() == 0 or scale.size(-1) == K // 32),
        lambda: f"{sn} must hold one byte per 32-element block: [..., K/32] = [..., {K // 32}], "
                f"got {tuple(scale.shape)}")
    return K


def _mx_scale_rows(s, K):
    """Scale bytes as [rows, K/32], contiguous and 8-B aligned (the MFMA route's 8-B loads)."""
    s2 = s.reshape(-1, K // 32)
    return s2 if s2.is_contiguous() and s2.data_ptr() % 8 == 0 else s2.clone()


def _check_mx_weight(wq, w_scale):
    torch._check(wq.dim() == 2, lambda: "wq must be a 2D float8_e4m3fn tensor")
    return wq.size(0), _check_mx_operand(wq, w_scale, "wq", "w_scale")


@torch.library.register_fake("torchao::mx_quantize_rows")
def _(x):
    K = x.size(-1)
    torch._check(K % 32 == 0, lambda: f"K ({K}) must be a multiple of 32")
    return (x.new_empty(x.shape, dtype=torch.float8_e4m3fn),
            x.new_empty((*x.shape[:-1], K // 32), dtype=torch.uint8))


def _mx_quantize_rows_cuda(x: Tensor):
    """bf16 x [..., K] -> (e4m3fn codes [..., K], E8M0 bytes uint8 [..., K/32]); to_mx, FLOOR."""
    torch._check(x.dtype is torch.bfloat16, lambda: "mx quantize (HIP) needs bf16 x")
    torch._check(x.dim() >= 1, lambda: "mx quantize: x must have at least one dimension")
    K = x.size(-1)
    torch._check(K % 32 == 0, lambda: f"K ({K}) must be a multiple of 32")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    q = torch.empty((M, K), dtype=torch.float8_e4m3fn, device=x.device)
    s = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("tao_mx_quantize_rows_bf16", _ptr(x2), _ptr(q), _ptr(s), M, K, _stream(x))
    return q.reshape(x.shape), s.reshape(*x.shape[:-1], K // 32)


@torch.library.register_fake("torchao::mx_scaled_mm")
def _(xq, x_scale, wq, w_scale, bias=None):
    N, K = _check_mx_weight(wq, w_scale)
    torch._check(xq.size(-1) == K, lambda: f"x last dim {xq.size(-1)} != K {K}")
    return xq.new_empty(_linear_out_shape(xq, N), dtype=torch.bfloat16)


def _mx_scaled_mm_cuda(xq, x_scale, wq, w_scale, bias=None):
    """y = bf16(sum_b 2^(xs-127) 2^(ws-127) (f(xq) . f(wq))_b + bias), fp32 up to the one rounding
    (include/torchao_mi355x.h tao_mx_scaled_mm_bf16)."""
    N, K = _check_mx_weight(wq, w_scale)
    torch._check(xq.dim() >= 1 and xq.size(-1) == K,
                 lambda: f"x last dim {xq.size(-1) if xq.dim() else 0} != K {K}")
    _check_mx_operand(xq, x_scale, "xq", "x_scale")
    _same_device(xq, x_scale=x_scale, wq=wq, w_scale=w_scale, bias=bias)
    x2 = xq.reshape(-1, K).contiguous()
    M = x2.size(0)
    xs = _mx_scale_rows(x_scale, K)
    ws = _mx_scale_rows(w_scale, K)
    wq = wq.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=xq.device)
    with torch.cuda.device(xq.device):
        _lib.call("tao_mx_scaled_mm_bf16", _ptr(x2), _ptr(xs), _ptr(wq), _ptr(ws), _ptr(bias),
                  _ptr(y), M, N, K, _stream(xq))
    return y.reshape(_linear_out_shape(xq, N))


@torch.library.register_fake("torchao::mx_dyn_linear")
def _(x, wq, w_scale, bias=None):
    N, K = _check_mx_weight(wq, w_scale)
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    return x.new_empty(_linear_out_shape(x, N), dtype=torch.bfloat16)


def _mx_dyn_linear_cuda(x, wq, w_scale, bias=None):
    """The whole linear from a bf16 activation. One token: block quantisation + GEMV in one
    launch. More: mx_quantize_rows into buffers of the caching allocator, then mx_scaled_mm;
    bit-identical to calling the two ops."""
    N, K = _check_mx_weight(wq, w_scale)
    torch._check(x.dtype is torch.bfloat16, lambda: "mx_dyn_linear (HIP) needs bf16 x")
    torch._check(x.dim() >= 1 and x.size(-1) == K,
                 lambda: f"x last dim {x.size(-1) if x.dim() else 0} != K {K}")
    _same_device(x, wq=wq, w_scale=w_scale, bias=bias)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    ws = _mx_scale_rows(w_scale, K)
    wq = wq.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        if M == 1 and K <= 65536:
            _lib.call("tao_mx_dyn_linear_bf16", _ptr(x2), _ptr(wq), _ptr(ws), _ptr(bias),
                      _ptr(y), 1, N, K, _stream(x))
        elif M > 0:
            q = torch.empty((M, K), dtype=torch.float8_e4m3fn, device=x.device)
            s = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
            _lib.call("tao_mx_quantize_rows_bf16", _ptr(x2), _ptr(q), _ptr(s), M, K, _stream(x))
            _lib.call("tao_mx_scaled_mm_bf16", _ptr(q), _ptr(s), _ptr(wq), _ptr(ws), _ptr(bias),
                      _ptr(y), M, N, K, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


# ---------------------------------------------------------------------------------------------
# MXFP4 weights under MXFP8 activations: e2m1 codes, two per byte (element 2 j in the high nibble),
# one E8M0 scale byte per 32-element block (csrc/mx_fp4.hip)
# ---------------------------------------------------------------------------------------------
def _check_mxfp4_weight(wq, w_scale):
    torch._check(wq.dim() == 2 and wq.dtype is torch.uint8,
                 lambda: "wq must be a 2D uint8 tensor of packed e2m1 codes [N, K/2]")
    torch._check(w_scale.dtype is torch.uint8, lambda: "w_scale must be uint8 (E8M0 bytes)")
    K = 2 * wq.size(1)
    torch._check(K % 32 == 0, lambda: f"K ({K}) must be a multiple of 32")
    torch._check(
        w_scale.numel() * 32 == 2 * wq.numel()
        and (w_scale.dim() == 0 or w_scale.size(-1) == K // 32),
        lambda: f"w_scale must hold one byte per 32-element block: [..., K/32] = [..., {K // 32}], "
                f"got {tuple(w_scale.shape)}")
    return wq.size(0), K


@torch.library.register_fake("torchao::mxfp4_quantize_rows")
def _(x):
    K = x.size(-1)
    torch._check(K % 32 == 0, lambda: f"K ({K}) must be a multiple of 32")
    return (x.new_empty((*x.shape[:-1], K // 2), dtype=torch.uint8),
            x.new_empty((*x.shape[:-1], K // 32), dtype=torch.uint8))


def _mxfp4_quantize_rows_cuda(x: Tensor):
    """bf16 x [..., K] -> (packed e2m1 codes uint8 [..., K/2], E8M0 bytes uint8 [..., K/32]);
    to_mx with float4_e2m1fn_x2, FLOOR."""
    torch._check(x.dtype is torch.bfloat16, lambda: "mxfp4 quantize (HIP) needs bf16 x")
    torch._check(x.dim() >= 1, lambda: "mxfp4 quantize: x must have at least one dimension")
    K = x.size(-1)
    torch._check(K % 32 == 0, lambda: f"K ({K}) must be a multiple of 32")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    q = torch.empty((M, K // 2), dtype=torch.uint8, device=x.device)
    s = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("tao_mxfp4_quantize_rows_bf16", _ptr(x2), _ptr(q), _ptr(s), M, K, _stream(x))
    return q.reshape(*x.shape[:-1], K // 2), s.reshape(*x.shape[:-1], K // 32)


@torch.library.register_fake("torchao::mxfp4w_scaled_mm")
def _(xq, x_scale, wq, w_scale, bias=None):
    N, K = _check_mxfp4_weight(wq, w_scale)
    torch._check(xq.size(-1) == K, lambda: f"x last dim {xq.size(-1)} != K {K}")
    return xq.new_empty(_linear_out_shape(xq, N), dtype=torch.bfloat16)


def _mxfp4w_scaled_mm_cuda(xq, x_scale, wq, w_scale, bias=None):
    """y = bf16(sum_b 2^(xs-127) 2^(ws-127) (e4m3(xq) . e2m1(wq))_b + bias), fp32 up to the one
    rounding (include/torchao_mi355x.h tao_mxfp4w_scaled_mm_bf16)."""
    N, K = _check_mxfp4_weight(wq, w_scale)
    torch._check(xq.dim() >= 1 and xq.size(-1) == K,
                 lambda: f"x last dim {xq.size(-1) if xq.dim() else 0} != K {K}")
    _check_mx_operand(xq, x_scale, "xq", "x_scale")
    _same_device(xq, x_scale=x_scale, wq=wq, w_scale=w_scale, bias=bias)
    x2 = xq.reshape(-1, K).contiguous()
    M = x2.size(0)
    xs = _mx_scale_rows(x_scale, K)
    ws = _mx_scale_rows(w_scale, K)
    wq = wq.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=xq.device)
    with torch.cuda.device(xq.device):
        _lib.call("tao_mxfp4w_scaled_mm_bf16", _ptr(x2), _ptr(xs), _ptr(wq), _ptr(ws),
                  _ptr(bias), _ptr(y), M, N, K, _stream(xq))
    return y.reshape(_linear_out_shape(xq, N))


@torch.library.register_fake("torchao::mxfp4w_dyn_linear")
def _(x, wq, w_scale, bias=None):
    N, K = _check_mxfp4_weight(wq, w_scale)
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    return x.new_empty(_linear_out_shape(x, N), dtype=torch.bfloat16)


def _mxfp4w_dyn_linear_cuda(x, wq, w_scale, bias=None):
    """The whole linear from a bf16 activation. One token: the e4m3fn block quantisation + GEMV in
    one launch. More: mx_quantize_rows into buffers of the caching allocator, then
    mxfp4w_scaled_mm; bit-identical to calling the two ops."""
    N, K = _check_mxfp4_weight(wq, w_scale)
    torch._check(x.dtype is torch.bfloat16, lambda: "mxfp4w_dyn_linear (HIP) needs bf16 x")
    torch._check(x.dim() >= 1 and x.size(-1) == K,
                 lambda: f"x last dim {x.size(-1) if x.dim() else 0} != K {K}")
    _same_device(x, wq=wq, w_scale=w_scale, bias=bias)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    ws = _mx_scale_rows(w_scale, K)
    wq = wq.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        if M == 1 and K <= 65536:
            _lib.call("tao_mxfp4w_dyn_linear_bf16", _ptr(x2), _ptr(wq), _ptr(ws), _ptr(bias),
                      _ptr(y), 1, N, K, _stream(x))
        elif M > 0:
            q = torch.empty((M, K), dtype=torch.float8_e4m3fn, device=x.device)
            s = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
            _lib.call("tao_mx_quantize_rows_bf16", _ptr(x2), _ptr(q), _ptr(s), M, K, _stream(x))
            _lib.call("tao_mxfp4w_scaled_mm_bf16", _ptr(q), _ptr(s), _ptr(wq), _ptr(ws),
                      _ptr(bias), _ptr(y), M, N, K, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


# ---------------------------------------------------------------------------------------------
# Blockwise float8 (torchao.prototype.blockwise_fp8_inference): e4m3fn codes, one fp32 scale per
# 1 x 128 block of the activation and per 128 x 128 block of the weight (csrc/block_fp8.hip)
# ---------------------------------------------------------------------------------------------
def _check_blockfp8_k(t, name):
    torch._check(t.dim() >= 1, lambda: f"{name} must have at least one dimension")
    K = t.size(-1)
    torch._check(K % 128 == 0, lambda: f"K ({K}) must be a multiple of 128 (blockwise float8 "
                                       f"serves block size 128 only)")
    return K


def _check_blockfp8_act(xq, x_scale):
    torch._check(xq.dtype is torch.float8_e4m3fn, lambda: "xq must be float8_e4m3fn")
    torch._check(x_scale.dtype is torch.float32, lambda: "x_scale must be float32")
    K = _check_blockfp8_k(xq, "xq")
    torch._check(
        x_scale.numel() * 128 == xq.numel() and (x_scale.dim() == 0 or x_scale.size(-1) == K // 128),
        lambda: f"x_scale must hold one float32 per 1x128 block: [..., K/128] = [..., {K // 128}], "
                f"got {tuple(x_scale.shape)}")


def _check_blockfp8_weight(wq, w_scale):
    torch._check(wq.dim() == 2 and wq.dtype is torch.float8_e4m3fn,
                 lambda: "wq must be a 2D float8_e4m3fn tensor")
    torch._check(w_scale.dtype is torch.float32, lambda: "w_scale must be float32")
    N, K = wq.size(0), _check_blockfp8_k(wq, "wq")
    NB = (N + 127) // 128
    torch._check(
        w_scale.dim() == 2 and w_scale.size(0) == NB and w_scale.size(1) == K // 128,
        lambda: f"w_scale must hold one float32 per 128x128 block: [ceil(N/128), K/128] = "
                f"[{NB}, {K // 128}], got {tuple(w_scale.shape)}")
    return N, K


def _check_blockfp8_bias(bias, N):
    torch._check(bias is None or (bias.dtype is torch.bfloat16 and bias.numel() == N),
                 lambda: "bias must be bfloat16 with N elements")


@torch.library.register_fake("torchao::blockfp8_quantize_act")
def _(x):
    K = _check_blockfp8_k(x, "x")
    return (x.new_empty(x.shape, dtype=torch.float8_e4m3fn),
            x.new_empty((*x.shape[:-1], K // 128), dtype=torch.float32))


def _blockfp8_quantize_act_cuda(x: Tensor):
    """bf16 x [..., K] -> (e4m3fn codes [..., K], fp32 scales [..., K/128])."""
    torch._check(x.dtype is torch.bfloat16, lambda: "blockfp8 quantize act (HIP) needs bf16 x")
    K = _check_blockfp8_k(x, "x")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    q = torch.empty((M, K), dtype=torch.float8_e4m3fn, device=x.device)
    s = torch.empty((M, K // 128), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("tao_blockfp8_quantize_act_bf16", _ptr(x2), _ptr(q), _ptr(s), M, K, _stream(x))
    return q.reshape(x.shape), s.reshape(*x.shape[:-1], K // 128)


@torch.library.register_fake("torchao::blockfp8_quantize_weight")
def _(w):
    torch._check(w.dim() == 2, lambda: "blockfp8 quantize weight: w must be 2D [N, K]")
    K = _check_blockfp8_k(w, "w")
    return (w.new_empty(w.shape, dtype=torch.float8_e4m3fn),
            w.new_empty(((w.size(0) + 127) // 128, K // 128), dtype=torch.float32))


def _blockfp8_quantize_weight_cuda(w: Tensor):
    """bf16 w [N, K] -> (e4m3fn codes [N, K], fp32 scales [ceil(N/128), K/128])."""
    torch._check(w.dtype is torch.bfloat16, lambda: "blockfp8 quantize weight (HIP) needs bf16 w")
    torch._check(w.dim() == 2, lambda: "blockfp8 quantize weight: w must be 2D [N, K]")
    K = _check_blockfp8_k(w, "w")
    N = w.size(0)
    w2 = w if w.is_contiguous() and w.data_ptr() % 16 == 0 else w.contiguous()
    q = torch.empty((N, K), dtype=torch.float8_e4m3fn, device=w.device)
    s = torch.empty(((N + 127) // 128, K // 128), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("tao_blockfp8_quantize_weight_bf16", _ptr(w2), _ptr(q), _ptr(s), N, K,
                  _stream(w))
    return q, s


@torch.library.register_fake("torchao::blockfp8_dequantize_weight")
def _(wq, w_scale, out_bf16=False):
    _check_blockfp8_weight(wq, w_scale)
    return wq.new_empty(wq.shape, dtype=torch.bfloat16 if out_bf16 else torch.float32)


def _blockfp8_dequantize_weight_cuda(wq, w_scale, out_bf16=False):
    """float(code) * scale in fp32, stored as fp32 or rounded once to bf16."""
    N, K = _check_blockfp8_weight(wq, w_scale)
    _same_device(wq, w_scale=w_scale)
    q, s = wq.contiguous(), w_scale.contiguous()
    out = torch.empty((N, K), dtype=torch.bfloat16 if out_bf16 else torch.float32,
                      device=wq.device)
    with torch.cuda.device(wq.device):
        _lib.call("tao_blockfp8_dequant_weight", _ptr(q), _ptr(s), _ptr(out), N, K,
                  1 if out_bf16 else 0, _stream(wq))
    return out


@torch.library.register_fake("torchao::blockfp8_scaled_mm")
def _(xq, x_scale, wq, w_scale, bias=None):
    N, K = _check_blockfp8_weight(wq, w_scale)
    torch._check(xq.size(-1) == K, lambda: f"x last dim {xq.size(-1)} != K {K}")
    return xq.new_empty(_linear_out_shape(xq, N), dtype=torch.bfloat16)


def _blockfp8_scaled_mm_cuda(xq, x_scale, wq, w_scale, bias=None):
    """y = bf16(sum_b P_b * (xs_b * ws_b) + bias), fp32 up to the one rounding
    (include/torchao_mi355x.h tao_blockfp8_scaled_mm_bf16)."""
    N, K = _check_blockfp8_weight(wq, w_scale)
    torch._check(xq.dim() >= 1 and xq.size(-1) == K,
                 lambda: f"x last dim {xq.size(-1) if xq.dim() else 0} != K {K}")
    _check_blockfp8_act(xq, x_scale)
    _check_blockfp8_bias(bias, N)
    _same_device(xq, x_scale=x_scale, wq=wq, w_scale=w_scale, bias=bias)
    x2 = xq.reshape(-1, K).contiguous()
    M = x2.size(0)
    xs = x_scale.reshape(-1, K // 128).contiguous()
    ws = w_scale.contiguous()
    wq = wq.contiguous()
    if bias is not None:
        bias = bias.contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=xq.device)
    with torch.cuda.device(xq.device):
        _lib.call("tao_blockfp8_scaled_mm_bf16", _ptr(x2), _ptr(xs), _ptr(wq), _ptr(ws),
                  _ptr(bias), _ptr(y), M, N, K, _stream(xq))
    return y.reshape(_linear_out_shape(xq, N))


@torch.library.register_fake("torchao::blockfp8_dyn_linear")
def _(x, wq, w_scale, bias=None):
    N, K = _check_blockfp8_weight(wq, w_scale)
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    return x.new_empty(_linear_out_shape(x, N), dtype=torch.bfloat16)


def _blockfp8_dyn_linear_cuda(x, wq, w_scale, bias=None):
    """The whole linear from a bf16 activation. One token: block quantisation + GEMV in one
    launch. More: blockfp8_quantize_act into buffers of the caching allocator, then
    blockfp8_scaled_mm; bit-identical to calling the two ops."""
    N, K = _check_blockfp8_weight(wq, w_scale)
    torch._check(x.dtype is torch.bfloat16, lambda: "blockfp8_dyn_linear (HIP) needs bf16 x")
    torch._check(x.dim() >= 1 and x.size(-1) == K,
                 lambda: f"x last dim {x.size(-1) if x.dim() else 0} != K {K}")
    _check_blockfp8_bias(bias, N)
    _same_device(x, wq=wq, w_scale=w_scale, bias=bias)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    ws = w_scale.contiguous()
    wq = wq.contiguous()
    if bias is not None:
        bias = bias.contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        if M == 1 and K <= 65536:
            _lib.call("tao_blockfp8_dyn_linear_bf16", _ptr(x2), _ptr(wq), _ptr(ws), _ptr(bias),
                      _ptr(y), 1, N, K, _stream(x))
        elif M > 0:
            q = torch.empty((M, K), dtype=torch.float8_e4m3fn, device=x.device)
            s = torch.empty((M, K // 128), dtype=torch.float32, device=x.device)
            _lib.call("tao_blockfp8_quantize_act_bf16", _ptr(x2), _ptr(q), _ptr(s), M, K,
                      _stream(x))
            _lib.call("tao_blockfp8_scaled_mm_bf16", _ptr(q), _ptr(s), _ptr(wq), _ptr(ws),
                      _ptr(bias), _ptr(y), M, N, K, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


# ---- register device impls ------------------------------------------------------------------
# ---------------------------------------------------------------------------------------------
# W4A8: int8 dynamic activation x packed int4 weight (csrc/w4a8.hip)
# ---------------------------------------------------------------------------------------------
def _check_w4a8_weight(weight, weight_scale):
    torch._check(weight.dim() == 2 and weight.dtype in (torch.int8, torch.uint8),
                 lambda: "weight must be a 2D int8 [N, K/2] tensor of packed int4 codes")
    torch._check(weight_scale.dtype is torch.float32, lambda: "weight_scale must be float32")
    N, K = weight.size(0), weight.size(1) * 2
    torch._check(weight_scale.dim() == 1 and weight_scale.numel() == N,
                 lambda: f"weight_scale must be [N] = ({N}), got {tuple(weight_scale.shape)}")
    torch._check(K % 32 == 0, lambda: f"K ({K}) must be a multiple of 32")
    return N, K


def _check_w4a8_bias(bias, N):
    torch._check(bias is None or (bias.dim() == 1 and bias.numel() == N),
                 lambda: f"bias must be [N] = ({N})")


@torch.library.register_fake("torchao::rowwise_scaled_linear_cutlass_s8s4")
def _(input, input_scale, weight, weight_scale, bias=None, out_dtype=None):
    N, K = _check_w4a8_weight(weight, weight_scale)
    torch._check(input.dtype is torch.int8, lambda: "input must be int8")
    torch._check(input.size(-1) == K, lambda: f"input last dim {input.size(-1)} != K {K}")
    torch._check(out_dtype in (None, torch.bfloat16),
                 lambda: "rowwise_scaled_linear_cutlass_s8s4 (HIP) gives bfloat16 output only")
    return input.new_empty(_linear_out_shape(input, N), dtype=torch.bfloat16)


def _w4a8_scaled_mm_cuda(input, input_scale, weight, weight_scale, bias=None, out_dtype=None):
    """y = bf16(fp32(int32 acc) * input_scale[m] * weight_scale[n] + bias), fp32 up to the one
    rounding (include/torchao_mi355x.h tao_w4a8_scaled_mm_bf16)."""
    N, K = _check_w4a8_weight(weight, weight_scale)
    torch._check(input.dtype is torch.int8, lambda: "input must be int8")
    torch._check(input_scale.dtype is torch.float32, lambda: "input_scale must be float32")
    torch._check(input.size(-1) == K, lambda: f"input last dim {input.size(-1)} != K {K}")
    torch._check(out_dtype in (None, torch.bfloat16),
                 lambda: "rowwise_scaled_linear_cutlass_s8s4 (HIP) gives bfloat16 output only")
    _check_w4a8_bias(bias, N)
    _same_device(input, input_scale=input_scale, weight=weight, weight_scale=weight_scale,
                 bias=bias)
    x2 = input.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    xs = input_scale.reshape(-1).contiguous()
    torch._check(xs.numel() == M, lambda: "input_scale must have one entry per row")
    weight = weight.contiguous()
    ws = weight_scale.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=input.device)
    with torch.cuda.device(input.device):
        _lib.call("tao_w4a8_scaled_mm_bf16", _ptr(x2), _ptr(xs), _ptr(weight), _ptr(ws),
                  _ptr(bias), _ptr(y), M, N, K, _stream(input))
    return y.reshape(_linear_out_shape(input, N))


@torch.library.register_fake("torchao::int8_quantize_per_token_f32")
def _(x):
    torch._check(x.size(-1) % 8 == 0, lambda: f"K ({x.size(-1)}) must be a multiple of 8")
    return (x.new_empty(x.shape, dtype=torch.int8),
            x.new_empty(x.shape[:-1], dtype=torch.float32))


def _int8_quant_f32_cuda(x: Tensor):
    """bf16 x [..., K] -> (int8 [..., K], per-token scale fp32 [...]): _int8_symm_cutlass_quant."""
    torch._check(x.dtype is torch.bfloat16,
                 lambda: "int8_quantize_per_token_f32 (HIP) needs bf16 x")
    K = x.size(-1)
    torch._check(K % 8 == 0, lambda: f"K ({K}) must be a multiple of 8")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    q = torch.empty((M, K), dtype=torch.int8, device=x.device)
    s = torch.empty((M,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("tao_int8_quant_per_token_f32", _ptr(x2), _ptr(q), _ptr(s), M, K, _stream(x))
    return q.reshape(x.shape), s.reshape(x.shape[:-1])


@torch.library.register_fake("torchao::int4_quantize_rows_packed")
def _(w):
    torch._check(w.dim() == 2, lambda: "int4_quantize_rows_packed: w must be [N, K]")
    torch._check(w.size(1) % 8 == 0, lambda: f"K ({w.size(1)}) must be a multiple of 8")
    return (w.new_empty((w.size(0), w.size(1) // 2), dtype=torch.int8),
            w.new_empty((w.size(0),), dtype=torch.float32))


def _int4_quantize_rows_packed_cuda(w: Tensor):
    """bf16 W [N, K] -> (int8 [N, K/2] packed int4 codes, per-row scale fp32 [N]):
    _int4_symm_cutlass_quant and CutlassInt4PackedLayout's from_plain in one pass."""
    torch._check(w.dtype is torch.bfloat16,
                 lambda: "int4_quantize_rows_packed (HIP) needs a bf16 weight")
    torch._check(w.dim() == 2, lambda: "int4_quantize_rows_packed: w must be [N, K]")
    R, K = w.shape
    torch._check(K % 8 == 0, lambda: f"K ({K}) must be a multiple of 8")
    if not w.is_contiguous() or w.data_ptr() % 16:
        w = w.contiguous()
    q = torch.empty((R, K // 2), dtype=torch.int8, device=w.device)
    s = torch.empty((R,), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("tao_int4_quantize_rows_packed_bf16", _ptr(w), _ptr(q), _ptr(s), R, K,
                  _stream(w))
    return q, s


@torch.library.register_fake("torchao::w4a8_dyn_linear")
def _(x, weight, weight_scale, bias=None):
    N, K = _check_w4a8_weight(weight, weight_scale)
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    return x.new_empty(_linear_out_shape(x, N), dtype=torch.bfloat16)


def _w4a8_dyn_linear_cuda(x, weight, weight_scale, bias=None):
    """The whole linear from a bf16 activation. One token: quantisation + GEMV in one launch.
    More: int8_quantize_per_token_f32 into a buffer of the caching allocator, then the scaled mm;
    bit-identical to calling the two ops."""
    N, K = _check_w4a8_weight(weight, weight_scale)
    torch._check(x.dtype is torch.bfloat16, lambda: "w4a8_dyn_linear (HIP) needs bf16 x")
    torch._check(x.size(-1) == K, lambda: f"x last dim {x.size(-1)} != K {K}")
    _check_w4a8_bias(bias, N)
    _same_device(x, weight=weight, weight_scale=weight_scale, bias=bias)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.size(0)
    weight = weight.contiguous()
    ws = weight_scale.contiguous()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        if M == 1 and K <= 65536:
            _lib.call("tao_w4a8_dyn_linear_bf16", _ptr(x2), _ptr(weight), _ptr(ws), _ptr(bias),
                      _ptr(y), 1, N, K, _stream(x))
        elif M > 0:
            q = torch.empty((M, K), dtype=torch.int8, device=x.device)
            s = torch.empty((M,), dtype=torch.float32, device=x.device)
            _lib.call("tao_int8_quant_per_token_f32", _ptr(x2), _ptr(q), _ptr(s), M, K,
                      _stream(x))
            _lib.call("tao_w4a8_scaled_mm_bf16", _ptr(q), _ptr(s), _ptr(weight), _ptr(ws),
                      _ptr(bias), _ptr(y), M, N, K, _stream(x))
    return y.reshape(_linear_out_shape(x, N))


# ---------------------------------------------------------------------------------------------
# NF4 (csrc/nf4.hip): fake kernels only; the CUDA kernels are C++ (csrc/torch_ops.cpp)
# ---------------------------------------------------------------------------------------------
def _check_nf4_parts(codes, qscalers, qfactor, mean, levels, numel, op):
    torch._check(codes.dtype is torch.uint8, lambda: f"{op}: codes must be uint8")
    torch._check(qscalers.dtype is torch.int8, lambda: f"{op}: qscalers must be int8")
    torch._check(numel % 64 == 0,
                 lambda: f"{op}: numel ({numel}) must be a multiple of the block size 64")
    torch._check(codes.numel() == numel // 2,
                 lambda: f"{op}: codes must have numel / 2 = {numel // 2} bytes")
    torch._check(qscalers.numel() == numel // 64,
                 lambda: f"{op}: qscalers must have numel / 64 = {numel // 64} elements")
    torch._check(qfactor.numel() == (numel + 16383) // 16384,
                 lambda: f"{op}: qfactor must have ceil(numel / 16384) elements")
    torch._check(mean.numel() == 1 and levels.numel() == 16,
                 lambda: f"{op}: mean must have one element and levels 16")


@torch.library.register_fake("torchao::nf4_quantize_blocks")
def _(w, levels):
    torch._check(w.numel() % 64 == 0,
                 lambda: f"nf4_quantize_blocks: numel ({w.numel()}) must be a multiple of 64")
    return (w.new_empty((w.numel() // 2,), dtype=torch.uint8),
            w.new_empty((w.numel() // 64,), dtype=torch.bfloat16))


@torch.library.register_fake("torchao::nf4_dequantize")
def _(codes, qscalers, qfactor, mean, levels, shape):
    numel = 1
    for d in shape:
        numel *= d
    _check_nf4_parts(codes, qscalers, qfactor, mean, levels, numel, "nf4_dequantize")
    return codes.new_empty(tuple(shape), dtype=torch.bfloat16)


@torch.library.register_fake("torchao::nf4_linear")
def _(x, codes, qscalers, qfactor, mean, levels, N, bias=None):
    K = x.shape[-1]
    torch._check(K % 64 == 0, lambda: f"nf4_linear: K ({K}) must be a multiple of 64")
    _check_nf4_parts(codes, qscalers, qfactor, mean, levels, N * K, "nf4_linear")
    return x.new_empty((*x.shape[:-1], N), dtype=torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# FP6 (csrc/fp6.hip): fake kernels only; the CUDA kernels are C++ (csrc/torch_ops.cpp)
# ---------------------------------------------------------------------------------------------
def _check_fp6_format(ebits, mbits, op):
    torch._check((ebits, mbits) in ((3, 2), (2, 3)),
                 lambda: f"{op}: (ebits, mbits) = ({ebits}, {mbits}) is not served; served: "
                         f"(3, 2) and (2, 3)")


def _check_fp6_weight(codes, scale, op):
    torch._check(codes.dtype is torch.int32 and codes.dim() == 2,
                 lambda: f"{op}: codes must be a 2D int32 [N, K * 6 / 32] tensor")
    torch._check(codes.shape[1] % 6 == 0,
                 lambda: f"{op}: codes must hold whole 32-code groups of 6 dwords, got "
                         f"{codes.shape[1]} dwords per row")
    torch._check(scale.numel() == codes.shape[0],
                 lambda: f"{op}: scale must have N = {codes.shape[0]} elements")


@torch.library.register_fake("torchao::fp6_quantize_rows")
def _(w, ebits, mbits):
    _check_fp6_format(ebits, mbits, "fp6_quantize_rows")
    torch._check(w.dim() == 2 and w.shape[1] % 32 == 0,
                 lambda: "fp6_quantize_rows: w must be 2D with K a multiple of 32")
    return (w.new_empty((w.shape[0], w.shape[1] // 32 * 6), dtype=torch.int32),
            w.new_empty((w.shape[0],), dtype=torch.bfloat16))


@torch.library.register_fake("torchao::fp6_dequantize")
def _(codes, scale, ebits, mbits):
    _check_fp6_format(ebits, mbits, "fp6_dequantize")
    _check_fp6_weight(codes, scale, "fp6_dequantize")
    return codes.new_empty((codes.shape[0], codes.shape[1] // 6 * 32), dtype=torch.bfloat16)


@torch.library.register_fake("torchao::fp6_weight_only_linear")
def _(x, codes, scale, ebits, mbits, bias=None):
    _check_fp6_format(ebits, mbits, "fp6_weight_only_linear")
    _check_fp6_weight(codes, scale, "fp6_weight_only_linear")
    K = codes.shape[1] // 6 * 32
    torch._check(K % 64 == 0,
                 lambda: f"fp6_weight_only_linear: K ({K}) must be a multiple of 64")
    torch._check(x.shape[-1] == K, lambda: f"x last dim {x.shape[-1]} != K {K}")
    return x.new_empty((*x.shape[:-1], codes.shape[0]), dtype=torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# MoE (csrc/moe_gemm.hip): fake kernels only; the CUDA kernels are C++ (csrc/torch_ops.cpp)
# ---------------------------------------------------------------------------------------------
MOE_MAX_EXPERTS = 256
MOE_MAX_TOP_K = 8


@torch.library.register_fake("torchao::moe_route")
def _(expert_indices, num_experts, top_k):
    torch._check(1 <= num_experts <= MOE_MAX_EXPERTS,
                 lambda: f"moe_route: num_experts ({num_experts}) is not served; served: 1 to "
                         f"{MOE_MAX_EXPERTS}")
    torch._check(1 <= top_k <= MOE_MAX_TOP_K,
                 lambda: f"moe_route: top_k ({top_k}) is not served; served: 1 to {MOE_MAX_TOP_K}")
    R = expert_indices.numel()
    return (expert_indices.new_empty((num_experts + 1,), dtype=torch.int32),
            expert_indices.new_empty((R,), dtype=torch.int32),
            expert_indices.new_empty((R,), dtype=torch.int32))


@torch.library.register_fake("torchao::int4_grouped_linear")
def _(x, src_row, row_div, packed, scales_and_zeros, packed_b, scales_and_zeros_b, offsets,
      group_size):
    torch._check(group_size in _GROUP_SIZES, lambda: "qGroupSize must be 32, 64, 128, or 256")
    torch._check(packed.dim() == 3 and packed.dtype is torch.int32,
                 lambda: "int4_grouped_linear: packed must be a 3D int32 [E, N, K/8] tensor")
    torch._check(x.dim() == 2 and x.shape[1] == packed.shape[2] * 8,
                 lambda: f"x last dim {x.shape[-1]} != K {packed.shape[2] * 8}")
    R = x.shape[0] if src_row is None else src_row.numel()
    return x.new_empty((R, packed.shape[1]), dtype=torch.bfloat16)


@torch.library.register_fake("torchao::moe_combine")
def _(y2, expert_weights, inverse, top_k):
    torch._check(1 <= top_k <= MOE_MAX_TOP_K,
                 lambda: f"moe_combine: top_k ({top_k}) is not served; served: 1 to {MOE_MAX_TOP_K}")
    torch._check(y2.dim() == 2, lambda: "moe_combine: y2 must be 2D")
    return y2.new_empty((y2.shape[0] // top_k, y2.shape[1]))


# The per-linear ops take their CUDA kernels from libtorchao_ops.so (csrc/torch_ops.cpp: the
# same checks, then the C-ABI, with no Python frame: ~19 -> ~7 µs of host time per call at
# M = 1, profiles/r2_eager_overhead*.json). The Python impls below serve the rest, and these
# too when that library cannot load or an experiment points TORCHAO_MI355X_LIB at a variant
# build (the C++ kernels are linked to the in-tree library).
_OPS_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libtorchao_ops.so")
_native_served: frozenset = frozenset()
_native_served_float8: frozenset = frozenset()
_native_served_float8_dyn: frozenset = frozenset()
_native_served_mx: frozenset = frozenset()
_native_served_mxfp4: frozenset = frozenset()
_native_served_blockfp8: frozenset = frozenset()
_native_served_awq: frozenset = frozenset()
_native_served_smoothquant: frozenset = frozenset()
_native_served_w4a8: frozenset = frozenset()
_native_served_nf4: frozenset = frozenset()
_native_served_fp6: frozenset = frozenset()
_native_served_moe: frozenset = frozenset()
_native_error: Optional[str] = None
if os.environ.get("TORCHAO_MI355X_LIB"):
    _native_error = "TORCHAO_MI355X_LIB is set (variant build): Python impls"
else:
    try:
        torch.ops.load_library(_OPS_LIB)
        _ops_dll = ctypes.CDLL(_OPS_LIB)
        _served = _ops_dll.tao_torch_ops_served
        _served.restype = ctypes.c_char_p
        _native_served = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_float8
        _served.restype = ctypes.c_char_p
        _native_served_float8 = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_float8_dyn
        _served.restype = ctypes.c_char_p
        _native_served_float8_dyn = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_mx
        _served.restype = ctypes.c_char_p
        _native_served_mx = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_mxfp4
        _served.restype = ctypes.c_char_p
        _native_served_mxfp4 = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_blockfp8
        _served.restype = ctypes.c_char_p
        _native_served_blockfp8 = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_awq
        _served.restype = ctypes.c_char_p
        _native_served_awq = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_smoothquant
        _served.restype = ctypes.c_char_p
        _native_served_smoothquant = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_w4a8
        _served.restype = ctypes.c_char_p
        _native_served_w4a8 = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_nf4
        _served.restype = ctypes.c_char_p
        _native_served_nf4 = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_fp6
        _served.restype = ctypes.c_char_p
        _native_served_fp6 = frozenset(_served().decode().split(","))
        _served = _ops_dll.tao_torch_ops_served_moe
        _served.restype = ctypes.c_char_p
        _native_served_moe = frozenset(_served().decode().split(","))
    except (OSError, RuntimeError, AttributeError) as e:
        _native_error = f"{type(e).__name__}: {e}"


def native_dispatch() -> frozenset:
    """The integer per-linear ``torch.ops.torchao`` ops whose CUDA kernel is C++
    (libtorchao_ops.so); the float8 weight-only set is ``native_dispatch_float8()``."""
    return _native_served


def native_dispatch_float8() -> frozenset:
    """The float8 weight-only ops whose CUDA kernel is C++ (libtorchao_ops.so)."""
    return _native_served_float8


def native_dispatch_float8_dyn() -> frozenset:
    """The float8 dynamic-activation ops whose CUDA kernel is C++ (libtorchao_ops.so)."""
    return _native_served_float8_dyn


def native_dispatch_mx() -> frozenset:
    """The MXFP8 ops whose CUDA kernel is C++ (libtorchao_ops.so)."""
    return _native_served_mx


def native_dispatch_mxfp4() -> frozenset:
    """The MXFP4-weight ops whose CUDA kernel is C++ (libtorchao_ops.so)."""
    return _native_served_mxfp4


def native_dispatch_blockfp8() -> frozenset:
    """The blockwise float8 ops whose CUDA kernel is C++ (libtorchao_ops.so)."""
    return _native_served_blockfp8


def native_dispatch_awq() -> frozenset:
    """The activation pre-scale (AWQ) ops whose CUDA kernel is C++ (libtorchao_ops.so)."""
    return _native_served_awq


def native_dispatch_smoothquant() -> frozenset:
    """The SmoothQuant ops whose CUDA kernel is C++ (libtorchao_ops.so)."""
    return _native_served_smoothquant


def native_dispatch_nf4() -> frozenset:
    """The NF4 ops (they have C++ CUDA kernels only; empty when libtorchao_ops.so did not load)."""
    return _native_served_nf4


def native_dispatch_fp6() -> frozenset:
    """The FP6 ops (they have C++ CUDA kernels only; empty when libtorchao_ops.so did not load)."""
    return _native_served_fp6


def native_dispatch_moe() -> frozenset:
    """The MoE ops (they have C++ CUDA kernels only; empty when libtorchao_ops.so did not load)."""
    return _native_served_moe


def native_dispatch_w4a8() -> frozenset:
    """The W4A8 ops whose CUDA kernel is C++ (libtorchao_ops.so)."""
    return _native_served_w4a8


for _name, _fn in [
    ("unpack_tensor_core_tiled_layout", _unpack_tile_cuda),
    ("dequantize_tensor_core_tiled_layout", _dequant_tile_cuda),
    ("pack_tensor_core_tiled_layout", _pack_tile_cuda),
    ("int4_pack", _int4_pack_cuda),
    ("int4_pack_u8", _int4_pack_u8_cuda),
    ("int4_unpack", _int4_unpack_cuda),
    ("int4_dequantize", _int4_dequant_cuda),
    ("int4_weight_only_linear", _int4_linear_cuda),
    ("int8_weight_only_linear", _int8wo_linear_cuda),
    ("int8_quantize_per_token", _int8_quant_cuda),
    ("int4_quantize_pack", _int4_quantize_pack_cuda),
    ("int8_quantize_rows", _int8_quantize_rows_cuda),
    ("int8_scaled_mm", _int8_scaled_mm_cuda),
    ("int8_dyn_linear", _int8_dyn_linear_cuda),
]:
    if _name not in _native_served:
        lib.impl(_name, _fn, "CUDA")
for _name, _fn in [
    ("fp8_weight_only_linear", _fp8wo_linear_cuda),
    ("fp8_quantize_rows", _fp8_quantize_rows_cuda),
    ("fp8_dequantize", _fp8_dequantize_cuda),
]:
    if _name not in _native_served_float8:
        lib_float8.impl(_name, _fn, "CUDA")
for _name, _fn in [
    ("fp8_scaled_mm", _fp8_scaled_mm_cuda),
    ("fp8_dyn_linear", _fp8_dyn_linear_cuda),
]:
    if _name not in _native_served_float8_dyn:
        lib_float8_dyn.impl(_name, _fn, "CUDA")
for _name, _fn in [
    ("mx_quantize_rows", _mx_quantize_rows_cuda),
    ("mx_scaled_mm", _mx_scaled_mm_cuda),
    ("mx_dyn_linear", _mx_dyn_linear_cuda),
]:
    if _name not in _native_served_mx:
        lib_mx.impl(_name, _fn, "CUDA")
for _name, _fn in [
    ("mxfp4_quantize_rows", _mxfp4_quantize_rows_cuda),
    ("mxfp4w_scaled_mm", _mxfp4w_scaled_mm_cuda),
    ("mxfp4w_dyn_linear", _mxfp4w_dyn_linear_cuda),
]:
    if _name not in _native_served_mxfp4:
        lib_mxfp4.impl(_name, _fn, "CUDA")
for _name, _fn in [
    ("blockfp8_quantize_act", _blockfp8_quantize_act_cuda),
    ("blockfp8_quantize_weight", _blockfp8_quantize_weight_cuda),
    ("blockfp8_dequantize_weight", _blockfp8_dequantize_weight_cuda),
    ("blockfp8_scaled_mm", _blockfp8_scaled_mm_cuda),
    ("blockfp8_dyn_linear", _blockfp8_dyn_linear_cuda),
]:
    if _name not in _native_served_blockfp8:
        lib_blockfp8.impl(_name, _fn, "CUDA")
for _name, _fn in [
    ("act_prescale", _act_prescale_cuda),
    ("int4_prescaled_linear", _int4_prescaled_linear_cuda),
]:
    if _name not in _native_served_awq:
        lib_awq.impl(_name, _fn, "CUDA")
for _name, _fn in [
    ("int8_smooth_quantize_per_token", _int8_smooth_quant_per_token_cuda),
    ("int8_smooth_quantize_static", _int8_smooth_quant_static_cuda),
    ("int8_smooth_dyn_linear", _int8_smooth_dyn_linear_cuda),
    ("int8_smooth_static_linear", _int8_smooth_static_linear_cuda),
]:
    if _name not in _native_served_smoothquant:
        lib_smoothquant.impl(_name, _fn, "CUDA")
for _name, _fn in [
    ("rowwise_scaled_linear_cutlass_s8s4", _w4a8_scaled_mm_cuda),
    ("int8_quantize_per_token_f32", _int8_quant_f32_cuda),
    ("int4_quantize_rows_packed", _int4_quantize_rows_packed_cuda),
    ("w4a8_dyn_linear", _w4a8_dyn_linear_cuda),
]:
    if _name not in _native_served_w4a8:
        lib_w4a8.impl(_name, _fn, "CUDA")
lib_hqq.impl("int4_hqq_quantize_pack", _int4_hqq_quantize_pack_cuda, "CUDA")
# Host packers (C++ in the same library) so quantize_ works on CPU-resident models.
lib.impl("int4_pack", _int4_pack_cpu, "CPU")
lib.impl("int4_unpack", _int4_unpack_cpu, "CPU")
lib.impl("unpack_tensor_core_tiled_layout", _unpack_tile_cpu, "CPU")


# ---- Python-level wrappers with the reference names (ops.py:255-377) ------------------------
def unpack_tensor_core_tiled_layout(packed_w: Tensor, inner_k_tiles: int,
                                    tile_format=-1) -> Tensor:
    """Tile-format int4 weight [N/8][K/(ikt*16)][32][ikt/2] -> int32 [N, K]."""
    return torch.ops.torchao.unpack_tensor_core_tiled_layout.default(
        packed_w, inner_k_tiles, _tile_format(tile_format))


def dequantize_tensor_core_tiled_layout(
    packed_w: Tensor, scales_and_zeros: Tensor, group_size: int, inner_k_tiles: int,
    tile_format=-1,
) -> Tensor:
    """Tile-format int4 weight + [K/g, N, 2] scales/zeros -> bf16 [N, K]."""
    return torch.ops.torchao.dequantize_tensor_core_tiled_layout.default(
        packed_w, scales_and_zeros, group_size, inner_k_tiles, _tile_format(tile_format)
    )


def pack_tensor_core_tiled_layout(int_data: Tensor, inner_k_tiles: int,
                                  tile_format=-1) -> Tensor:
    """int32 [N, K] -> the tile format (tile_format 1 == PyTorch-ROCm's
    aten._convert_weight_to_int4pack of the same nibbles, bit for bit)."""
    return torch.ops.torchao.pack_tensor_core_tiled_layout.default(
        int_data, inner_k_tiles, _tile_format(tile_format))


def rowwise_scaled_linear_cutlass_s8s4(
    input: Tensor,
    input_scale: Tensor,
    weight: Tensor,
    weight_scale: Tensor,
    bias: Optional[Tensor] = None,
    out_dtype: Optional[torch.dtype] = None,
) -> Tensor:
    """The reference's wrapper (torchao/ops.py:666-695): int8 ``input`` [..., K] with per-row fp32
    ``input_scale`` [...], int4 ``weight`` packed two per byte in int8 [N, K/2] with per-row fp32
    ``weight_scale`` [N]; bf16 output. Served by the gfx950 kernels of csrc/w4a8.hip."""
    return torch.ops.torchao.rowwise_scaled_linear_cutlass_s8s4.default(
        input, input_scale, weight, weight_scale, bias, out_dtype)


def int4_weight_only_linear(x, packed_w, scales_and_zeros, group_size, bias=None):
    return torch.ops.torchao.int4_weight_only_linear.default(
        x, packed_w, scales_and_zeros, group_size, bias
    )
