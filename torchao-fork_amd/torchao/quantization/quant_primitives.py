"""Affine quantization primitives for the weight-only / dynamic int8 linear path.

Restates the subset of the reference ``torchao/quantization/quant_primitives.py`` the hot path
uses, with identical names, arguments and floating-point op order (results are pinned
bit-for-bit against fixtures generated from the reference, tests/golden/):

  * ``choose_qparams_affine``            (reference :1497-1577, SYMMETRIC / ASYMMETRIC)
  * ``_choose_qparams_affine_tinygemm``  (:1238-1307; scale/zero in the input dtype)
  * ``quantize_affine``                  (:398-459; ``clamp(round(x * (1/s)) + zp)``)
  * ``_quantize_affine_tinygemm``        (:461-573; ``clamp(round((x - (z - s*mid)) / s))``)
  * ``_quantize_affine_no_zero_point``   (:600-690)
  * ``dequantize_affine`` / ``_dequantize_affine_tinygemm`` / ``_dequantize_affine_no_zero_point``
    (:779-1031)
  * ``_choose_scale_float8`` / ``_quantize_affine_float8`` / ``_dequantize_affine_float8`` /
    ``_expand_scale_to_tensor_shape``    (:2175-2312; float8 e4m3fn, fp32 scales)
  * ``_choose_qparams_affine_floatx`` / ``_quantize_affine_floatx`` /
    ``_dequantize_affine_floatx``        (:2114-2171; FP6 e3m2 / e2m3, one bf16 scale per row;
    written here from the formats' definition, pinned against the reference by fixtures)
  * ``_choose_qparams_and_quantize_affine_hqq`` / ``optimize_weights_proximal_legacy`` /
    ``_shrink_lp_op`` / ``_convert_to_affinequantized_format``  (:1901-2111; HQQ, in fp32 on
    every device: the reference's CPU arithmetic)

These run with torch ops on whatever device the weight lives on: they execute once at
quantization time, outside the per-token hot loop (which is the HIP kernels behind torchao.ops).
"""

import functools
import math
from enum import Enum, auto
from typing import Callable, List, Optional, Tuple, Union

import torch

__all__ = [
    "MappingType",
    "ZeroPointDomain",
    "choose_qparams_affine",
    "choose_qparams_affine_with_min_max",
    "quantize_affine",
    "dequantize_affine",
    "_choose_qparams_affine_tinygemm",
    "_choose_qparams_affine_dont_preserve_zero",
    "_quantize_affine_tinygemm",
    "_dequantize_affine_tinygemm",
    "_quantize_affine_no_zero_point",
    "_dequantize_affine_no_zero_point",
    "_get_reduction_params",
    "FP8_TYPES",
    "_choose_scale_float8",
    "_quantize_affine_float8",
    "_dequantize_affine_float8",
    "_expand_scale_to_tensor_shape",
    "FLOATX_SERVED",
    "_floatx_max_normal",
    "_floatx_code_values",
    "_choose_qparams_affine_floatx",
    "_quantize_affine_floatx",
    "_dequantize_affine_floatx",
    "_shrink_lp_op",
    "optimize_weights_proximal_legacy",
    "_convert_to_affinequantized_format",
    "_choose_qparams_and_quantize_affine_hqq",
    "HQQ_OPT_PARAMS",
]


class MappingType(Enum):
    """How float values map onto the integer grid (reference quant_primitives.py:61-80)."""

    SYMMETRIC = auto()
    SYMMETRIC_NO_CLIPPING_ERR = auto()
    ASYMMETRIC = auto()


class ZeroPointDomain(Enum):
    """Where the zero point lives: integer grid, float domain (tinygemm), or absent."""

    INT = auto()
    FLOAT = auto()
    NONE = auto()


_DTYPE_TO_QVALUE_BOUNDS = {
    torch.uint8: (0, 255),
    torch.int8: (-128, 127),
    torch.int16: (-(2**15), 2**15 - 1),
    torch.int32: (-(2**31), 2**31 - 1),
}
for _bits in range(1, 8):
    _u = getattr(torch, f"uint{_bits}", None)
    _s = getattr(torch, f"int{_bits}", None)
    if _u is not None:
        _DTYPE_TO_QVALUE_BOUNDS[_u] = (0, 2**_bits - 1)
    if _s is not None:
        _DTYPE_TO_QVALUE_BOUNDS[_s] = (-(2 ** (_bits - 1)), 2 ** (_bits - 1) - 1)


def _get_and_check_qmin_qmax(dtype, quant_min, quant_max):
    if dtype not in _DTYPE_TO_QVALUE_BOUNDS:
        raise ValueError(f"Unsupported dtype: {dtype}")
    lo, hi = _DTYPE_TO_QVALUE_BOUNDS[dtype]
    quant_min = lo if quant_min is None else quant_min
    quant_max = hi if quant_max is None else quant_max
    assert quant_min >= lo, f"quant_min out of bound for dtype, lower bound {lo}: {quant_min}"
    assert quant_max <= hi, f"quant_max out of bound for dtype, upper bound {hi}: {quant_max}"
    return quant_min, quant_max


def _get_reduction_params(block_size, input_size):
    """Shape that exposes every quantization block as its own axis, and the block axes.

    block (1, 32) on a [4, 64] tensor -> view [4, 2, 32], reduce over [2].
    """
    assert len(block_size) == len(input_size)
    view: List[int] = []
    red: List[int] = []
    for b, s in zip(block_size, input_size):
        if b != s and b > 1:
            assert s % b == 0, f"Expecting input size {s} to be divisible by block_size {b}"
            view += [s // b, b]
            red.append(len(view) - 1)
        else:
            view.append(s)
            if b != 1:
                red.append(len(view) - 1)
    return view, red


def _qparam_view(t: torch.Tensor, block_size, input_shape):
    """Broadcastable view of per-block qparams against the reduction view of the input."""
    view, red = _get_reduction_params(block_size, input_shape)
    shape = list(view)
    for d in red:
        shape[d] = 1
    return view, t.view(shape)


class _Round(torch.autograd.Function):
    """round-half-to-even with a straight-through gradient."""

    @staticmethod
    def forward(ctx, x):
        return torch.round(x)

    @staticmethod
    def backward(ctx, gy):
        return gy


# ---------------------------------------------------------------------------------------------
# choose_qparams
# ---------------------------------------------------------------------------------------------
def _block_min_max(input: torch.Tensor, block_size):
    view, red = _get_reduction_params(block_size, input.size())
    x = input.view(view)
    return torch.amin(x, dim=red, keepdim=False), torch.amax(x, dim=red, keepdim=False)


@torch.no_grad()
def choose_qparams_affine(
    input: torch.Tensor,
    mapping_type: MappingType,
    block_size: Tuple[int, ...],
    target_dtype: torch.dtype,
    quant_min: Optional[Union[int, float]] = None,
    quant_max: Optional[Union[int, float]] = None,
    eps: Optional[float] = None,
    scale_dtype: Optional[torch.dtype] = None,
    zero_point_dtype: Optional[torch.dtype] = torch.int32,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-block scale / zero point preserving zero (integer zero-point domain)."""
    quant_min, quant_max = _get_and_check_qmin_qmax(target_dtype, quant_min, quant_max)
    scale_dtype = input.dtype if scale_dtype is None else scale_dtype
    eps = torch.finfo(input.dtype).eps if eps is None else eps
    assert len(block_size) == input.dim(), f"Got input dim:{input.dim()}, block_size: {block_size}"
    mn, mx = _block_min_max(input, block_size)
    mn_neg = torch.min(mn, torch.zeros_like(mn))
    mx_pos = torch.max(mx, torch.zeros_like(mx))
    if mapping_type in (MappingType.SYMMETRIC, MappingType.SYMMETRIC_NO_CLIPPING_ERR):
        if mapping_type is MappingType.SYMMETRIC:
            amax = torch.max(-mn_neg, mx_pos)
            scale = amax / (float(quant_max - quant_min) / 2)
        else:
            smin = mn_neg / float(quant_min)
            smax = mx_pos / float(quant_max)
            scale = torch.where(smin > smax, smin, smax)
        zero_point = torch.full_like(scale, int((quant_max + quant_min + 1) / 2))
        scale = torch.clamp(scale, min=eps)
    elif mapping_type is MappingType.ASYMMETRIC:
        scale = (mx_pos - mn_neg) / float(quant_max - quant_min)
        scale = torch.clamp(scale, min=eps)
        zero_point = torch.clamp(quant_min - _Round.apply(mn_neg / scale), quant_min, quant_max)
        if zero_point_dtype is None:
            zero_point_dtype = torch.int32
    else:
        raise ValueError(f"Unsupported mapping type: {mapping_type}")
    if zero_point_dtype is not None:
        zero_point = zero_point.to(dtype=zero_point_dtype)
    return scale.to(dtype=scale_dtype, device=input.device), zero_point


@torch.no_grad()
def choose_qparams_affine_with_min_max(
    min_val: torch.Tensor,
    max_val: torch.Tensor,
    mapping_type: MappingType,
    block_size: Tuple[int, ...],
    target_dtype: torch.dtype,
    quant_min: Optional[int] = None,
    quant_max: Optional[int] = None,
    eps: Optional[float] = None,
    scale_dtype: Optional[torch.dtype] = None,
    zero_point_dtype: Optional[torch.dtype] = None,
    preserve_zero: bool = True,
    zero_point_domain: ZeroPointDomain = ZeroPointDomain.INT,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``choose_qparams_affine`` from already reduced per-block ``min_val`` / ``max_val`` (the
    observers of torchao.quantization.observer; reference quant_primitives.py:1378-1494).
    ``block_size`` is unused, as in the reference. Served: zero-preserving qparams in the integer
    or the zero-point-free domain; dtypes and eps default to those of ``min_val``."""
    if zero_point_domain is None:
        raise ValueError("Please use ZeroPointDomain.NONE instead of None")
    if not preserve_zero or zero_point_domain is ZeroPointDomain.FLOAT:
        raise NotImplementedError(
            "choose_qparams_affine_with_min_max serves preserve_zero=True with "
            "ZeroPointDomain.INT or ZeroPointDomain.NONE")
    quant_min, quant_max = _get_and_check_qmin_qmax(target_dtype, quant_min, quant_max)
    assert min_val is not None and max_val is not None, "min_val and max_val are required"
    assert min_val.dtype == max_val.dtype, (
        f"min_val and max_val must share a dtype, got {min_val.dtype}, {max_val.dtype}")
    scale_dtype = min_val.dtype if scale_dtype is None else scale_dtype
    eps = torch.finfo(min_val.dtype).eps if eps is None else eps
    mn_neg = torch.min(min_val, torch.zeros_like(min_val))
    mx_pos = torch.max(max_val, torch.zeros_like(max_val))
    if mapping_type in (MappingType.SYMMETRIC, MappingType.SYMMETRIC_NO_CLIPPING_ERR):
        if mapping_type is MappingType.SYMMETRIC:
            scale = torch.max(-mn_neg, mx_pos) / (float(quant_max - quant_min) / 2)
        else:
            smin = mn_neg / float(quant_min)
            smax = mx_pos / float(quant_max)
            scale = torch.where(smin > smax, smin, smax)
        zero_point = None
        if zero_point_domain is not ZeroPointDomain.NONE:
            zero_point = torch.full_like(scale, int((quant_max + quant_min + 1) / 2))
        scale = torch.clamp(scale, min=eps)
    elif mapping_type is MappingType.ASYMMETRIC:
        scale = (mx_pos - mn_neg) / torch.tensor(
            float(quant_max - quant_min), dtype=scale_dtype, device=min_val.device)
        scale = torch.clamp(scale, min=eps)
        zero_point = None
        if zero_point_domain is not ZeroPointDomain.NONE:
            zero_point = torch.clamp(quant_min - _Round.apply(mn_neg / scale), quant_min, quant_max)
            zero_point_dtype = torch.int32 if zero_point_dtype is None else zero_point_dtype
    else:
        raise ValueError(f"Unsupported mapping type: {mapping_type}")
    if zero_point is not None:
        zero_point = zero_point.to(dtype=zero_point_dtype)
    return scale.to(dtype=scale_dtype, device=min_val.device), zero_point


@torch.no_grad()
def _choose_qparams_affine_tinygemm(
    input: torch.Tensor,
    mapping_type: MappingType,
    block_size: Tuple[int, ...],
    target_dtype: torch.dtype,
    quant_min: Optional[Union[int, float]] = None,
    quant_max: Optional[Union[int, float]] = None,
    eps: Optional[float] = None,
    scale_dtype: Optional[torch.dtype] = None,
    zero_point_dtype: Optional[torch.dtype] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """tinygemm qparams: s = clamp((max - min) / (qmax - qmin), eps), z = min + s * mid,
    both computed in the input dtype (bf16 for Int4WeightOnlyConfig)."""
    quant_min, quant_max = _get_and_check_qmin_qmax(target_dtype, quant_min, quant_max)
    assert mapping_type is MappingType.ASYMMETRIC, f"Unsupported mapping type: {mapping_type}"
    scale_dtype = input.dtype if scale_dtype is None else scale_dtype
    eps = torch.finfo(input.dtype).eps if eps is None else eps
    assert len(block_size) == input.dim(), f"Got input dim:{input.dim()}, block_size: {block_size}"
    mn, mx = _block_min_max(input, block_size)
    scale = torch.clamp((mx - mn) / float(quant_max - quant_min), min=eps)
    mid = (quant_max + quant_min + 1) / 2
    zero_point = mn + scale * mid
    zero_point_dtype = input.dtype if zero_point_dtype is None else zero_point_dtype
    return scale.to(dtype=scale_dtype, device=input.device), zero_point.to(zero_point_dtype)


@torch.no_grad()
def _choose_qparams_affine_dont_preserve_zero(
    input: torch.Tensor,
    mapping_type: MappingType,
    block_size: Tuple[int, ...],
    target_dtype: torch.dtype,
    quant_min: Optional[Union[int, float]] = None,
    quant_max: Optional[Union[int, float]] = None,
    eps: Optional[float] = None,
    scale_dtype: Optional[torch.dtype] = None,
    zero_point_dtype: Optional[torch.dtype] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Integer zero-point domain WITHOUT zero preservation (quant_primitives.py:1310-1373): the
    block's own [min, max] (not widened to include 0) maps to [qmin, qmax]; s = clamp((max - min)
    / (qmax - qmin), eps), z = clamp(qmin - round(min / s), qmin, qmax) as an integer."""
    quant_min, quant_max = _get_and_check_qmin_qmax(target_dtype, quant_min, quant_max)
    assert mapping_type is MappingType.ASYMMETRIC, f"Unsupported mapping type: {mapping_type}"
    scale_dtype = input.dtype if scale_dtype is None else scale_dtype
    eps = torch.finfo(input.dtype).eps if eps is None else eps
    assert len(block_size) == input.dim(), f"Got input dim:{input.dim()}, block_size: {block_size}"
    mn, mx = _block_min_max(input, block_size)
    scale = torch.clamp((mx - mn) / float(quant_max - quant_min), min=eps)
    zero_point = torch.clamp(quant_min - _Round.apply(mn / scale), quant_min, quant_max)
    zero_point_dtype = torch.int32 if zero_point_dtype is None else zero_point_dtype
    return scale.to(dtype=scale_dtype, device=input.device), zero_point.to(dtype=zero_point_dtype)


# ---------------------------------------------------------------------------------------------
# quantize
# ---------------------------------------------------------------------------------------------
def _check_float_input(input: torch.Tensor, block_size):
    assert input.dtype in (torch.float32, torch.float16, torch.bfloat16), (
        f"Unsupported input dtype: {input.dtype}"
    )
    assert len(block_size) == input.dim(), f"Got input dim:{input.dim()}, block_size: {block_size}"


def _sub_byte_storage(dtype):
    """Sub-byte unsigned dtypes are stored in uint8 (reference quant_primitives.py:509-511)."""
    if dtype in _DTYPE_TO_QVALUE_BOUNDS and str(dtype).startswith("torch.uint") and dtype != torch.uint8:
        return torch.uint8
    return dtype


@torch.no_grad()
def quantize_affine(
    input: torch.Tensor,
    block_size: Tuple[int, ...],
    scale: torch.Tensor,
    zero_point: Optional[torch.Tensor],
    output_dtype: torch.dtype,
    quant_min: Optional[Union[int, float]] = None,
    quant_max: Optional[Union[int, float]] = None,
) -> torch.Tensor:
    """Integer zero-point domain: q = clamp(round(x * (1 / s)) + zp, qmin, qmax)."""
    quant_min, quant_max = _get_and_check_qmin_qmax(output_dtype, quant_min, quant_max)
    _check_float_input(input, block_size)
    view, s = _qparam_view(scale, block_size, input.shape)
    x = input.view(view)
    q = _Round.apply(x * (1.0 / s))
    if zero_point is not None and zero_point.numel() > 0:
        q = q + _qparam_view(zero_point, block_size, input.shape)[1]
    q = torch.clamp(q, quant_min, quant_max).view(input.shape)
    return q.to(_sub_byte_storage(output_dtype))


@torch.no_grad()
def _quantize_affine_no_zero_point(
    input: torch.Tensor,
    block_size: Tuple[int, ...],
    scale: torch.Tensor,
    zero_point: Optional[torch.Tensor],
    output_dtype: torch.dtype,
    quant_min: Optional[Union[int, float]] = None,
    quant_max: Optional[Union[int, float]] = None,
) -> torch.Tensor:
    """Zero-point-free domain: q = clamp(round(x * (1 / s)), qmin, qmax)."""
    quant_min, quant_max = _get_and_check_qmin_qmax(output_dtype, quant_min, quant_max)
    _check_float_input(input, block_size)
    view, s = _qparam_view(scale, block_size, input.shape)
    q = torch.clamp(_Round.apply(input.view(view) * (1.0 / s)), quant_min, quant_max)
    return q.view(input.shape).to(_sub_byte_storage(output_dtype))


@torch.no_grad()
def _quantize_affine_tinygemm(
    input: torch.Tensor,
    block_size: List[int],
    scale: torch.Tensor,
    zero_point: Optional[torch.Tensor],
    output_dtype: torch.dtype,
    quant_min: Optional[Union[int, float]] = None,
    quant_max: Optional[Union[int, float]] = None,
) -> torch.Tensor:
    """Float zero-point domain: q = clamp(round((x - (z - s * mid)) / s), qmin, qmax)."""
    quant_min, quant_max = _get_and_check_qmin_qmax(output_dtype, quant_min, quant_max)
    _check_float_input(input, block_size)
    view, s = _qparam_view(scale, block_size, input.shape)
    mid = (quant_max + quant_min + 1) / 2
    if zero_point is not None and zero_point.numel() > 0:
        z = _qparam_view(zero_point, block_size, input.shape)[1]
        lo = z - s * mid
        q = _Round.apply((input.view(view) - lo) / s)
    else:
        q = _Round.apply(input.view(view) / s)
    q = torch.clamp(q, quant_min, quant_max).view(input.shape)
    return q.to(_sub_byte_storage(output_dtype))


# ---------------------------------------------------------------------------------------------
# dequantize
# ---------------------------------------------------------------------------------------------
@torch.no_grad()
def dequantize_affine(
    input: torch.Tensor,
    block_size: Tuple[int, ...],
    scale: torch.Tensor,
    zero_point: Optional[torch.Tensor],
    input_dtype: torch.dtype,
    quant_min: Optional[Union[int, float]] = None,
    quant_max: Optional[Union[int, float]] = None,
    *,
    output_dtype: torch.dtype = torch.float32,
) -> torch.Tensor:
    """Integer zero-point domain: x = (q - zp) * s, evaluated in ``output_dtype``."""
    _get_and_check_qmin_qmax(input_dtype, quant_min, quant_max)
    view, s = _qparam_view(scale, block_size, input.shape)
    x = input.view(view).to(output_dtype, copy=True)
    if zero_point is not None:
        x = x - _qparam_view(zero_point, block_size, input.shape)[1].to(output_dtype)
    x = x * s
    return x.view(input.shape).to(output_dtype)


@torch.no_grad()
def _dequantize_affine_no_zero_point(
    input: torch.Tensor,
    block_size: Tuple[int, ...],
    scale: torch.Tensor,
    zero_point: Optional[torch.Tensor],
    input_dtype: torch.dtype,
    quant_min: Optional[Union[int, float]] = None,
    quant_max: Optional[Union[int, float]] = None,
    *,
    output_dtype: torch.dtype = torch.float32,
) -> torch.Tensor:
    """x = q * s."""
    _get_and_check_qmin_qmax(input_dtype, quant_min, quant_max)
    view, s = _qparam_view(scale, block_size, input.shape)
    x = input.view(view).to(output_dtype, copy=True) * s
    return x.view(input.shape).to(output_dtype)


@torch.no_grad()
def _dequantize_affine_tinygemm(
    input: torch.Tensor,
    block_size: Tuple[int, ...],
    scale: torch.Tensor,
    zero_point: Optional[torch.Tensor],
    input_dtype: torch.dtype,
    quant_min: Optional[Union[int, float]] = None,
    quant_max: Optional[Union[int, float]] = None,
    *,
    output_dtype: torch.dtype = torch.float32,
) -> torch.Tensor:
    """Float zero-point domain: x = (q - mid).to(out) * s + z — two roundings in ``output_dtype``
    (the multiply, then the add), as the reference (quant_primitives.py:1017-1023)."""
    quant_min, quant_max = _get_and_check_qmin_qmax(input_dtype, quant_min, quant_max)
    view, s = _qparam_view(scale, block_size, input.shape)
    mid = (quant_max + quant_min + 1) / 2
    x = (input.view(view) - mid).to(output_dtype)
    x *= s  # in place: stays in output_dtype, one rounding
    if zero_point is not None:
        x += _qparam_view(zero_point, block_size, input.shape)[1]  # second rounding
    return x.view(input.shape).to(output_dtype)


# ---------------------------------------------------------------------------------------------
# float8 (reference quant_primitives.py:2175-2312)
# ---------------------------------------------------------------------------------------------
FP8_TYPES = {torch.float8_e4m3fn, torch.float8_e5m2, torch.float8_e4m3fnuz, torch.float8_e5m2fnuz}


@torch.no_grad()
def _choose_scale_float8(
    tensor: torch.Tensor,
    block_size: List[int],
    float8_dtype: torch.dtype = torch.float8_e4m3fn,
    scale_dtype: torch.dtype = torch.float32,
    hp_value_lb: Optional[float] = None,
    hp_value_ub: Optional[float] = None,
) -> torch.Tensor:
    """scale = amax|block| / finfo(float8_dtype).max, one per block (``block_size`` empty: one
    for the tensor), returned in fp32 with shape ``tensor.shape // block_size``.

    The division runs in the tensor's own dtype, as the reference's does: a bf16 weight gives
    bf16(amax / 448) widened to fp32. It is a tensor-by-tensor (true) division on every device;
    dividing by a Python scalar would let the GPU multiply by a reciprocal instead, and the CPU
    and GPU scales could then differ in the last bit. No eps: an all-zero block gets scale 0.
    ``hp_value_lb`` / ``hp_value_ub`` and the e8m0 scale dtype are not supported here."""
    if hp_value_lb is not None or hp_value_ub is not None:
        raise NotImplementedError("_choose_scale_float8: hp_value_lb / hp_value_ub are out of scope")
    if scale_dtype is not torch.float32:
        raise NotImplementedError("_choose_scale_float8: only float32 scales are supported")
    quant_max = torch.finfo(float8_dtype).max
    if len(block_size) == 0:
        max_abs = tensor.abs().max()
        return (max_abs / torch.full_like(max_abs, quant_max)).to(torch.float32)
    view, red = _get_reduction_params(block_size, tensor.shape)
    max_abs = tensor.view(view).abs().amax(dim=red, keepdim=True)
    scale = max_abs / torch.full_like(max_abs, quant_max)
    out_shape = [s // b for s, b in zip(tensor.shape, block_size)]
    return scale.reshape(out_shape).to(torch.float32)


def _expand_scale_to_tensor_shape(scale: torch.Tensor, target_shape: torch.Size) -> torch.Tensor:
    """A per-block scale repeated over its blocks so it multiplies a ``target_shape`` tensor
    elementwise (scalars and already-matching scales are returned as they are)."""
    if scale.shape == target_shape or scale.numel() == 1:
        return scale
    if scale.dim() != len(target_shape):
        raise ValueError(
            f"Scale tensor has {scale.dim()} dimensions but target has {len(target_shape)}"
        )
    out = scale
    for d, (t, s) in enumerate(zip(target_shape, scale.shape)):
        if t % s != 0:
            raise ValueError(
                f"Dimension {d}: target size {t} is not evenly divisible by scale size {s}"
            )
        if t != s:
            out = out.repeat_interleave(t // s, dim=d)
    return out


@torch.no_grad()
def _quantize_affine_float8(
    tensor: torch.Tensor,
    scale: torch.Tensor,
    float8_dtype: torch.dtype = torch.float8_e4m3fn,
    cast_to_float8_dtype: bool = True,
) -> torch.Tensor:
    """q = float8(clamp(float(x) / scale, -max, max)): an fp32 true division, then the dtype's
    round-to-nearest-even cast. 0 / 0 (an all-zero block) stays NaN through the clamp."""
    scaled = tensor.to(torch.float32) / _expand_scale_to_tensor_shape(scale, tensor.shape)
    max_value = torch.finfo(float8_dtype).max
    clamped = scaled.clamp(min=-max_value, max=max_value)
    return clamped.to(float8_dtype) if cast_to_float8_dtype else clamped


@torch.no_grad()
def _dequantize_affine_float8(
    tensor: torch.Tensor,
    scale: torch.Tensor,
    output_dtype: torch.dtype = torch.float32,
) -> torch.Tensor:
    """x = float(q) * scale in fp32, then one rounding to ``output_dtype``."""
    hp = tensor.to(torch.float32) * _expand_scale_to_tensor_shape(scale, tensor.shape)
    return hp.to(output_dtype)


# ---- floatx (FP6 e3m2 / e2m3; FPXWeightOnlyConfig) -----------------------------------------------
# A floatx(ebits, mbits) number is sign | ebits exponent | mbits mantissa with bias
# 2^(ebits - 1) - 1, subnormals, and no inf or NaN (every exponent is a finite binade: OCP FP6).
# Codes are uint8, 00SEEEMM for e3m2. Each row has one scale in the weight's dtype.
FLOATX_SERVED = ((3, 2), (2, 3))


def _floatx_check(ebits: int, mbits: int) -> None:
    if (ebits, mbits) not in FLOATX_SERVED:
        raise NotImplementedError(
            f"floatx (ebits, mbits) = ({ebits}, {mbits}) is not served; served: the FP6 formats "
            f"(3, 2) and (2, 3)")


def _floatx_max_normal(ebits: int, mbits: int) -> float:
    """Largest value: exponent and mantissa all ones (28 for e3m2, 7.5 for e2m3)."""
    bias = 2 ** (ebits - 1) - 1
    return 2.0 ** (2**ebits - 1 - bias) * (2.0 - 2.0 ** -mbits)


@functools.lru_cache(maxsize=16)
def _floatx_code_values(ebits: int, mbits: int, device=None) -> torch.Tensor:
    """fp32 [2^(1 + ebits + mbits)]: the value of every code, from the definition (one shared,
    read-only tensor per format and device, so that a graph capture does not meet its upload)."""
    bias = 2 ** (ebits - 1) - 1
    values = []
    for code in range(2 ** (1 + ebits + mbits)):
        e = (code >> mbits) & (2**ebits - 1)
        m = code & (2**mbits - 1)
        mag = m * 2.0 ** (1 - bias - mbits) if e == 0 else (1 + m / 2**mbits) * 2.0 ** (e - bias)
        values.append(-mag if code >> (ebits + mbits) else mag)
    return torch.tensor(values, dtype=torch.float32, device=device)


@torch.no_grad()
def _choose_qparams_affine_floatx(tensor: torch.Tensor, ebits: int, mbits: int) -> torch.Tensor:
    """scale[n] = dtype(clamp(amax_fp32 |row n|, 1e-12) / max_normal): an fp32 true division (a
    tensor divisor: torch turns a division by a Python scalar into a multiplication on the GPU),
    rounded once to the weight's dtype."""
    _floatx_check(ebits, mbits)
    amax = tensor.to(torch.float32).abs().amax(1).clamp(min=1e-12)
    max_normal = torch.full((), _floatx_max_normal(ebits, mbits), dtype=torch.float32,
                            device=tensor.device)
    return (amax / max_normal).to(tensor.dtype)


@torch.no_grad()
def _quantize_affine_floatx(tensor: torch.Tensor, scale: torch.Tensor, ebits: int,
                            mbits: int) -> torch.Tensor:
    """uint8 codes of float(x) / float(scale[n]) (an fp32 true division): round to nearest even,
    saturated at +-max_normal, subnormals and the sign of zero kept. Integer arithmetic on the
    fp32 bits; a NaN quotient takes an unspecified six-bit code."""
    _floatx_check(ebits, mbits)
    bias = 2 ** (ebits - 1) - 1
    x = tensor.to(torch.float32) / scale.to(torch.float32).view(-1, 1)
    bits = x.contiguous().view(torch.int32)
    sign = (bits >> 31) & 1
    ab = bits & 0x7FFFFFFF
    a = ab.view(torch.float32)
    shift = 23 - mbits
    # normal range: add half an fp6 ulp (minus one, plus the kept bit's parity: ties to even),
    # drop the fp32 mantissa's low bits, re-bias; a carry moves into the exponent by itself
    normal = ((ab + ((1 << (shift - 1)) - 1) + ((ab >> shift) & 1)) >> shift) - (
        (127 - bias) << mbits)
    # below the smallest normal 2^(1 - bias): whole subnormal steps 2^(1 - bias - mbits);
    # torch.round is half-to-even and the product is exact (2^mbits is the smallest normal's code)
    sub = torch.round(a * 2.0 ** (bias - 1 + mbits)).to(torch.int32)
    code = torch.where(a < 2.0 ** (1 - bias), sub, normal)
    code = torch.where(a >= _floatx_max_normal(ebits, mbits),
                       torch.full_like(code, 2 ** (ebits + mbits) - 1), code)
    # (a NaN's normal branch is wider than the field: masked, as the HIP encoder does)
    magnitude = code & (2 ** (ebits + mbits) - 1)
    return (magnitude | (sign << (ebits + mbits))).to(torch.uint8)


@torch.no_grad()
def _dequantize_affine_floatx(tensor: torch.Tensor, scale: torch.Tensor, ebits: int, mbits: int,
                              output_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """x = value(code) * float(scale[n]) in fp32, then one rounding to ``output_dtype``."""
    _floatx_check(ebits, mbits)
    values = _floatx_code_values(ebits, mbits, tensor.device)[tensor.long()]
    return (values * scale.to(torch.float32).view(-1, 1)).to(output_dtype)


# ---------------------------------------------------------------------------------------------
# HQQ (half-quadratic quantization; reference :1901-2111)
# ---------------------------------------------------------------------------------------------
HQQ_OPT_PARAMS = {"lp_norm": 0.7, "beta": 1e1, "kappa": 1.01, "iters": 20, "early_stop": True}


def _shrink_lp_op(x: torch.Tensor, beta: float, lp_norm: float) -> torch.Tensor:
    """Proximal operator of the lp norm: sign(x) * relu(|x| - |x|^(p-1) / beta)."""
    if lp_norm == 1:
        return torch.sign(x) * torch.nn.functional.relu(torch.abs(x) - 1.0 / beta)
    return torch.sign(x) * torch.nn.functional.relu(
        torch.abs(x) - (1.0 / beta) * torch.pow(torch.abs(x), lp_norm - 1)
    )


def _hqq_proximal_loop(W_f, scale, zero, min_max, axis, opt_params):
    """The proximal iteration on zero alone (scale is fixed). Returns the final zero and the
    error e_i of every iteration run (mean |W - W_r| over the whole tensor, measured with the
    zero from before that iteration's update). The update of an iteration is applied before its
    stop test, so a loop that stops at iteration i has updated zero i + 1 times."""
    lp_norm, beta, kappa = opt_params["lp_norm"], opt_params["beta"], opt_params["kappa"]
    best_error, errors = 1e4, []
    for _ in range(opt_params["iters"]):
        W_q = torch.round(W_f * scale + zero).clamp(min_max[0], min_max[1])
        W_r = (W_q - zero) / scale
        W_e = _shrink_lp_op(W_f - W_r, beta, lp_norm)
        zero = torch.mean(W_q - (W_f - W_e) * scale, axis=axis, keepdim=True)
        beta *= kappa
        current_error = float(torch.abs(W_f - W_r).mean())
        errors.append(current_error)
        if opt_params["early_stop"]:
            if current_error < best_error:
                best_error = current_error
            else:
                break
    return zero, errors


@torch.inference_mode()
def optimize_weights_proximal_legacy(
    tensor: torch.Tensor,
    scale: torch.Tensor,
    zero: torch.Tensor,
    min_max: list,
    axis: int = 0,
    dtype: Union[torch.dtype, None] = None,
    device: Union[str, None] = None,
    verbose: bool = False,
    opt_params: dict = HQQ_OPT_PARAMS,
) -> tuple:
    """Proximal solver of || W - dequantize(quantize(W)) ||_p^p over the zero point (reference
    :1913-1972). ``dtype=None`` is float32 on every device: the reference picks float16 on a GPU,
    this package serves its CPU arithmetic everywhere."""
    device = tensor.device if (device is None) else torch.device(device)
    if dtype is None:
        dtype = torch.float32
    W_f = tensor.to(dtype=dtype, device=device)
    scale = scale.to(dtype=dtype, device=device)
    zero = zero.to(dtype=dtype, device=device)
    zero, errors = _hqq_proximal_loop(W_f, scale, zero, min_max, axis, opt_params)
    if verbose:
        for i, e in enumerate(errors):
            print("Iter " + str(i + 1), " | Error: " + str(e))
    scale = scale.to(tensor.device)
    zero = zero.to(tensor.device)
    W_q = torch.round(tensor * scale + zero).clamp(min_max[0], min_max[1])
    return W_q, scale, zero


def _is_divisible(val1: int, val2: int) -> bool:
    return int(val2 * math.ceil(val1 / val2)) == val1


def _convert_to_affinequantized_format(
    W_q: torch.Tensor,
    scale: torch.Tensor,
    zero: torch.Tensor,
    nbits: int,
    shape: Union[List, Tuple, torch.Size],
) -> Tuple:
    """HQQ's W = (W_q - zero) * scale -> the affine form (W_q - mid_point) * scale_ao + zero_ao
    (reference :1980-1994)."""
    quant_min = 0
    quant_max = 2**nbits - 1
    mid_point = (quant_max + quant_min + 1) / 2
    zero_ao = ((mid_point - zero.float()) * scale.float()).to(zero.dtype)
    scale_ao = scale
    W_q_ao = W_q.view(shape)
    return W_q_ao, scale_ao, zero_ao


def _choose_qparams_and_quantize_affine_hqq(
    tensor: torch.Tensor,
    nbits: float = 4,
    group_size: int = 64,
    optimize: bool = True,
    axis: int = 1,
    compute_dtype: torch.dtype = torch.float16,
    device: str = "cuda",
    verbose: bool = False,
    raw_output: bool = False,
    optimize_weights: Callable = optimize_weights_proximal_legacy,
) -> tuple:
    """HQQ quantizer (reference :1998-2111): the min/max scale of every group, clamped at 2e4 and
    never changed afterwards, and a zero point moved by the proximal solver. Returns
    (W_q uint8 of the input's shape, scale, zero, shape) with scale / zero [numel / g, 1] in
    ``compute_dtype`` and in the affine form (W_q - 8) * scale + zero. Plain torch ops in fp32;
    bf16 GPU weights of the int4 layout take ``torchao::int4_hqq_quantize_pack`` instead
    (AffineQuantizedTensor.from_hp_to_intx). ``axis=1``, ``raw_output=False`` are served."""
    assert axis in [0, 1], "axis should be either 0 or 1"
    if axis != 1 or raw_output:
        raise NotImplementedError("HQQ: only axis=1 with raw_output=False is served")
    if group_size is not None:
        assert _is_divisible(tensor.numel(), group_size), (
            "group_size should be divisble by the total tensor dimensions. shape: "
            + str(tensor.shape)
            + ", group_size: "
            + str(group_size)
        )
    W = tensor.to(device=device, dtype=torch.float32)
    shape = W.shape
    if group_size is not None:
        W = W.reshape([-1, group_size])
    _min = W.min(axis=axis, keepdim=True)[0]
    _max = W.max(axis=axis, keepdim=True)[0]
    max_v = round(2**nbits - 1)
    min_max = [0, max_v]
    # scalar / tensor is reciprocal(tensor) * scalar in torch: two roundings, which csrc/hqq.hip
    # reproduces (an ulp in the scale moves rint(-min * scale) on a tie, and with it the group)
    scale = (max_v / (_max - _min)).clamp(max=2e4)
    zero = -_min * scale
    if nbits in [4]:
        zero = _Round.apply(zero)
    if optimize:
        W_q, scale, zero = optimize_weights(
            tensor=W, scale=scale, zero=zero, min_max=min_max, axis=axis, device=device,
            verbose=verbose,
        )
    else:
        zero = zero.to(compute_dtype)
        scale = scale.to(compute_dtype)
        W_q = _Round.apply(W * scale + zero).clamp(min_max[0], min_max[1])
    scale = 1.0 / scale
    W_q, scale, zero = _convert_to_affinequantized_format(W_q, scale, zero, nbits, shape)
    W_q = W_q.to(dtype=torch.uint8, device=device)
    scale = scale.to(dtype=compute_dtype, device=device)
    zero = zero.to(dtype=compute_dtype, device=device)
    return W_q, scale, zero, shape


# enums appear in flattened AQT metadata: allow weights_only=True checkpoint loads
torch.serialization.add_safe_globals([MappingType, ZeroPointDomain])
