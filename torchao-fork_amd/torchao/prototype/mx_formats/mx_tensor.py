"""``MXTensor``: e4m3fn codes with one E8M0 scale per 32-element block of the last dimension.

Reference: torchao/prototype/mx_formats/mx_tensor.py (``to_mx`` :133-326, ``to_dtype`` :346-427,
``MXTensor`` :466-646) and mx_ops.py (``_addmm_mx_dispatch``). ``to_mx`` / ``to_dtype`` below are
the plain-torch statement of the arithmetic (FLOOR mode, e4m3fn); they run anywhere. On the GPU
``MXTensor.to_mx`` of a bf16 tensor is the fused quantizer (``torch.ops.torchao.mx_quantize_rows``),
byte for byte the same, and ``F.linear`` on an ``MXTensor`` weight is ``mx_dyn_linear`` /
``mx_scaled_mm`` (csrc/mx_fp8.hip). There is no emulated fall-back: a CPU forward raises.
"""

from dataclasses import dataclass
from typing import Optional, Union

import torch
from torch.utils._python_dispatch import return_and_correct_aliasing

from torchao.prototype.mx_formats.config import (
    MXGemmKernelChoice,
    ScaleCalculationMode,
    _check_served,
)
from torchao.utils import TorchAOBaseTensor

aten = torch.ops.aten

BLOCK_SIZE_DEFAULT = 32
E8M0_EXPONENT_BIAS = 127
E8M0_EXPONENT_NAN_VAL = 255
F8E4M3_MAX = 448.0
F8E4M3_MAX_POW2 = 8  # 448 = 1.75 * 2^8


@dataclass
class QuantizeTensorToMXKwargs:
    """How the activation of an MX linear is quantized (the reference's fields)."""

    elem_dtype: Union[torch.dtype, str] = torch.float8_e4m3fn
    block_size: int = 32
    scaling_mode: ScaleCalculationMode = ScaleCalculationMode.FLOOR
    use_fp4_custom_triton_dequant_kernel: bool = False
    gemm_kernel_choice: MXGemmKernelChoice = MXGemmKernelChoice.EMULATED
    pack_fp6: bool = False


def to_mx(data_hp: torch.Tensor, elem_dtype=torch.float8_e4m3fn,
          block_size: int = BLOCK_SIZE_DEFAULT,
          scaling_mode: ScaleCalculationMode = ScaleCalculationMode.FLOOR,
          pack_fp6: bool = False):
    """bf16 / fp32 [..., K] -> (float8_e8m0fnu scales [..., K/32], e4m3fn codes [..., K]).

    Per block of 32 consecutive elements, from float32(x): the scale byte is the biased fp32
    exponent field of amax|x| minus 8 (F8E4M3_MAX_POW2), floored at 0, and 255 where the amax is
    NaN; the divisor is the fp32 number with that byte as exponent field, at least 2^-126; the
    code is e4m3fn(clamp(x / divisor, -448, 448)), round to nearest even, NaN kept."""
    _check_served(elem_dtype, block_size, scaling_mode, pack_fp6)
    if data_hp.dtype not in (torch.bfloat16, torch.float32):
        raise AssertionError(f"{data_hp.dtype} is not supported yet")
    K = data_hp.shape[-1]
    if K % block_size:
        raise AssertionError(f"the last dimension of shape {tuple(data_hp.shape)} must be "
                             f"divisible by block_size {block_size}")
    x = data_hp.contiguous().reshape(*data_hp.shape[:-1], K // block_size, block_size)
    x = x.to(torch.float32)
    amax = x.abs().amax(-1, keepdim=True)
    field = (amax.view(torch.int32) >> 23) & 0xFF
    byte = (field - F8E4M3_MAX_POW2).clamp(min=0)
    byte = torch.where(torch.isnan(amax), E8M0_EXPONENT_NAN_VAL, byte)
    divisor = (byte.clamp(min=1) << 23).to(torch.int32).view(torch.float32)
    codes = (x / divisor).clamp(-F8E4M3_MAX, F8E4M3_MAX).to(torch.float8_e4m3fn)
    scale = byte.to(torch.uint8).view(torch.float8_e8m0fnu).squeeze(-1)
    return scale, codes.reshape(data_hp.shape)


def get_fp_scale(scale_e8m0: torch.Tensor) -> torch.Tensor:
    """E8M0 bytes -> fp32 2^(byte - 127), built from the bits (byte 0 is the subnormal 2^-127);
    byte 255 -> NaN."""
    b = scale_e8m0.view(torch.uint8).to(torch.int32)
    bits = torch.where(b == 0, 0x00400000, b << 23)
    bits = torch.where(b == E8M0_EXPONENT_NAN_VAL, 0x7FC00000, bits)
    return bits.to(torch.int32).view(torch.float32)


def to_dtype(data_lp, scale_e8m0, elem_dtype, block_size, target_dtype,
             use_fp4_custom_triton_dequant_kernel=False, pack_fp6=False):
    """codes * 2^(scale - 127) in ``target_dtype``: the codes and the scales are converted to
    ``target_dtype`` first and multiplied there, as the reference does."""
    _check_served(elem_dtype, block_size, pack_fp6=pack_fp6)
    transposed = not data_lp.is_contiguous()
    if transposed:
        data_lp = data_lp.t()
        assert data_lp.is_contiguous()
    hp = data_lp.to(target_dtype).reshape(-1, block_size)
    hp = hp * get_fp_scale(scale_e8m0).reshape(-1, 1).to(target_dtype)
    hp = hp.reshape(data_lp.shape)
    return hp.t() if transposed else hp


class MXTensor(TorchAOBaseTensor):
    """Attributes as in the reference (so that its checkpoints load): ``qdata`` e4m3fn [N, K],
    ``_scale_e8m0`` float8_e8m0fnu [N, K/32], and the recipe."""

    tensor_data_names = ["qdata", "_scale_e8m0"]
    tensor_attribute_names = [
        "_elem_dtype",
        "_block_size",
        "_orig_dtype",
        "_use_fp4_custom_triton_dequant_kernel",
        "_gemm_kernel_choice",
        "_pack_fp6",
        "act_quant_kwargs",
    ]

    def __new__(cls, qdata, scale_e8m0_bits, elem_dtype, block_size, orig_dtype,
                use_fp4_custom_triton_dequant_kernel, gemm_kernel_choice, pack_fp6,
                act_quant_kwargs):
        _check_served(elem_dtype, block_size, pack_fp6=pack_fp6)
        if qdata.dtype != torch.float8_e4m3fn or scale_e8m0_bits.dtype != torch.float8_e8m0fnu:
            raise TypeError("MXTensor holds float8_e4m3fn codes and float8_e8m0fnu scales, got "
                            f"{qdata.dtype} and {scale_e8m0_bits.dtype}")
        if scale_e8m0_bits.numel() * block_size != qdata.numel():
            raise ValueError(f"MXTensor: {scale_e8m0_bits.numel()} scales do not cover "
                             f"{qdata.numel()} codes in blocks of {block_size}")
        self = torch.Tensor._make_wrapper_subclass(
            cls, qdata.size(), strides=qdata.stride(), storage_offset=qdata.storage_offset(),
            layout=qdata.layout, dtype=orig_dtype, device=qdata.device)
        self.qdata = qdata
        self._scale_e8m0 = scale_e8m0_bits
        self._elem_dtype = elem_dtype
        self._block_size = block_size
        self._orig_dtype = orig_dtype
        self._use_fp4_custom_triton_dequant_kernel = use_fp4_custom_triton_dequant_kernel
        self._gemm_kernel_choice = gemm_kernel_choice
        self._pack_fp6 = pack_fp6
        self.act_quant_kwargs = act_quant_kwargs
        return self

    def __repr__(self):
        act = self.act_quant_kwargs
        return (f"MXTensor(shape={tuple(self.shape)}, elem_dtype={self._elem_dtype}, "
                f"block_size={self._block_size}, orig_dtype={self._orig_dtype}, "
                f"device={self.qdata.device}, gemm_kernel_choice={self._gemm_kernel_choice.name}, "
                f"activation={'none (weight-only)' if act is None else act.elem_dtype})")

    def __tensor_flatten__(self):
        return self.tensor_data_names, [getattr(self, n) for n in self.tensor_attribute_names]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        return cls(tensor_data_dict["qdata"], tensor_data_dict["_scale_e8m0"], *tensor_attributes)

    def _map(self, fn):
        """The same recipe around fn(codes), fn(scales)."""
        recipe = [getattr(self, n) for n in self.tensor_attribute_names]
        return MXTensor(fn(self.qdata), fn(self._scale_e8m0), *recipe)

    def to_dtype(self, target_dtype):
        return to_dtype(self.qdata, self._scale_e8m0, torch.float8_e4m3fn, 32, target_dtype)

    def dequantize(self, output_dtype: Optional[torch.dtype] = None):
        return self.to_dtype(self._orig_dtype if output_dtype is None else output_dtype)

    def to(self, *args, **kwargs):
        kw = self._get_to_kwargs(*args, **kwargs)
        if kw["dtype"] != self.dtype:
            raise NotImplementedError("MXTensor.to: a dtype change is not supported; dequantize()")
        return self._map(lambda t: t.to(device=kw["device"]))

    @staticmethod
    def to_mx(data_hp: torch.Tensor, elem_dtype=torch.float8_e4m3fn,
              block_size: int = BLOCK_SIZE_DEFAULT,
              scaling_mode: ScaleCalculationMode = ScaleCalculationMode.FLOOR,
              use_fp4_custom_triton_dequant_kernel: bool = False,
              gemm_kernel_choice: MXGemmKernelChoice = MXGemmKernelChoice.EMULATED,
              pack_fp6: bool = False,
              act_quant_kwargs: Optional[QuantizeTensorToMXKwargs] = None):
        """The fused HIP quantizer for a bf16 tensor on the GPU, ``to_mx`` above otherwise: the
        same bytes either way."""
        _check_served(elem_dtype, block_size, scaling_mode, pack_fp6)
        if data_hp.is_cuda and data_hp.dtype == torch.bfloat16:
            if data_hp.shape[-1] % block_size:
                raise AssertionError(f"the last dimension of shape {tuple(data_hp.shape)} must "
                                     f"be divisible by block_size {block_size}")
            codes, scale = torch.ops.torchao.mx_quantize_rows(data_hp)
            scale = scale.view(torch.float8_e8m0fnu)
        else:
            scale, codes = to_mx(data_hp, elem_dtype, block_size, scaling_mode, pack_fp6)
        return MXTensor(codes, scale, elem_dtype, block_size, data_hp.dtype,
                        use_fp4_custom_triton_dequant_kernel, gemm_kernel_choice, pack_fp6,
                        act_quant_kwargs)


implements = MXTensor.implements


def _scale_bytes(t: MXTensor) -> torch.Tensor:
    """The scales as the ops take them: uint8 [rows, K/32]."""
    K = t.qdata.shape[-1]
    return t._scale_e8m0.view(torch.uint8).reshape(-1, K // t._block_size)


@implements([torch.nn.functional.linear, aten.linear.default])
def _(func, types, args, kwargs):
    x, w = args[0], args[1]
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    if not isinstance(w, MXTensor):
        raise NotImplementedError("MXTensor: F.linear needs an MXTensor weight")
    if w.qdata.dim() != 2 or not w.qdata.is_contiguous():
        raise NotImplementedError("MXTensor: F.linear needs a contiguous [N, K] weight")
    if not w.qdata.is_cuda:
        raise NotImplementedError(
            "MXTensor: the MXFP8 linear runs on the GPU only (HIP kernels, csrc/mx_fp8.hip); "
            "there is no emulated CPU path. Move the module to the GPU, or dequantize().")
    if isinstance(x, MXTensor):
        return torch.ops.torchao.mx_scaled_mm(x.qdata, _scale_bytes(x), w.qdata, _scale_bytes(w),
                                              bias)
    if w.act_quant_kwargs is None:
        raise NotImplementedError("MXTensor: weight-only quant not yet supported")
    k = w.act_quant_kwargs
    _check_served(k.elem_dtype, k.block_size, k.scaling_mode, k.pack_fp6)
    return torch.ops.torchao.mx_dyn_linear(x, w.qdata, _scale_bytes(w), bias)


def _on_both(fn=None, move=False):
    """An aten op that acts on codes and scales alike: fn (the op itself when None) on each,
    after MXTensor.to for the copying ops."""
    def impl(func, types, args, kwargs):
        src = args[0].to(*args[1:], **kwargs) if move else args[0]
        return return_and_correct_aliasing(func, args, kwargs, src._map(fn or func))
    return impl


implements([aten.detach.default, aten.alias.default])(_on_both())
implements(aten.clone.default)(_on_both(torch.clone))
implements(aten._to_copy.default)(_on_both(torch.clone, move=True))


@implements(aten.copy_.default)
def _(func, types, args, kwargs):
    dst, src = args[0], args[1]
    if (isinstance(dst, MXTensor) and isinstance(src, MXTensor) and dst.shape == src.shape
            and dst._elem_dtype == src._elem_dtype and dst._block_size == src._block_size
            and dst._orig_dtype == src._orig_dtype):
        dst.qdata.copy_(src.qdata)
        dst._scale_e8m0.view(torch.uint8).copy_(
            src._scale_e8m0.view(torch.uint8).reshape(dst._scale_e8m0.shape))
        return dst
    raise ValueError(f"Not supported args for copy_ due to metadata mismatch: {dst, src}")


torch.serialization.add_safe_globals([MXTensor, QuantizeTensorToMXKwargs])
