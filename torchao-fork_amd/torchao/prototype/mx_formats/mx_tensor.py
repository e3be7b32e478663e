"""``MXTensor``: e4m3fn codes, or e2m1 codes two per byte (weights), with one E8M0 scale per
32-element block of the last dimension.

Reference: torchao/prototype/mx_formats/mx_tensor.py (``to_mx`` :133-326, ``to_dtype`` :346-427,
``MXTensor`` :466-646) and mx_ops.py (``_addmm_mx_dispatch``). ``to_mx`` / ``to_dtype`` below are
the plain-torch statement of the arithmetic (FLOOR mode, e4m3fn); they run anywhere. On the GPU
``MXTensor.to_mx`` of a bf16 tensor is the fused quantizer (``torch.ops.torchao.mx_quantize_rows``),
byte for byte the same, and ``F.linear`` on an ``MXTensor`` weight is ``mx_dyn_linear`` /
``mx_scaled_mm`` (csrc/mx_fp8.hip). An e2m1 (``torch.float4_e2m1fn_x2``) weight keeps the reference's
packing (element 2 j in the high nibble of byte j); its quantizer is ``mxfp4_quantize_rows`` and its
linear, under e4m3fn activations, ``mxfp4w_dyn_linear`` / ``mxfp4w_scaled_mm`` (csrc/mx_fp4.hip).
There is no emulated fall-back: a CPU forward raises.
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
F4_E2M1 = torch.float4_e2m1fn_x2
F4_E2M1_MAX_POW2 = 2  # 6 = 1.5 * 2^2
F4_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # the magnitude codes; bit 3 is the sign


@dataclass
class QuantizeTensorToMXKwargs:
    """How the activation of an MX linear is quantized (the reference's fields)."""

    elem_dtype: Union[torch.dtype, str] = torch.float8_e4m3fn
    block_size: int = 32
    scaling_mode: ScaleCalculationMode = ScaleCalculationMode.FLOOR
    use_fp4_custom_triton_dequant_kernel: bool = False
    gemm_kernel_choice: MXGemmKernelChoice = MXGemmKernelChoice.EMULATED
    pack_fp6: bool = False


def _f32_to_e2m1_codes(y: torch.Tensor) -> torch.Tensor:
    """fp32 -> uint8 e2m1 codes (sign bit 3), round to nearest even, saturating at +-6 (inf too).
    Below 1 the codes 0, 1, 2 lie 0.5 apart (ties 0.25 -> 0, 0.75 -> 2); in [1, 6) the code is the
    top of the fp32 pattern rebiased from 127 to 1 and rounded at bit 22, ties to the even code. A
    NaN pattern takes that last formula, its low byte kept (the default NaN gives 3), as the
    reference's integer arithmetic does."""
    bits = y.contiguous().view(torch.int32)
    a = bits & 0x7FFFFFFF
    norm = ((a - (126 << 23) + 0x1FFFFF + ((a >> 22) & 1)) >> 22) & 0xFF
    sub = (a > 0x3E800000).to(torch.int32) + (a >= 0x3F400000).to(torch.int32)
    code = torch.where(a < 0x3F800000, sub, norm)
    code = torch.where((a >= 0x40C00000) & (a <= 0x7F800000), 7, code)
    return (((bits >> 28) & 8) | (code & 0xF)).to(torch.uint8)


def _pack_e2m1(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes [..., K] -> [..., K/2], element 2 j in the high nibble of byte j."""
    return (codes[..., ::2] << 4) | codes[..., 1::2]


def _unpack_e2m1(packed: torch.Tensor) -> torch.Tensor:
    return torch.stack([packed >> 4, packed & 0xF], dim=-1).reshape(*packed.shape[:-1], -1)


def to_mx(data_hp: torch.Tensor, elem_dtype=torch.float8_e4m3fn,
          block_size: int = BLOCK_SIZE_DEFAULT,
          scaling_mode: ScaleCalculationMode = ScaleCalculationMode.FLOOR,
          pack_fp6: bool = False):
    """bf16 / fp32 [..., K] -> (float8_e8m0fnu scales [..., K/32], e4m3fn codes [..., K]).

    Per block of 32 consecutive elements, from float32(x): the scale byte is the biased fp32
    exponent field of amax|x| minus 8 (F8E4M3_MAX_POW2), floored at 0, and 255 where the amax is
    NaN; the divisor is the fp32 number with that byte as exponent field, at least 2^-126; the
    code is e4m3fn(clamp(x / divisor, -448, 448)), round to nearest even, NaN kept.

    ``torch.float4_e2m1fn_x2``: the exponent field minus 2 (F4_E2M1_MAX_POW2), no clamp before
    the cast (it saturates at +-6), and the codes packed two per byte: uint8 [..., K/2]."""
    _check_served(elem_dtype, block_size, scaling_mode, pack_fp6, weight=True)
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
    fp4 = elem_dtype == F4_E2M1
    byte = (field - (F4_E2M1_MAX_POW2 if fp4 else F8E4M3_MAX_POW2)).clamp(min=0)
    byte = torch.where(torch.isnan(amax), E8M0_EXPONENT_NAN_VAL, byte)
    divisor = (byte.clamp(min=1) << 23).to(torch.int32).view(torch.float32)
    scale = byte.to(torch.uint8).view(torch.float8_e8m0fnu).squeeze(-1)
    if fp4:
        return scale, _pack_e2m1(_f32_to_e2m1_codes(x / divisor).reshape(data_hp.shape))
    codes = (x / divisor).clamp(-F8E4M3_MAX, F8E4M3_MAX).to(torch.float8_e4m3fn)
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
    ``target_dtype`` first and multiplied there, as the reference does. Packed e2m1 codes are
    unpacked and looked up in the value table (``use_fp4_custom_triton_dequant_kernel`` picks
    nothing)."""
    _check_served(elem_dtype, block_size, pack_fp6=pack_fp6, weight=True)
    transposed = not data_lp.is_contiguous()
    if transposed:
        data_lp = data_lp.t()
        assert data_lp.is_contiguous()
    if elem_dtype == F4_E2M1:
        u = _unpack_e2m1(data_lp)
        table = torch.tensor(F4_E2M1_VALUES + tuple(-v for v in F4_E2M1_VALUES),
                             dtype=torch.float32, device=u.device)
        hp = table[u.long()].to(target_dtype)
    else:
        hp = data_lp.to(target_dtype)
    shape = hp.shape
    hp = hp.reshape(-1, block_size)
    hp = hp * get_fp_scale(scale_e8m0).reshape(-1, 1).to(target_dtype)
    hp = hp.reshape(shape)
    return hp.t() if transposed else hp


class MXTensor(TorchAOBaseTensor):
    """Attributes as in the reference (so that its checkpoints load): ``qdata`` e4m3fn [N, K], or
    uint8 [N, K/2] for ``_elem_dtype`` float4_e2m1fn_x2 (the tensor's own shape is the logical
    [N, K] either way), ``_scale_e8m0`` float8_e8m0fnu [N, K/32], and the recipe."""

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
        _check_served(elem_dtype, block_size, pack_fp6=pack_fp6, weight=True)
        fp4 = elem_dtype == F4_E2M1
        want = torch.uint8 if fp4 else torch.float8_e4m3fn
        if qdata.dtype != want or scale_e8m0_bits.dtype != torch.float8_e8m0fnu:
            raise TypeError(f"MXTensor ({elem_dtype}) holds {want} codes and float8_e8m0fnu "
                            f"scales, got {qdata.dtype} and {scale_e8m0_bits.dtype}")
        per_byte = 2 if fp4 else 1
        if scale_e8m0_bits.numel() * block_size != per_byte * qdata.numel():
            raise ValueError(f"MXTensor: {scale_e8m0_bits.numel()} scales do not cover "
                             f"{per_byte * qdata.numel()} codes in blocks of {block_size}")
        size = list(qdata.size())
        if fp4:  # the logical size; the packed dimension is the contiguous one (as the reference)
            size[-1 if qdata.is_contiguous() else 0] *= 2
        self = torch.Tensor._make_wrapper_subclass(
            cls, size, strides=qdata.stride(), storage_offset=qdata.storage_offset(),
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
        return to_dtype(self.qdata, self._scale_e8m0, self._elem_dtype, 32, target_dtype)

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
        _check_served(elem_dtype, block_size, scaling_mode, pack_fp6, weight=True)
        if data_hp.is_cuda and data_hp.dtype == torch.bfloat16:
            if data_hp.shape[-1] % block_size:
                raise AssertionError(f"the last dimension of shape {tuple(data_hp.shape)} must "
                                     f"be divisible by block_size {block_size}")
            if elem_dtype == F4_E2M1:
                codes, scale = torch.ops.torchao.mxfp4_quantize_rows(data_hp)
            else:
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
    K = t.shape[-1]
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
            "MXTensor: the MX linear runs on the GPU only (HIP kernels, csrc/mx_fp8.hip, "
            "csrc/mx_fp4.hip); "
            "there is no emulated CPU path. Move the module to the GPU, or dequantize().")
    fp4 = w._elem_dtype == F4_E2M1
    if isinstance(x, MXTensor):
        # an activation is e4m3fn: refused by name if it is anything else
        _check_served(x._elem_dtype, x._block_size)
        mm = torch.ops.torchao.mxfp4w_scaled_mm if fp4 else torch.ops.torchao.mx_scaled_mm
        return mm(x.qdata, _scale_bytes(x), w.qdata, _scale_bytes(w), bias)
    if w.act_quant_kwargs is None:
        raise NotImplementedError("MXTensor: weight-only quant not yet supported")
    k = w.act_quant_kwargs
    _check_served(k.elem_dtype, k.block_size, k.scaling_mode, k.pack_fp6)
    linear = torch.ops.torchao.mxfp4w_dyn_linear if fp4 else torch.ops.torchao.mx_dyn_linear
    return linear(x, w.qdata, _scale_bytes(w), bias)


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
