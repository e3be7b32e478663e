"""FP6 (e3m2 / e2m3) layout of ``AffineQuantizedTensor`` and its weight-only linear on MI355X.

Reference: torchao/dtypes/floatx/floatx_tensor_core_layout.py. ``FloatxTensorCoreLayout(ebits,
mbits)`` and ``FloatxTensorCoreAQTTensorImpl`` keep its module path, attribute names
(``packed_floatx_data``, ``scale``, ``_layout``), flatten keys and ``get_plain()`` (uint8 codes
[N, K] as 00SEEEMM, scale), so a ``state_dict`` it saved after ``fpx_weight_only`` loads here with
``torch.load(weights_only=True)``.

Storage. The reference keeps ``packed_floatx_data`` as uint8 [N, K * 6 / 8] in the FP6-LLM
tensor-core pre-packing: every code split into a 2-bit and a 4-bit fragment, both shuffled for
NVIDIA MMA fragments. The gfx950 kernels want a row's codes in order, so the storage here is

    packed_floatx_data  int32 [N, K * 6 / 32]   code k of a row at bits 6 k .. 6 k + 5 of the row's
                                                little-endian bit stream: 32 codes = 6 dwords = one
                                                operand of v_cvt_scalef32_pk32_bf16_{bf6,fp6}
    scale               bf16  [N]

The two are told apart by dtype. ``_adopt`` converts reference storage when an AQT is unpickled or
unflattened (the int4 precedent: uintx/tensor_core_tiled_layout.py);
``convert_from_floatx_tensor_core`` / ``convert_to_floatx_tensor_core`` are the two directions as
functions, on any device.

Linear. bf16 activations on the GPU run ``torch.ops.torchao.fp6_weight_only_linear`` (csrc/fp6.hip:
the decode GEMV up to the boundary of csrc/fp6_host.h, the HIP dequantizer + bf16 matmul above);
on the CPU the linear is ``F.linear(x, W.dequantize(), bias)`` (the reference raises there: its
kernel is CUDA only). Other activation dtypes take the dispatch table's dequantize fallback.
Only the two FP6 formats are served; the reference's fp5 forms (e2m2, e3m1) raise.
"""

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch.utils._python_dispatch import (
    is_traceable_wrapper_subclass,
    return_and_correct_aliasing,
)

from torchao.dtypes.affine_quantized_tensor import AffineQuantizedTensor, register_layout
from torchao.dtypes.utils import AQTTensorImpl, Layout
from torchao.quantization.quant_primitives import FLOATX_SERVED

aten = torch.ops.aten

__all__ = [
    "FloatxTensorCoreLayout",
    "FloatxTensorCoreAQTTensorImpl",
    "pack_floatx_native",
    "unpack_floatx_native",
    "convert_from_floatx_tensor_core",
    "convert_to_floatx_tensor_core",
]


def _check_fp6(ebits: int, mbits: int) -> None:
    if (ebits, mbits) not in FLOATX_SERVED:
        raise NotImplementedError(
            f"floatx (ebits, mbits) = ({ebits}, {mbits}) is not served; served: the FP6 formats "
            f"(3, 2) and (2, 3)")


# ---- native storage <-> codes ----------------------------------------------------------------------
def pack_floatx_native(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes [N, K] (K % 32 == 0, values < 64) -> int32 [N, K * 6 / 32]. Four codes are three
    bytes of the bit stream: c0 | c1 << 6, c1 >> 2 | c2 << 4, c2 >> 4 | c3 << 2."""
    assert codes.dim() == 2 and codes.dtype == torch.uint8, "codes must be uint8 [N, K]"
    N, K = codes.shape
    assert K % 32 == 0, f"K ({K}) must be a multiple of 32"
    c = codes.reshape(N, K // 4, 4).to(torch.int32) & 0x3F  # a wider value stays in its field
    c0, c1, c2, c3 = c.unbind(-1)
    b = torch.stack([c0 | (c1 << 6), (c1 >> 2) | (c2 << 4), (c2 >> 4) | (c3 << 2)], -1) & 0xFF
    return b.to(torch.uint8).reshape(N, K * 3 // 4).contiguous().view(torch.int32)


def unpack_floatx_native(packed: torch.Tensor) -> torch.Tensor:
    """int32 [N, K * 6 / 32] -> uint8 codes [N, K]."""
    assert packed.dim() == 2 and packed.dtype == torch.int32, "native storage is int32 [N, K*6/32]"
    N = packed.shape[0]
    b = packed.contiguous().view(torch.uint8).reshape(N, -1, 3).to(torch.int32)
    b0, b1, b2 = b.unbind(-1)
    c = torch.stack([b0, (b0 >> 6) | (b1 << 2), (b1 >> 4) | (b2 << 4), b2 >> 2], -1) & 0x3F
    return c.to(torch.uint8).reshape(N, -1)


# ---- the reference's tensor-core pre-packing -------------------------------------------------------
# For a weight [N, K] (N % 64 == 0, K % 64 == 0) the N K codes are cut into their top 2 bits and
# low 4 bits. All 2-bit fragments come first (N K / 4 bytes, four per byte, the first in the
# byte's top bits), then all 4-bit fragments (N K / 2 bytes, two per byte, the first in the high
# nibble). With row n = 64 n0 + 32 a + 16 b + 8 c + d and column k = 16 k0 + 8 e + f, fragment
# streams are ordered (slowest first)
#     2-bit: n0, k0, a, d, f, 1 - c, b, e        4-bit: n0, k0, a, b, d, f, 1 - c, e
# (tests/golden/fp6_*.npz pin this map byte for byte).
def _tc_positions(N: int, K: int, dev):
    """(p2, p4) int64 [N, K]: where element (n, k)'s fragments sit in the two streams. Computed
    per call and freed with it: a conversion runs once per weight, and the two maps of a
    14336 x 4096 weight are 0.9 GB."""
    n = torch.arange(N, device=dev).view(N, 1)
    k = torch.arange(K, device=dev).view(1, K)
    n0, a, b, c, d = n // 64, (n // 32) % 2, (n // 16) % 2, (n // 8) % 2, n % 8
    k0, e, f = k // 16, (k // 8) % 2, k % 8
    tile = n0 * (K // 16) + k0
    p2 = (((((tile * 2 + a) * 8 + d) * 8 + f) * 2 + (1 - c)) * 2 + b) * 2 + e
    p4 = (((((tile * 2 + a) * 2 + b) * 8 + d) * 8 + f) * 2 + (1 - c)) * 2 + e
    return p2, p4


def _tc_unpack(packed_u8: torch.Tensor) -> torch.Tensor:
    """The reference's uint8 [N, K * 6 / 8] -> uint8 codes [N, K]: two gathers."""
    assert packed_u8.dim() == 2 and packed_u8.dtype == torch.uint8
    N = packed_u8.shape[0]
    K = packed_u8.shape[1] // 3 * 4
    assert N % 64 == 0 and K % 64 == 0 and packed_u8.shape[1] * 4 == K * 3, (
        f"the tensor-core format holds weights with N % 64 == 0 and K % 64 == 0, got storage "
        f"{tuple(packed_u8.shape)}")
    flat = packed_u8.reshape(-1).to(torch.int32)
    s2, s4 = flat[: N * K // 4], flat[N * K // 4:]
    p2, p4 = _tc_positions(N, K, packed_u8.device)
    hi = (s2[p2 // 4] >> (6 - 2 * (p2 % 4))) & 3
    lo = (s4[p4 // 2] >> (4 - 4 * (p4 % 2))) & 15
    return ((hi << 4) | lo).to(torch.uint8)


def _tc_pack(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes [N, K] -> the reference's uint8 [N, K * 6 / 8]: two scatters (the position maps
    are permutations), then 4 resp. 2 fragments per byte."""
    assert codes.dim() == 2 and codes.dtype == torch.uint8
    N, K = codes.shape
    assert N % 64 == 0 and K % 64 == 0, (
        f"the tensor-core format holds weights with N % 64 == 0 and K % 64 == 0, got {N} x {K}")
    p2, p4 = _tc_positions(N, K, codes.device)
    c = codes.to(torch.int32)
    s2 = torch.empty(N * K, dtype=torch.int32, device=codes.device)
    s4 = torch.empty(N * K, dtype=torch.int32, device=codes.device)
    s2[p2.reshape(-1)] = ((c >> 4) & 3).reshape(-1)
    s4[p4.reshape(-1)] = (c & 15).reshape(-1)
    s2 = s2.view(-1, 4)
    s4 = s4.view(-1, 2)
    b2 = (s2[:, 0] << 6) | (s2[:, 1] << 4) | (s2[:, 2] << 2) | s2[:, 3]
    b4 = (s4[:, 0] << 4) | s4[:, 1]
    return torch.cat([b2, b4]).to(torch.uint8).view(N, K * 3 // 4)


def convert_from_floatx_tensor_core(packed_u8: torch.Tensor, ebits: int, mbits: int) -> torch.Tensor:
    """Reference storage (uint8 [N, K * 6 / 8]) -> native storage (int32 [N, K * 6 / 32])."""
    _check_fp6(ebits, mbits)
    return pack_floatx_native(_tc_unpack(packed_u8))


def convert_to_floatx_tensor_core(packed_i32: torch.Tensor, ebits: int, mbits: int) -> torch.Tensor:
    """Native storage -> reference storage, for handing a weight back to the reference."""
    _check_fp6(ebits, mbits)
    return _tc_pack(unpack_floatx_native(packed_i32))


# ---- layout and impl ---------------------------------------------------------------------------------
@dataclass(frozen=True)
class FloatxTensorCoreLayout(Layout):
    """floatx(ebits, mbits) data packed for the tensor / matrix cores (reference name)."""

    ebits: int
    mbits: int


@register_layout(FloatxTensorCoreLayout)
class FloatxTensorCoreAQTTensorImpl(AQTTensorImpl):
    """``packed_floatx_data`` (native int32 [N, K * 6 / 32]; uint8 [N, K * 6 / 8] only between
    unpickling a reference checkpoint and ``_adopt``), ``scale`` [N], ``_layout``."""

    def __new__(cls, packed_floatx_data: torch.Tensor, scale: torch.Tensor, _layout: Layout):
        assert packed_floatx_data.ndim == 2
        assert packed_floatx_data.dtype in (torch.int32, torch.uint8), (
            f"packed_floatx_data must be int32 (native) or uint8 (reference format), got "
            f"{packed_floatx_data.dtype}")
        nbits = 1 + _layout.ebits + _layout.mbits
        per = 32 if packed_floatx_data.dtype == torch.int32 else 8
        shape = (packed_floatx_data.shape[0], packed_floatx_data.shape[1] // nbits * per)
        return torch.Tensor._make_wrapper_subclass(
            cls,
            shape,
            device=packed_floatx_data.device,
            layout=packed_floatx_data.layout,
            dtype=packed_floatx_data.dtype,
            requires_grad=False,
        )

    def __init__(self, packed_floatx_data: torch.Tensor, scale: torch.Tensor, _layout: Layout):
        self.packed_floatx_data = packed_floatx_data
        self.scale = scale
        self._layout = _layout

    def __tensor_flatten__(self):
        return ["packed_floatx_data", "scale"], [self._layout]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        (_layout,) = tensor_attributes
        return cls(tensor_data_dict["packed_floatx_data"], tensor_data_dict["scale"], _layout)

    @classmethod
    def _adopt(cls, impl, shape):
        """Called when an AQT is unpickled / unflattened with this impl: storage in the reference's
        tensor-core format (uint8) is converted to the native bit stream; native storage is
        returned as it is."""
        if impl.packed_floatx_data.dtype != torch.uint8:
            return impl
        lay = impl._layout
        native = convert_from_floatx_tensor_core(impl.packed_floatx_data, lay.ebits, lay.mbits)
        return cls(native, impl.scale, lay)

    def _native(self) -> torch.Tensor:
        if self.packed_floatx_data.dtype == torch.uint8:
            lay = self._layout
            return convert_from_floatx_tensor_core(self.packed_floatx_data, lay.ebits, lay.mbits)
        return self.packed_floatx_data

    def get_plain(self) -> Tuple[torch.Tensor, torch.Tensor]:
        return unpack_floatx_native(self._native()), self.scale

    @classmethod
    def from_plain(cls, unpacked_floatx_data: torch.Tensor, scale: torch.Tensor,
                   zero_point: Optional[torch.Tensor], _layout: Layout):
        """``unpacked_floatx_data``: uint8 [N, K], zero padding | sign | exponent | mantissa
        (00SEEEMM for e3m2)."""
        assert isinstance(_layout, FloatxTensorCoreLayout)
        _check_fp6(_layout.ebits, _layout.mbits)
        return cls(pack_floatx_native(unpacked_floatx_data), scale, _layout)

    def __repr__(self):
        data, scale = self.get_plain()
        return (f"{type(self).__name__}(unpacked_floatx_data={data}, scale={scale}, "
                f"_layout={self._layout})")

    def _apply_fn_to_data(self, fn):
        return type(self)(fn(self.packed_floatx_data), fn(self.scale), self._layout)

    def to(self, *args, **kwargs):
        device = self._get_to_kwargs(*args, **kwargs)["device"]
        return type(self)(self.packed_floatx_data.to(device), self.scale.to(device), self._layout)

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs):
        kwargs = {} if kwargs is None else kwargs
        if func in (aten.detach.default, aten.alias.default):
            return return_and_correct_aliasing(
                func, args, kwargs, args[0]._apply_fn_to_data(torch.detach))
        if func is aten.clone.default:
            return return_and_correct_aliasing(
                func, args, kwargs, args[0]._apply_fn_to_data(torch.clone))
        if func is aten._to_copy.default:
            return return_and_correct_aliasing(
                func, args, kwargs, args[0].to(*args[1:], **kwargs)._apply_fn_to_data(torch.clone))
        raise NotImplementedError(
            f"FloatxTensorCoreAQTTensorImpl dispatch: attempting to run {func}, this is not "
            f"supported")

    __torch_function__ = torch._C._disabled_torch_function_impl

    def get_layout(self) -> Layout:
        return self._layout


# ---- the quantized-linear pair ---------------------------------------------------------------------
def _is_fp6_weight(weight_tensor) -> bool:
    return (
        isinstance(weight_tensor, AffineQuantizedTensor)
        and isinstance(weight_tensor._layout, FloatxTensorCoreLayout)
        and (weight_tensor._layout.ebits, weight_tensor._layout.mbits) in FLOATX_SERVED
    )


def _linear_bf16_act_floatx_weight_check(input_tensor, weight_tensor, bias) -> bool:
    return (
        not is_traceable_wrapper_subclass(input_tensor)
        and input_tensor.dtype == torch.bfloat16
        and _is_fp6_weight(weight_tensor)
    )


def _linear_bf16_act_floatx_weight_impl(input_tensor, weight_tensor, bias):
    """y = bf16(fp32(x . value(codes)) * scale) (+ bias) on the GPU (csrc/fp6.hip; a missing
    kernel is an error); on the CPU F.linear on the dequantized weight."""
    impl = weight_tensor.tensor_impl
    lay = impl._layout
    if not input_tensor.is_cuda:
        return torch.nn.functional.linear(input_tensor, weight_tensor.dequantize(), bias)
    return torch.ops.torchao.fp6_weight_only_linear(
        input_tensor, impl._native(), impl.scale, lay.ebits, lay.mbits, bias)
