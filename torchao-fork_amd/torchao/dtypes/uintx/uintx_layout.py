"""``UintxLayout``: 1- to 7-bit codes bit-packed into shards, and their linear on MI355X.

Reference: torchao/dtypes/uintx/uintx_layout.py (``UintxTensor``, ``to_uintx``, ``UintxLayout``,
``UintxAQTTensorImpl``; same names, fields and pickled attributes, so a reference ``state_dict``
loads here and the other way round). ``UintxTensor`` holds the shards of
``torchao.dtypes.uintx.bitpacking``; ``UintxAQTTensorImpl`` is the plain impl whose ``int_data``
is such a tensor.

The reference has no kernel for this layout on any device: its linear unpacks the shards,
dequantizes the whole weight and calls ``F.linear``. Here bf16 activations on the GPU with
``K % 128 == 0`` and ``group_size % 16 == 0`` run ``torch.ops.torchao.uintx_weight_only_linear``
(csrc/uintx.hip), which reads the shards in place (above 8 tokens it dequantizes into a temporary
and calls the bf16 matmul; under ``torchao.kernel.tuning.tuning(uintx_mfma=1)`` an MFMA GEMM on
the same shards serves those calls where ``group_size % 32 == 0``); every other input takes the table's generic
dequantize -> ``F.linear`` route, the reference's arithmetic. One addition to the reference's
surface: ``UintxTensor`` is registered as a safe global, so a ``state_dict`` saved here loads with
``weights_only=True``.
"""

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
from torch.utils._python_dispatch import (
    is_traceable_wrapper_subclass,
    return_and_correct_aliasing,
)

from torchao.dtypes.affine_quantized_tensor import AffineQuantizedTensor, register_layout
from torchao.dtypes.uintx.bitpacking import pack, unpack
from torchao.dtypes.uintx.plain_layout import PlainAQTTensorImpl
from torchao.dtypes.utils import Layout
from torchao.quantization.quant_primitives import ZeroPointDomain
from torchao.utils import TorchAOBaseTensor

aten = torch.ops.aten

__all__ = ["UintxTensor", "to_uintx", "UintxLayout", "UintxAQTTensorImpl"]

_DTYPE_TO_BIT_WIDTH = {getattr(torch, f"uint{b}"): b for b in range(1, 8)}
_BIT_WIDTH_TO_DTYPE = {b: d for d, b in _DTYPE_TO_BIT_WIDTH.items()}


class UintxTensor(TorchAOBaseTensor):
    """uint8 codes of ``bit_width`` bits, stored as packed shards.

    fields: ``int4_shard`` / ``int2_shard`` / ``int1_shard`` (those of the set bits of
    ``bit_width``), ``packed_shape`` (of the unpacked codes: the tensor's own shape),
    ``bit_width``, ``pack_dim``.
    """

    bits_to_shard = {
        b: [f"int{w}_shard" for w in (4, 2, 1) if b & w] for b in range(1, 8)
    }

    def __new__(cls, shards: List[torch.Tensor], packed_shape: List[int], bit_width: int,
                pack_dim: int = -1):
        return torch.Tensor._make_wrapper_subclass(
            cls, packed_shape, device=shards[0].device, layout=shards[0].layout,
            dtype=torch.uint8, requires_grad=False,
        )

    def __init__(self, shards: List[torch.Tensor], packed_shape: List[int], bit_width: int,
                 pack_dim: int = -1):
        names = self.bits_to_shard[bit_width]
        assert len(shards) == len(names), f"uint{bit_width} has {len(names)} shards"
        for name, shard in zip(names, shards):
            setattr(self, name, shard)
        self.packed_shape = packed_shape
        self.bit_width = bit_width
        self.pack_dim = pack_dim

    def get_shards(self) -> List[torch.Tensor]:
        return [getattr(self, name) for name in self.bits_to_shard[self.bit_width]]

    def get_plain(self) -> torch.Tensor:
        return unpack(self.get_shards(), self.bit_width, dim=self.pack_dim)

    def __repr__(self):
        return f"Int{self.bit_width}Tensor(shape = {self.packed_shape}, data = {self.get_plain()})"

    def __tensor_flatten__(self):
        return self.bits_to_shard[self.bit_width], [self.packed_shape, self.bit_width,
                                                    self.pack_dim]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        packed_shape, bit_width, pack_dim = tensor_attributes
        return cls([tensor_data_dict[n] for n in cls.bits_to_shard[bit_width]], packed_shape,
                   bit_width, pack_dim)

    def _apply_fn_to_shards(self, fn):
        return type(self)([fn(s) for s in self.get_shards()], self.packed_shape, self.bit_width,
                          self.pack_dim)

    @classmethod
    def from_uint8(cls, int_data: torch.Tensor, dtype: torch.dtype, pack_dim: int = -1):
        assert dtype in _DTYPE_TO_BIT_WIDTH, (
            f"Expected dtype to be one of {list(_DTYPE_TO_BIT_WIDTH)}, got {dtype}"
        )
        bit_width = _DTYPE_TO_BIT_WIDTH[dtype]
        return cls(pack(int_data, bit_width, dim=pack_dim), int_data.shape, bit_width, pack_dim)

    def to(self, *args, **kwargs):
        device = self._get_to_kwargs(*args, **kwargs)["device"]
        return self._apply_fn_to_shards(lambda s: s.to(device))


@UintxTensor.implements([aten.detach.default, aten.alias.default])
def _(func, types, args, kwargs):
    return return_and_correct_aliasing(func, args, kwargs,
                                       args[0]._apply_fn_to_shards(torch.detach))


@UintxTensor.implements(aten.clone.default)
def _(func, types, args, kwargs):
    return return_and_correct_aliasing(func, args, kwargs,
                                       args[0]._apply_fn_to_shards(torch.clone))


@UintxTensor.implements(aten._to_copy.default)
def _(func, types, args, kwargs):
    device = kwargs.get("device", None)
    t = args[0] if device is None else args[0].to(device)
    return return_and_correct_aliasing(func, args, kwargs, t)


to_uintx = UintxTensor.from_uint8

torch.serialization.add_safe_globals([UintxTensor])


@dataclass(frozen=True)
class UintxLayout(Layout):
    """Codes of ``dtype`` (``torch.uint1`` .. ``torch.uint7``) bit-packed along ``pack_dim``."""

    dtype: torch.dtype
    pack_dim: int = -1

    def post_process(self, input: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor,
                     block_size: Tuple[int, ...]):
        return to_uintx(input, self.dtype, self.pack_dim), scale, zero_point


@register_layout(UintxLayout)
class UintxAQTTensorImpl(PlainAQTTensorImpl):
    """``int_data`` is a ``UintxTensor``; ``scale`` / ``zero_point`` are plain tensors."""

    def get_plain(self) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        return self.int_data.get_plain(), self.scale, self.zero_point

    @classmethod
    def from_plain(cls, int_data, scale, zero_point, _layout):
        assert isinstance(_layout, UintxLayout)
        return cls(int_data, scale, zero_point, _layout)

    def _hip_operands(self, block_size, zero_point_domain):
        """(s4, s2, s1, scale, zero_point, bit_width, group_size) where csrc/uintx.hip serves this
        weight, else None: shards on the GPU packed along the last dimension of a 2-D weight,
        bf16 scales and int32 zero points per (row, group), K % 128 == 0, group_size % 16 == 0
        (and, for a group size that is no power of two, K * group_size < 2^32)."""
        data = self.int_data
        if not (isinstance(data, UintxTensor) and data.is_cuda and data.dim() == 2
                and data.pack_dim in (-1, 1) and len(block_size) == 2 and block_size[0] == 1
                and zero_point_domain == ZeroPointDomain.INT and self.zero_point is not None
                and self.scale.dtype == torch.bfloat16 and self.zero_point.dtype == torch.int32):
            return None
        K, g = data.shape[1], block_size[1]
        if not (K % 128 == 0 and g % 16 == 0 and K % g == 0
                and ((g & (g - 1)) == 0 or K * g < 2**32)):
            return None
        return (getattr(data, "int4_shard", None), getattr(data, "int2_shard", None),
                getattr(data, "int1_shard", None), self.scale, self.zero_point, data.bit_width, g)

    def _dequantize_hip(self, block_size, zero_point_domain, output_dtype):
        """bf16(bf16(q - zp) * scale) by the HIP dequantizer (``torchao::uintx_dequantize``),
        bit-identical to unpack + ``dequantize_affine``; None where it does not serve."""
        ops = self._hip_operands(block_size, zero_point_domain)
        if ops is None or output_dtype != torch.bfloat16:
            return None
        return torch.ops.torchao.uintx_dequantize(*ops)


def _linear_bf16_act_uintx_weight_check(input_tensor, weight_tensor, bias) -> bool:
    return (
        not is_traceable_wrapper_subclass(input_tensor)
        and input_tensor.dtype == torch.bfloat16
        and input_tensor.is_cuda
        and isinstance(weight_tensor, AffineQuantizedTensor)
        and isinstance(weight_tensor._layout, UintxLayout)
        and weight_tensor.dtype == torch.bfloat16
        and weight_tensor.tensor_impl._hip_operands(
            weight_tensor.block_size, weight_tensor.zero_point_domain) is not None
    )


def _linear_bf16_act_uintx_weight_impl(input_tensor, weight_tensor, bias):
    """y = bf16(sum_k x (q - zp) s) (+ bias -> bf16), the shards read in place: the decode GEMV up
    to the measured boundary M, the HIP dequantizer + the bf16 matmul above."""
    s4, s2, s1, scale, zero_point, bits, g = weight_tensor.tensor_impl._hip_operands(
        weight_tensor.block_size, weight_tensor.zero_point_domain)
    return torch.ops.torchao.uintx_weight_only_linear(
        input_tensor, s4, s2, s1, scale, zero_point, bits, g, bias)
