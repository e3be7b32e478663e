"""Packed int4 layout (two codes per byte) and the int8-activation x int4-weight linear on MI355X.

Reference: torchao/dtypes/uintx/cutlass_int4_packed_layout.py. ``CutlassInt4PackedLayout`` /
``Int4PackedTensorImpl`` (:47-152) keep the reference's names, tensor attributes and bytes:
``int_data`` int8 ``[N, K/2]`` with element 2 j in the low nibble of byte j and element 2 j + 1 in
the high nibble (two's complement), ``scale`` float32 ``[N]``. A state dict the reference saved
for ``Int8DynamicActivationInt4WeightConfig(layout=CutlassInt4PackedLayout())`` therefore loads as
it is. Nothing is reordered in storage; the kernels pair the nibbles in flight (csrc/w4a8.hip).

The quantized-linear pair (:155-189) calls ``rowwise_scaled_linear_cutlass_s8s4`` as the reference
does. The reference builds that op as a CUTLASS kernel for sm80 only; here the same op name is
served by gfx950 HIP kernels (an int8 GEMV up to 2 tokens, or 4 on weights of at most 32 Mi
elements; ``v_mfma_i32_16x16x64_i8`` above). On CPU tensors, where the reference raises, the impl
evaluates the op's formula with plain torch ops:

    acc = Xq.to(int32) @ Wq.to(int32).T                       # exact
    y   = bf16( fp32(acc) * xs[m] * ws[n] + fp32(bias[n]) )   # fp32, one rounding

which is also the oracle of the GPU tests: every partial sum is an integer, so the GPU result
equals it bit for bit whatever the route.
"""

from dataclasses import dataclass
from typing import Optional

import torch
from torch.utils._python_dispatch import return_and_correct_aliasing

from torchao.dtypes.affine_quantized_tensor import AffineQuantizedTensor, register_layout
from torchao.dtypes.uintx.plain_layout import _aqt_is_int8
from torchao.dtypes.utils import AQTTensorImpl, Layout, PlainLayout

aten = torch.ops.aten

__all__ = ["CutlassInt4PackedLayout", "Int4PackedTensorImpl"]


def _aqt_is_int4(aqt) -> bool:
    return aqt.tensor_impl.dtype == torch.int8 and aqt.quant_min == -8 and aqt.quant_max == 7


def _same_metadata(self, src) -> bool:
    return (
        isinstance(self, Int4PackedTensorImpl)
        and isinstance(src, Int4PackedTensorImpl)
        and self.shape == src.shape
        and self.int_data.shape == src.int_data.shape
        and self.scale.shape == src.scale.shape
        and type(self._layout) is type(src._layout)
    )


@dataclass(frozen=True)
class CutlassInt4PackedLayout(Layout):
    """int4 codes packed two per byte with one float32 scale per row (reference :47-51)."""


@register_layout(CutlassInt4PackedLayout)
class Int4PackedTensorImpl(AQTTensorImpl):
    """``int_data`` (int8 ``[N, K/2]``, two int4 per byte) and ``scale`` (float32 ``[N]``)."""

    def __new__(cls, int_data, scale, _layout):
        return torch.Tensor._make_wrapper_subclass(
            cls,
            int_data.shape,
            device=int_data.device,
            layout=int_data.layout,
            dtype=int_data.dtype,
            requires_grad=False,
        )

    def __init__(self, int_data: torch.Tensor, scale: torch.Tensor, _layout: Layout):
        self.int_data = int_data
        self.scale = scale
        self._layout = _layout

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs):
        kwargs = {} if kwargs is None else kwargs
        if func is aten.detach.default:
            return return_and_correct_aliasing(
                func, args, kwargs, args[0]._apply_fn_to_data(torch.detach)
            )
        if func is aten.clone.default:
            return return_and_correct_aliasing(
                func, args, kwargs, args[0]._apply_fn_to_data(torch.clone)
            )
        if func is aten.copy_.default:
            dst, src = args[0], args[1]
            if _same_metadata(dst, src):
                for name in dst.__tensor_flatten__()[0]:
                    getattr(dst, name).copy_(getattr(src, name))
                return
            raise ValueError(f"Not supported args for copy_ due to metadata mismatch: {dst, src}")
        raise NotImplementedError(
            f"Int4PackedTensorImpl dispatch: attempting to run {func}, this is not supported"
        )

    __torch_function__ = torch._C._disabled_torch_function_impl

    def __tensor_flatten__(self):
        return ["int_data", "scale"], [self._layout]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        (_layout,) = tensor_attributes
        return cls(tensor_data_dict["int_data"], tensor_data_dict["scale"], _layout)

    def to(self, *args, **kwargs):
        device = self._get_to_kwargs(*args, **kwargs)["device"]
        return type(self)(self.int_data.to(device), self.scale.to(device), self._layout)

    def get_plain(self):
        """int8 codes ``[N, K]`` in [-8, 7], the scale, no zero point (reference :124-128)."""
        d = self.int_data
        int_data = torch.stack(((d << 4) >> 4, d >> 4), dim=-1).view(
            d.shape[:-1] + (2 * d.shape[-1],)
        )
        return int_data, self.scale, None

    @classmethod
    def from_plain(
        cls,
        int_data: torch.Tensor,
        scale: torch.Tensor,
        zero_point: Optional[torch.Tensor],
        _layout: Layout,
    ):
        assert zero_point is None or torch.all(zero_point == 0)
        packed = ((int_data[..., 1::2] & 0xF) << 4) | (int_data[..., 0::2] & 0xF)
        return cls(packed, scale, _layout)

    def get_layout(self) -> Layout:
        return self._layout

    def _apply_fn_to_data(self, fn):
        return type(self)(fn(self.int_data), fn(self.scale), self._layout)


def _w4a8_linear_formula(xq, xs, w_packed, ws, bias):
    """The op's arithmetic with plain torch ops on CPU tensors (the docstring's formula)."""
    wq = torch.stack(((w_packed << 4) >> 4, w_packed >> 4), dim=-1).view(w_packed.shape[0], -1)
    x2 = xq.reshape(-1, xq.shape[-1])
    acc = (x2.to(torch.int32) @ wq.to(torch.int32).t()).to(torch.float32)
    y = acc * xs.reshape(-1, 1).float() * ws.reshape(1, -1).float()
    if bias is not None:
        y = y + bias.float()
    return y.to(torch.bfloat16).reshape(*xq.shape[:-1], w_packed.shape[0])


def _linear_int8_act_int4_weight_cutlass_check(input_tensor, weight_tensor, bias):
    return (
        isinstance(input_tensor, AffineQuantizedTensor)
        and isinstance(input_tensor._layout, PlainLayout)
        and _aqt_is_int8(input_tensor)
        and input_tensor.dtype == torch.bfloat16
        and len(input_tensor.shape) >= 2
        and input_tensor.tensor_impl.scale.dtype == torch.float32
        and len(input_tensor.tensor_impl.scale.shape) == len(input_tensor.shape) - 1
        and isinstance(weight_tensor, AffineQuantizedTensor)
        and isinstance(weight_tensor._layout, CutlassInt4PackedLayout)
        and _aqt_is_int4(weight_tensor)
        and weight_tensor.dtype == input_tensor.dtype
        and len(weight_tensor.shape) == 2
        and weight_tensor.tensor_impl.scale.dtype == torch.float32
        and len(weight_tensor.tensor_impl.scale.shape) == 1
        and (bias is None or bias.dtype == input_tensor.dtype)
        and (bias is None or len(bias.shape) == 1)
    )


def _linear_int8_act_int4_weight_cutlass_impl(input_tensor, weight_tensor, bias):
    from torchao.ops import rowwise_scaled_linear_cutlass_s8s4

    weight = weight_tensor.tensor_impl.int_data
    weight_scale = weight_tensor.tensor_impl.scale
    input = input_tensor.tensor_impl.int_data
    input_scale = input_tensor.tensor_impl.scale
    if not input.is_cuda:
        return _w4a8_linear_formula(input, input_scale, weight, weight_scale, bias)
    return rowwise_scaled_linear_cutlass_s8s4(
        input, input_scale, weight, weight_scale, bias, input_tensor.dtype
    )
