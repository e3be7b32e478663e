"""2:4 semi-structured sparse layout of an int8 weight (reference
torchao/dtypes/uintx/semi_sparse_layout.py), for ``Int8DynamicActivationInt8WeightConfig(
layout=SemiSparseLayout())``.

The reference keeps the weight in cuSPARSELt's opaque compressed form (``torch._cslt_compress``)
and multiplies with ``torch._cslt_sparse_mm``; a ROCm build of torch has neither. Here the storage
is documented (csrc/sparse24.hip, DESIGN.md "2:4 sparse int8"):

* ``values`` int8 [N, K/2]: the two kept elements of every group of four dense k;
* ``meta`` int32 [N, K/32]: sixteen 2-bit positions per dword,

0.625 B per dense weight, the operand layout of gfx950's sparse MFMA. The linear runs
``torch.ops.torchao.int8_sp24_scaled_mm`` (``int8_sp24_dyn_linear`` for one token), whose output
equals the dense ``int8_scaled_mm`` on the decompressed weight bit for bit; the reference's sparse
impl rounds after the weight scale first.
"""

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch.utils._python_dispatch import return_and_correct_aliasing

from torchao.dtypes.affine_quantized_tensor import AffineQuantizedTensor, register_layout
from torchao.dtypes.uintx.plain_layout import (
    PlainLayout,
    _aqt_is_int8,
    _aqt_is_int8_reduced_range,
)
from torchao.dtypes.utils import AQTTensorImpl, Layout

aten = torch.ops.aten

__all__ = ["SemiSparseLayout", "SemiSparseAQTTensorImpl"]


@dataclass(frozen=True)
class SemiSparseLayout(Layout):
    """``pre_process`` prunes the weight 2:4: the two smallest magnitudes of every four
    consecutive input features become zero. Of equal magnitudes the lower index is pruned first
    (the reference's ``argsort`` leaves ties unspecified)."""

    def pre_process(self, input: torch.Tensor) -> torch.Tensor:
        if input.dim() != 2 or input.shape[-1] % 4 != 0:
            raise NotImplementedError(
                f"SemiSparseLayout serves 2-D weights with K % 4 == 0, got {tuple(input.shape)}"
            )
        g = input.detach().reshape(-1, 4)
        # stable ascending sort of |w|: the first two of each group are pruned
        pruned = g.abs().float().argsort(dim=1, stable=True)[:, :2]
        return g.clone().scatter_(1, pruned, 0).reshape(input.shape)


@register_layout(SemiSparseLayout)
class SemiSparseAQTTensorImpl(AQTTensorImpl):
    """``values`` / ``meta`` of the compressed int8 weight plus its per-row ``scale``."""

    def __new__(cls, values, meta, scale, zero_point, _layout):
        return torch.Tensor._make_wrapper_subclass(
            cls,
            (values.shape[0], values.shape[1] * 2),
            device=values.device,
            layout=values.layout,
            dtype=values.dtype,
            requires_grad=False,
        )

    def __init__(
        self,
        values: torch.Tensor,
        meta: torch.Tensor,
        scale: torch.Tensor,
        zero_point: Optional[torch.Tensor],
        _layout: Layout,
    ):
        self.values = values
        self.meta = meta
        self.scale = scale
        self.zero_point = zero_point
        self._layout = _layout

    def __tensor_flatten__(self):
        names = ["values", "meta", "scale"] + ([] if self.zero_point is None else ["zero_point"])
        return names, [self._layout]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        (layout,) = tensor_attributes
        return cls(
            tensor_data_dict["values"],
            tensor_data_dict["meta"],
            tensor_data_dict["scale"],
            tensor_data_dict.get("zero_point", None),
            layout,
        )

    def _apply_fn_to_data(self, fn):
        return type(self)(
            fn(self.values),
            fn(self.meta),
            fn(self.scale),
            None if self.zero_point is None else fn(self.zero_point),
            self._layout,
        )

    def to(self, *args, **kwargs):
        device = self._get_to_kwargs(*args, **kwargs)["device"]
        return self._apply_fn_to_data(lambda t: t.to(device))

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
            if (
                isinstance(src, cls)
                and dst.shape == src.shape
                and dst.scale.shape == src.scale.shape
                and (dst.zero_point is None) == (src.zero_point is None)
            ):
                for name in dst.__tensor_flatten__()[0]:
                    getattr(dst, name).copy_(getattr(src, name))
                return
            raise ValueError(f"Not supported args for copy_ due to metadata mismatch: {dst, src}")
        raise NotImplementedError(f"SemiSparseAQTTensorImpl dispatch: {func} is not supported")

    __torch_function__ = torch._C._disabled_torch_function_impl

    def get_plain(self) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        int_data = torch.ops.torchao.int8_sp24_decompress(self.values, self.meta)
        return int_data, self.scale, self.zero_point

    def get_layout(self) -> Layout:
        return self._layout

    @classmethod
    def from_plain(cls, int_data, scale, zero_point, _layout):
        assert isinstance(_layout, SemiSparseLayout)
        if int_data.dim() != 2 or int_data.dtype != torch.int8 or int_data.shape[1] % 128 != 0:
            raise NotImplementedError(
                "SemiSparseLayout serves 2-D int8 weights with K % 128 == 0, got "
                f"{int_data.dtype} {tuple(int_data.shape)}"
            )
        values, meta, err = torch.ops.torchao.int8_sp24_compress(int_data.contiguous())
        if int(err.item()) != 0:  # a host sync, at quantization time only
            raise ValueError(
                "SemiSparseLayout: the weight is not 2:4 sparse (a group of four input features "
                "holds more than two nonzeros)"
            )
        return cls(values, meta, scale, zero_point, _layout)


def _linear_int8_act_int8_sp24_weight_check(input_tensor, weight_tensor, bias) -> bool:
    return (
        isinstance(input_tensor, AffineQuantizedTensor)
        and _aqt_is_int8_reduced_range(input_tensor)
        and isinstance(weight_tensor, AffineQuantizedTensor)
        and _aqt_is_int8(weight_tensor)
        and input_tensor.dtype == weight_tensor.dtype
        and input_tensor.dtype == torch.bfloat16
        and isinstance(input_tensor._layout, PlainLayout)
        and isinstance(weight_tensor._layout, SemiSparseLayout)
    )


def _linear_int8_act_int8_sp24_weight_impl(input_tensor, weight_tensor, bias):
    """The plain impl's formula, y = bf16(bf16(float(xq @ wq^T) * s_x) * s_w) (+ bias), on the
    compressed weight."""
    x_impl = input_tensor.tensor_impl
    w_impl = weight_tensor.tensor_impl
    y = torch.ops.torchao.int8_sp24_scaled_mm(
        x_impl.int_data,
        x_impl.scale,
        w_impl.values,
        w_impl.meta,
        w_impl.scale.reshape(-1),
        bias,
    )
    return y.to(input_tensor.dtype)
