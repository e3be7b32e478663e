"""``WeightTensorWithLinearActivationQuantizationMetadata`` — static activation quantization
wrapper (SmoothQuant's static mode).

Reference: torchao/quantization/weight_tensor_linear_activation_quantization.py:21-204. The wrapper
holds an (already quantized) weight, a calibrated activation ``scale`` (and ``zero_point``) and
``input_quant_func_static(x, scale=..., zero_point=..., **quant_kwargs)``; on ``F.linear`` the
activation goes through that function and the pair dispatches again on the inner weight. Module
path, class name and attribute names are the reference's.

Under a ``WeightTensorWithLinearActivationScaleMetadata`` with SmoothQuant's ``_ActQuantizer`` the
outer wrapper takes the fused route (``torch.ops.torchao.int8_smooth_static_linear``,
linear_activation_scale.py) and this class's ``F.linear`` is not reached; reached on its own it
runs the reference's steps, each inner op keeping its own rules.
"""

from typing import Any, Callable, Dict, Optional

import torch
from torch.utils._python_dispatch import return_and_correct_aliasing

from torchao.utils import TorchAOBaseTensor

__all__ = [
    "WeightTensorWithLinearActivationQuantizationMetadata",
    "to_weight_tensor_with_linear_activation_quantization_metadata",
]

aten = torch.ops.aten


class WeightTensorWithLinearActivationQuantizationMetadata(TorchAOBaseTensor):
    """Weight wrapper that quantizes the linear's input with fixed, calibrated qparams."""

    original_weight_tensor: torch.Tensor
    input_quant_func_static: Callable
    scale: torch.Tensor
    zero_point: Optional[torch.Tensor]
    quant_kwargs: Dict[str, Any]

    def __new__(cls, original_weight_tensor, input_quant_func_static, scale, zero_point,
                quant_kwargs):
        return torch.Tensor._make_wrapper_subclass(
            cls,
            original_weight_tensor.shape,
            dtype=original_weight_tensor.dtype,
            device=original_weight_tensor.device,
            requires_grad=False,
        )

    def __init__(
        self,
        original_weight_tensor: torch.Tensor,
        input_quant_func_static: Callable,
        scale: torch.Tensor,
        zero_point: Optional[torch.Tensor],
        quant_kwargs: Dict[str, Any],
    ):
        self.original_weight_tensor = original_weight_tensor
        self.input_quant_func_static = input_quant_func_static
        self.scale = scale
        self.zero_point = zero_point
        self.quant_kwargs = quant_kwargs

    def __repr__(self):
        return (
            f"{type(self).__name__}({self.original_weight_tensor}, "
            f"{self.input_quant_func_static}, scale={self.scale}, zero_point={self.zero_point}, "
            f"quant_kwargs={self.quant_kwargs})"
        )

    def __tensor_flatten__(self):
        tensor_data = ["original_weight_tensor", "scale"]
        if self.zero_point is not None:
            tensor_data.append("zero_point")
        return tensor_data, [self.input_quant_func_static, self.quant_kwargs]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        input_quant_func_static, quant_kwargs = tensor_attributes
        return cls(
            tensor_data_dict["original_weight_tensor"],
            input_quant_func_static,
            tensor_data_dict["scale"],
            tensor_data_dict.get("zero_point", None),
            quant_kwargs,
        )

    @staticmethod
    def _quantized_linear_op(input_tensor, weight_tensor, bias):
        qx = weight_tensor.input_quant_func_static(
            input_tensor, scale=weight_tensor.scale, zero_point=weight_tensor.zero_point,
            **weight_tensor.quant_kwargs)
        return torch.nn.functional.linear(qx, weight_tensor.original_weight_tensor, bias)

    @classmethod
    def from_float(
        cls,
        input_float: torch.Tensor,
        input_quant_func: Callable,
        scale: torch.Tensor,
        zero_point: Optional[torch.Tensor] = None,
        quant_kwargs: Optional[Dict[str, Any]] = None,
    ):
        return cls(input_float, input_quant_func, scale, zero_point,
                   {} if quant_kwargs is None else quant_kwargs)

    def _apply_fn_to_data(self, fn):
        return type(self)(
            fn(self.original_weight_tensor),
            self.input_quant_func_static,
            fn(self.scale),
            fn(self.zero_point) if self.zero_point is not None else None,
            self.quant_kwargs,
        )

    def to(self, *args, **kwargs):
        # as the reference: the device moves, the dtypes stay (an int64 zero point stays int64)
        device = self._get_to_kwargs(*args, **kwargs).pop("device")
        return type(self)(
            self.original_weight_tensor.to(device),
            self.input_quant_func_static,
            self.scale.to(device),
            self.zero_point.to(device) if self.zero_point is not None else None,
            self.quant_kwargs,
        )


implements = WeightTensorWithLinearActivationQuantizationMetadata.implements


@implements([torch.nn.functional.linear, aten.linear.default])
def _(func, types, args, kwargs):
    input_tensor, weight_tensor = args[0], args[1]
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    if isinstance(weight_tensor, WeightTensorWithLinearActivationQuantizationMetadata):
        return weight_tensor._quantized_linear_op(input_tensor, weight_tensor, bias)
    raise NotImplementedError(
        "WeightTensorWithLinearActivationQuantizationMetadata: No specialized dispatch found for "
        "linear op"
    )


@implements(aten.detach.default)
def _(func, types, args, kwargs):
    return return_and_correct_aliasing(func, args, kwargs, args[0]._apply_fn_to_data(torch.detach))


@implements(aten.clone.default)
def _(func, types, args, kwargs):
    return return_and_correct_aliasing(func, args, kwargs, args[0]._apply_fn_to_data(torch.clone))


@implements(aten._to_copy.default)
def _(func, types, args, kwargs):
    return return_and_correct_aliasing(
        func, args, kwargs, args[0].to(*args[1:], **kwargs)._apply_fn_to_data(torch.clone)
    )


@implements(aten.t.default)
def _(func, types, args, kwargs):
    # as the reference, torch.t reaches the qparams too (a 0-d or 1-d scale is its own transpose)
    return return_and_correct_aliasing(func, args, kwargs, args[0]._apply_fn_to_data(torch.t))


to_weight_tensor_with_linear_activation_quantization_metadata = (
    WeightTensorWithLinearActivationQuantizationMetadata.from_float
)

# a state_dict with these weights names this class when it is unpickled
torch.serialization.add_safe_globals([WeightTensorWithLinearActivationQuantizationMetadata])
