"""``WeightTensorWithLinearActivationScaleMetadata`` — a weight with a per-input-channel
activation scale (AWQ, SmoothQuant).

Reference: torchao/quantization/linear_activation_scale.py:19-120. The wrapper holds an (already
quantized) weight and a ``scale`` of K elements; on ``F.linear`` the activation is divided by the
scale and the pair dispatches again on the inner weight (:61-70). Module path, class name and the
tensor attribute names (``original_weight_tensor``, ``scale``) are the reference's, so a
``state_dict`` it saved unpickles into this class (``torch.load(weights_only=True)``).

What changes is which kernels run:

* inner weight a 2-D int4 ``TensorCoreTiledLayout`` AQT on the GPU, bf16 input and scale:
  ``torch.ops.torchao.int4_prescaled_linear`` (one token: the division happens while the GEMV
  stages x in LDS, one launch; more tokens: ``act_prescale`` then the int4 linear);
* any other inner weight: ``torch.ops.torchao.act_prescale`` for bf16 GPU operands (plain
  ``x / scale`` otherwise), then ``F.linear`` on the inner weight, which keeps its own rules
  (including raising on the CPU).
"""

import torch
from torch.utils._python_dispatch import return_and_correct_aliasing

from torchao.utils import TorchAOBaseTensor

__all__ = [
    "WeightTensorWithLinearActivationScaleMetadata",
    "to_weight_tensor_with_linear_activation_scale_metadata",
]

aten = torch.ops.aten


def _is_plain_bf16_gpu(t) -> bool:
    return type(t) in (torch.Tensor, torch.nn.Parameter) and t.is_cuda and t.dtype == torch.bfloat16


def _prescale(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    if (_is_plain_bf16_gpu(x) and _is_plain_bf16_gpu(scale) and x.dim() >= 1
            and scale.numel() == x.shape[-1] and scale.numel() % 8 == 0):
        return torch.ops.torchao.act_prescale(x, scale)
    return x / scale


class WeightTensorWithLinearActivationScaleMetadata(TorchAOBaseTensor):
    """Weight wrapper that divides the linear's input by ``scale`` (one value per input channel)."""

    tensor_data_names = ["original_weight_tensor", "scale"]
    tensor_attribute_names = []

    def __new__(cls, original_weight_tensor: torch.Tensor, scale: torch.Tensor):
        return torch.Tensor._make_wrapper_subclass(
            cls,
            original_weight_tensor.shape,
            dtype=original_weight_tensor.dtype,
            device=original_weight_tensor.device,
            requires_grad=False,
        )

    def __init__(self, original_weight_tensor: torch.Tensor, scale: torch.Tensor):
        self.original_weight_tensor = original_weight_tensor
        self.scale = scale

    def __repr__(self):
        return (f"{type(self).__name__}({self.original_weight_tensor}, "
                f"scale={self.scale})")

    def _quantization_type(self):
        return f"{self.__class__}"

    def __tensor_flatten__(self):
        return list(self.tensor_data_names), []

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        return cls(tensor_data_dict["original_weight_tensor"], tensor_data_dict["scale"])

    @staticmethod
    def _quantized_linear_op(input_tensor, weight_tensor, bias):
        from torchao.dtypes.uintx.tensor_core_tiled_layout import (
            _linear_bf16_act_uint4_weight_check,
        )

        w = weight_tensor.original_weight_tensor
        scale = weight_tensor.scale
        if (_is_plain_bf16_gpu(input_tensor) and _is_plain_bf16_gpu(scale)
                and input_tensor.numel() > 0
                and _linear_bf16_act_uint4_weight_check(input_tensor, w, bias)
                and w.tensor_impl.packed_weight.is_cuda
                and input_tensor.shape[-1] == w.shape[1] == scale.numel()):
            impl = w.tensor_impl
            return torch.ops.torchao.int4_prescaled_linear(
                input_tensor, scale, impl.packed_weight, impl.scale_and_zero, w.block_size[-1],
                bias)
        return torch.nn.functional.linear(_prescale(input_tensor, scale), w, bias)

    @classmethod
    def from_float(cls, input_float: torch.Tensor, scale: torch.Tensor):
        return cls(input_float, scale)

    def _apply_fn_to_data(self, fn):
        return type(self)(fn(self.original_weight_tensor), fn(self.scale))

    def to(self, *args, **kwargs):
        kwargs = self._get_to_kwargs(*args, **kwargs)
        return type(self)(self.original_weight_tensor.to(**kwargs), self.scale.to(**kwargs))


implements = WeightTensorWithLinearActivationScaleMetadata.implements


@implements([torch.nn.functional.linear, aten.linear.default])
def _(func, types, args, kwargs):
    input_tensor, weight_tensor = args[0], args[1]
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    if isinstance(weight_tensor, WeightTensorWithLinearActivationScaleMetadata):
        return weight_tensor._quantized_linear_op(input_tensor, weight_tensor, bias)
    raise NotImplementedError(
        "WeightTensorWithLinearActivationScaleMetadata: No specialized dispatch found for linear op"
    )


@implements([aten.detach.default, aten.alias.default])
def _(func, types, args, kwargs):
    return return_and_correct_aliasing(func, args, kwargs, args[0]._apply_fn_to_data(func))


@implements(aten.clone.default)
def _(func, types, args, kwargs):
    return return_and_correct_aliasing(func, args, kwargs, args[0]._apply_fn_to_data(torch.clone))


@implements(aten._to_copy.default)
def _(func, types, args, kwargs):
    return return_and_correct_aliasing(
        func, args, kwargs, args[0].to(*args[1:], **kwargs)._apply_fn_to_data(torch.clone)
    )


@implements(aten.copy_.default)
def _(func, types, args, kwargs):
    dst, src = args[0], args[1]
    if (
        isinstance(dst, WeightTensorWithLinearActivationScaleMetadata)
        and isinstance(src, WeightTensorWithLinearActivationScaleMetadata)
        and dst.shape == src.shape
        and dst.scale.shape == src.scale.shape
    ):
        dst.original_weight_tensor.copy_(src.original_weight_tensor)
        dst.scale.copy_(src.scale)
        return dst
    raise ValueError(f"Not supported args for copy_ due to metadata mismatch: {dst, src}")


@implements(aten.slice.Tensor)
def _(func, types, args, kwargs):
    # the reference keeps the whole scale whichever dimension is sliced (:99-105)
    self = args[0]
    new = type(self)(func(self.original_weight_tensor, *args[1:], **kwargs), self.scale)
    return return_and_correct_aliasing(func, args, kwargs, new)


@implements(aten.t.default)
def _(func, types, args, kwargs):
    self = args[0]
    new = type(self)(torch.t(self.original_weight_tensor), self.scale)
    return return_and_correct_aliasing(func, args, kwargs, new)


to_weight_tensor_with_linear_activation_scale_metadata = (
    WeightTensorWithLinearActivationScaleMetadata.from_float
)

# a state_dict with these weights loads with torch.load(weights_only=True)
torch.serialization.add_safe_globals([WeightTensorWithLinearActivationScaleMetadata])
