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
* inner weight SmoothQuant's dynamic or static int8 wrapper (``_smoothquant_int8_linear``), bf16
  input and factor on the GPU: ``torch.ops.torchao.int8_smooth_dyn_linear`` /
  ``int8_smooth_static_linear`` (one token up to K = 16384, static 8192: division, activation quantization and
  int8 GEMV in one launch; otherwise the fused smooth + quantize kernel, then the int8 GEMV / MFMA);
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


def _smoothquant_int8_linear(x, factor, inner, bias):
    """SmoothQuant's converted weight (prototype/smoothquant/api.py) with bf16 GPU input and
    factor: ``inner`` is a ``LinearActivationQuantizedTensor`` over
    ``_ActQuantizer(torch.int8, -127).dynamic_quantize``, or the static wrapper over
    ``.static_quantize`` with one bf16 scale and a zero (or no) zero point, around a 2-D int8
    ``PlainLayout`` AQT with a bf16 per-channel scale. Then the division, the activation
    quantization and the int8 linear are ``torch.ops.torchao.int8_smooth_dyn_linear`` /
    ``int8_smooth_static_linear``, bit-identical to the reference's steps. Anything else returns
    None and takes the generic path."""
    from torchao.dtypes.affine_quantized_tensor import AffineQuantizedTensor
    from torchao.dtypes.uintx.plain_layout import PlainLayout, _aqt_is_int8
    from torchao.prototype.smoothquant.api import _ActQuantizer
    from torchao.quantization.linear_activation_quantized_tensor import (
        LinearActivationQuantizedTensor,
    )
    from torchao.quantization.weight_tensor_linear_activation_quantization import (
        WeightTensorWithLinearActivationQuantizationMetadata,
    )

    if not (_is_plain_bf16_gpu(x) and _is_plain_bf16_gpu(factor) and x.numel() > 0):
        return None
    act_scale = None
    if isinstance(inner, LinearActivationQuantizedTensor):
        fn, method = inner.input_quant_func, _ActQuantizer.dynamic_quantize
    elif isinstance(inner, WeightTensorWithLinearActivationQuantizationMetadata):
        fn, method = inner.input_quant_func_static, _ActQuantizer.static_quantize
        act_scale = inner.scale
        if not (_is_plain_bf16_gpu(act_scale) and act_scale.numel() == 1):
            return None
        if inner.zero_point is not None:
            # read back once per wrapper object, not per call (a device-to-host copy)
            if not hasattr(inner, "_zero_point_is_zero"):
                inner._zero_point_is_zero = not bool(inner.zero_point.any())
            if not inner._zero_point_is_zero:
                return None
    else:
        return None
    quantizer = getattr(fn, "__self__", None)
    if not (getattr(fn, "__func__", None) is method and type(quantizer) is _ActQuantizer
            and quantizer.target_dtype == torch.int8 and quantizer.quant_min == -127
            and not inner.quant_kwargs):
        return None
    w = inner.original_weight_tensor
    K = x.shape[-1]
    if not (isinstance(w, AffineQuantizedTensor) and _aqt_is_int8(w) and w.dtype == torch.bfloat16
            and isinstance(w._layout, PlainLayout) and len(w.shape) == 2
            and w.shape[1] == K == factor.numel() and K % 16 == 0 and K <= 65536):
        return None
    impl = w.tensor_impl
    # (the weight's zero point is not read: _linear_int8_act_int8_weight_impl does not use it)
    if not (impl.int_data.is_cuda and impl.scale.dtype == torch.bfloat16
            and impl.scale.numel() == w.shape[0]):
        return None
    if act_scale is None:
        return torch.ops.torchao.int8_smooth_dyn_linear(
            x, factor, impl.int_data, impl.scale.reshape(-1), bias)
    return torch.ops.torchao.int8_smooth_static_linear(
        x, factor, act_scale, impl.int_data, impl.scale.reshape(-1), bias)


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
        y = _smoothquant_int8_linear(input_tensor, scale, w, bias)
        if y is not None:
            return y
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
