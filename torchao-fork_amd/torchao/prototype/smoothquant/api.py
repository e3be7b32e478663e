"""SmoothQuant's user surface (reference torchao/prototype/smoothquant/api.py).

``insert_smooth_quant_observer_(model, alpha, quant_mode)`` swaps observed linears in; run
calibration data through the model; ``quantize_(model, SmoothQuantConfig(), is_observed_linear)``
converts each into a linear whose weight is, from the outside in,

1. ``WeightTensorWithLinearActivationScaleMetadata`` holding the smoothing factor in the weight's
   dtype,
2. ``LinearActivationQuantizedTensor`` over ``_ActQuantizer(int8).dynamic_quantize`` (dynamic), or
   ``WeightTensorWithLinearActivationQuantizationMetadata`` over ``.static_quantize`` with the
   calibrated scale (static),
3. an int8 ``PlainLayout`` AQT of ``weight * factor`` under the observer's per-channel scales.

Convert is plain torch and works on CPU and GPU modules. On the GPU with bf16 input the outermost
wrapper's ``F.linear`` runs ``torch.ops.torchao.int8_smooth_dyn_linear`` /
``int8_smooth_static_linear`` (linear_activation_scale.py). ``save_smooth_quant_recipe`` /
``load_smooth_quant_recipe`` write and apply the reference's recipe file: a dict of
``<fqn>.smoothing_factor``, ``<fqn>.act_scales`` (None for dynamic) and ``<fqn>.wei_scales``.

Refused with ``NotImplementedError`` before a module is touched: 3-D weights, in_features that is
no multiple of 16, and non-bf16 modules on the GPU (core.check_smoothquant_served).
"""

import types
from dataclasses import dataclass
from typing import Dict, Optional

import torch

import torchao
from torchao.core.config import AOBaseConfig
from torchao.dtypes import to_affine_quantized_intx, to_affine_quantized_intx_static
from torchao.quantization.linear_activation_quantized_tensor import to_linear_activation_quantized
from torchao.quantization.linear_activation_scale import (
    to_weight_tensor_with_linear_activation_scale_metadata,
)
from torchao.quantization.quant_api import (
    _linear_extra_repr,
    _replace_with_custom_fn_if_matches_filter,
    quantize_,
)
from torchao.quantization.quant_primitives import MappingType
from torchao.quantization.transform_module import register_quantize_module_handler
from torchao.quantization.utils import _get_per_token_block_size
from torchao.quantization.weight_tensor_linear_activation_quantization import (
    to_weight_tensor_with_linear_activation_quantization_metadata,
)

from .core import SmoothQuantObservedLinear, SmoothQuantObserver, check_smoothquant_served

__all__ = [
    "insert_smooth_quant_observer_",
    "save_smooth_quant_recipe",
    "load_smooth_quant_recipe",
    "SmoothQuantConfig",
]


def insert_smooth_quant_observer_(model: torch.nn.Module, alpha: Optional[float] = 0.5,
                                  quant_mode: str = "dynamic"):
    """Replace, in place, every ``nn.Linear`` of ``model`` by a ``SmoothQuantObservedLinear``.
    ``alpha`` None gives a factor of ones; ``quant_mode`` is "dynamic" or "static". Calibrate on
    the device the model is on."""
    def is_linear(m, fqn):
        return isinstance(m, torch.nn.Linear)

    for m in model.modules():  # every linear is checked before the first is replaced
        if is_linear(m, ""):
            check_smoothquant_served(m.weight)

    quant_min, quant_max = -127, 127
    eps = torch.finfo(torch.float32).eps

    def replace_with_observer(layer):
        observer = SmoothQuantObserver(layer.weight, alpha, quant_mode, quant_min=quant_min,
                                       quant_max=quant_max, eps=eps)
        return SmoothQuantObservedLinear.from_float(layer, observer)

    _replace_with_custom_fn_if_matches_filter(model, replace_with_observer, is_linear)


def _named_observed_linears(module: torch.nn.Module, name: str = ""):
    for child_name, child in module.named_children():
        full_name = f"{name}.{child_name}" if name else child_name
        if isinstance(child, SmoothQuantObservedLinear):
            yield full_name, child
        yield from _named_observed_linears(child, full_name)


def save_smooth_quant_recipe(model: torch.nn.Module, save_path: str) -> None:
    """``torch.save`` the qparams of every calibrated ``SmoothQuantObservedLinear`` below
    ``model`` as ``{fqn.smoothing_factor, fqn.act_scales, fqn.wei_scales}``."""
    result: Dict[str, Optional[torch.Tensor]] = {}
    for name, child in _named_observed_linears(model):
        smoothing_factor, act_scales, wei_scales = child.obs.calculate_qparams()
        result[name + ".smoothing_factor"] = smoothing_factor
        result[name + ".act_scales"] = act_scales
        result[name + ".wei_scales"] = wei_scales
    torch.save(result, save_path)


def load_smooth_quant_recipe(model: torch.nn.Module, recipe_path: str, device=None) -> None:
    """Convert, in place, the observed linears below ``model`` that ``recipe_path`` has qparams
    for (moved to ``device`` first, if given); the others stay observed."""
    recipe = torch.load(recipe_path, weights_only=True)

    def in_recipe(m, fqn):
        return (isinstance(m, SmoothQuantObservedLinear)
                and recipe.get(fqn + ".smoothing_factor") is not None
                and recipe.get(fqn + ".wei_scales") is not None)

    for parent_name, parent in list(model.named_modules()):
        for child_name, child in list(parent.named_children()):
            fqn = f"{parent_name}.{child_name}" if parent_name else child_name
            if not isinstance(child, SmoothQuantObservedLinear):
                continue
            if device is not None:
                child.to(device=device)
            if not in_recipe(child, fqn):
                continue
            dev = child.weight.device
            act_scales = recipe.get(fqn + ".act_scales")  # None for dynamic quantization
            config = SmoothQuantConfig(
                recipe[fqn + ".smoothing_factor"].to(dev),
                None if act_scales is None else act_scales.to(dev),
                recipe[fqn + ".wei_scales"].to(dev),
            )
            wrapper = torch.nn.Sequential(child)
            quantize_(wrapper, config, lambda m, _: isinstance(m, SmoothQuantObservedLinear))
            setattr(parent, child_name, wrapper[0])


class _ActQuantizer:
    """SmoothQuant's activation quantizers, as bound methods so the target dtype travels with
    them. Plain torch; the GPU route recognises them and does not call them."""

    def __init__(self, target_dtype, quant_min=-127):
        self.target_dtype = target_dtype
        self.quant_min = quant_min

    def dynamic_quantize(self, input):
        # no eps: choose_qparams_affine clamps the scale at torch.finfo(input.dtype).eps
        return to_affine_quantized_intx(
            input, MappingType.SYMMETRIC, _get_per_token_block_size(input), self.target_dtype,
            self.quant_min)

    def static_quantize(self, input, scale, zero_point):
        return to_affine_quantized_intx_static(
            input, scale, zero_point, list(input.shape), self.target_dtype, self.quant_min)


@dataclass
class SmoothQuantConfig(AOBaseConfig):
    """``smoothing_factor``, ``act_scales``, ``wei_scales``: a layer's qparams (a recipe's), taken
    from the layer's observer when the factor or the weight scales are None; ``act_scales`` None
    means dynamic activation quantization. ``set_inductor_config``: apply the recommended
    torchinductor settings."""

    smoothing_factor: Optional[torch.Tensor] = None
    act_scales: Optional[torch.Tensor] = None
    wei_scales: Optional[torch.Tensor] = None
    set_inductor_config: bool = True


@register_quantize_module_handler(SmoothQuantConfig)
def _smooth_quant_transform(module: torch.nn.Module, config: SmoothQuantConfig):
    observed_linear = module
    check_smoothquant_served(observed_linear.weight)  # before anything is changed
    from_observer = config.smoothing_factor is None or config.wei_scales is None
    if from_observer and not isinstance(observed_linear, SmoothQuantObservedLinear):
        raise ValueError(
            "SmoothQuantConfig without smoothing_factor and wei_scales converts a "
            f"SmoothQuantObservedLinear (insert_smooth_quant_observer_), got {type(module)}")
    if config.set_inductor_config:
        torchao.quantization.utils.recommended_inductor_config_setter()

    if from_observer:
        factor, x_scale, w_scales = observed_linear.obs.calculate_qparams()
        weight = observed_linear.obs.weight * factor
    else:
        factor, x_scale, w_scales = config.smoothing_factor, config.act_scales, config.wei_scales
        weight = observed_linear.weight * factor
    weight = weight.to(observed_linear.weight.dtype)

    target_dtype = torch.int8
    qw = to_affine_quantized_intx_static(
        weight, w_scales, torch.zeros_like(w_scales, dtype=torch.int64), (1, weight.size(1)),
        target_dtype)
    if x_scale is None:
        qw = to_linear_activation_quantized(qw, _ActQuantizer(target_dtype).dynamic_quantize)
    else:
        qw = to_weight_tensor_with_linear_activation_quantization_metadata(
            qw, _ActQuantizer(target_dtype).static_quantize, x_scale,
            torch.zeros_like(x_scale, dtype=torch.int64))
    qw = to_weight_tensor_with_linear_activation_scale_metadata(qw, factor.to(qw.dtype))

    linear = torch.nn.Linear(
        observed_linear.in_features,
        observed_linear.out_features,
        observed_linear.bias is not None,
        device=observed_linear.weight.device,
        dtype=observed_linear.weight.dtype,
    )
    linear.bias = observed_linear.bias
    linear.weight = torch.nn.Parameter(qw, requires_grad=False)
    linear.extra_repr = types.MethodType(_linear_extra_repr, linear)
    return linear
