"""``AWQConfig`` and its ``quantize_`` handler (reference torchao/prototype/awq/api.py).

``quantize_(model, AWQConfig(base_config, step="prepare"))`` swaps in observed linears; run
calibration data through the model; ``step="convert"`` searches each observed linear's scale,
quantizes ``weight * scale`` with the base config's registered handler and wraps the result with
the scale (``WeightTensorWithLinearActivationScaleMetadata``). ``step="prepare_for_loading"`` gives
a float model the same structure without calibration, so a saved ``state_dict`` can be
``copy_``-ed or assigned in.

Served: weight-only base configs on 2-D linear weights (``Int4WeightOnlyConfig`` takes the fused
``int4_prescaled_linear`` path). 3-D (MoE) weights and activation-quantizing base configs raise
``NotImplementedError`` and leave the module untouched.
"""

import logging
import types
from dataclasses import dataclass

import torch

from torchao.core.config import AOBaseConfig
from torchao.quantization.linear_activation_scale import (
    to_weight_tensor_with_linear_activation_scale_metadata,
)
from torchao.quantization.quant_api import _linear_extra_repr
from torchao.quantization.transform_module import (
    _QUANTIZE_CONFIG_HANDLER,
    register_quantize_module_handler,
)
from torchao.utils import DummyModule

from .core import AWQObservedLinear, AWQObserver, AWQStep, check_awq_served

logger = logging.getLogger(__name__)

__all__ = ["AWQConfig"]


@dataclass
class AWQConfig(AOBaseConfig):
    """``base_config``: the weight-only config AWQ is applied on top of. ``step``: an ``AWQStep``
    or its string, in either case. ``scale_search_space_size``: the number of candidates."""

    base_config: AOBaseConfig
    step: AWQStep
    scale_search_space_size: int = 20

    def __post_init__(self):
        self.step = self.step.lower()
        all_step_values = [s.value for s in AWQStep]
        if self.step not in all_step_values:
            raise ValueError(f"{self.step} is not one of {all_step_values}")


@register_quantize_module_handler(AWQConfig)
def _awq_transform(module: torch.nn.Module, config: AWQConfig) -> torch.nn.Module:
    step = config.step
    base_config = config.base_config

    if step == AWQStep.CONVERT and not isinstance(module, AWQObservedLinear):
        logger.info(f"convert: module is not AWQObservedLinear, skipping: {type(module)}")
        return module
    check_awq_served(module.weight, base_config)  # before anything is changed

    if step == AWQStep.PREPARE:
        observer = AWQObserver(module.weight, module.bias, base_config,
                               config.scale_search_space_size)
        return AWQObservedLinear.from_float(module, observer)
    if step == AWQStep.PREPARE_FOR_LOADING:
        # the structure of a converted module; the loaded state_dict brings the real scale
        observed_linear = module
        equalization_scale = torch.ones(module.weight.shape[1], device=module.weight.device,
                                        dtype=module.weight.dtype)
    else:
        observed_linear = module
        equalization_scale = observed_linear.act_obs.calculate_qparams()

    base_config_handler = _QUANTIZE_CONFIG_HANDLER[type(base_config)]
    dummy_mod = DummyModule(observed_linear.weight * equalization_scale)
    qw = base_config_handler(dummy_mod, base_config).weight
    qw = to_weight_tensor_with_linear_activation_scale_metadata(qw, equalization_scale)

    linear = torch.nn.Linear(
        observed_linear.in_features,
        observed_linear.out_features,
        observed_linear.bias is not None,
        device=observed_linear.weight.device,
        dtype=observed_linear.weight.dtype,
    )
    linear.weight = torch.nn.Parameter(qw, requires_grad=False)
    linear.extra_repr = types.MethodType(_linear_extra_repr, linear)
    linear.bias = observed_linear.bias
    return linear
