"""``MoEQuantConfig`` and its module handler (reference torchao/prototype/moe_quant/utils.py).

``quantize_(model, MoEQuantConfig(Int4WeightOnlyConfig(group_size=32)), cond_ffn_filter)``
quantizes the 3-D expert weights ``w1`` / ``w2`` / ``w3`` of every
``ConditionalFeedForwardAOQuantizable`` through the base config's own handler, run on a
``DummyModule`` per weight (as the AWQ convert does).

Served base configs: ``Int4WeightOnlyConfig`` (the grouped gfx950 kernels), ``Int8WeightOnlyConfig``
and ``Float8WeightOnlyConfig`` (a per-expert loop on the existing linears): the three whose
3-D ``AffineQuantizedTensor`` this tree packs, indexes and selects. The reference's
``FakeExtraDimTensor`` (a list of 2-D quantized tensors posing as a 3-D one) is not served:
``UseFakeExtraDimTensor.TRUE``, any other base config, and ``AS_FALLBACK`` when the base handler
raises, all raise ``NotImplementedError`` before any parameter of any module is replaced.
"""

import enum
from dataclasses import dataclass

import torch

import torchao.quantization.utils
from torchao.core.config import AOBaseConfig
from torchao.quantization.quant_api import (
    Float8WeightOnlyConfig,
    Int4WeightOnlyConfig,
    Int8WeightOnlyConfig,
)
from torchao.quantization.transform_module import (
    _QUANTIZE_CONFIG_HANDLER,
    register_quantize_module_handler,
)
from torchao.utils import DummyModule

__all__ = ["MoEQuantConfig", "UseFakeExtraDimTensor", "moe_filter", "cond_ffn_filter",
           "moe_quant_fn"]

_SERVED_BASE_CONFIGS = (Int4WeightOnlyConfig, Int8WeightOnlyConfig, Float8WeightOnlyConfig)
_SERVED = ("served: Int4WeightOnlyConfig, Int8WeightOnlyConfig and Float8WeightOnlyConfig as "
           "3-D AffineQuantizedTensor weights (UseFakeExtraDimTensor.FALSE or AS_FALLBACK)")
_WEIGHTS = ("w1", "w2", "w3")


class UseFakeExtraDimTensor(enum.Enum):
    """Whether to hold the experts as a FakeExtraDimTensor (reference enum; here only the values
    that never need one are served)."""

    TRUE = enum.auto()
    FALSE = enum.auto()
    AS_FALLBACK = enum.auto()


@dataclass
class MoEQuantConfig(AOBaseConfig):
    """Quantize the 3-D expert weights of an MoE feed-forward with ``base_config``."""

    base_config: AOBaseConfig
    use_fake_extra_dim_tensor: UseFakeExtraDimTensor = UseFakeExtraDimTensor.AS_FALLBACK
    set_inductor_config: bool = True


def _quantize_expert_weight(weight: torch.Tensor, config: MoEQuantConfig) -> torch.Tensor:
    handler = _QUANTIZE_CONFIG_HANDLER[type(config.base_config)]
    try:
        return handler(DummyModule(weight), config.base_config).weight
    except Exception as e:
        if config.use_fake_extra_dim_tensor is UseFakeExtraDimTensor.AS_FALLBACK:
            raise NotImplementedError(
                f"MoEQuantConfig: {type(config.base_config).__name__} raised on a 3-D expert "
                f"weight ({type(e).__name__}: {e}) and the FakeExtraDimTensor fallback is not "
                f"served; {_SERVED}") from e
        raise


def _moe_quant_precheck(module: torch.nn.Module, config: MoEQuantConfig) -> None:
    """Everything the handler refuses, raised for every selected module before the first weight is
    swapped (quantize_ runs it over the whole model first). The base handler is tried on one
    expert's slice of each weight: what it refuses depends on its config and on the weight's last
    two dimensions, which the slice keeps."""
    base = config.base_config
    if not isinstance(base, AOBaseConfig):
        raise TypeError(
            f"MoEQuantConfig expects an AOBaseConfig instance as base_config, got {base!r} "
            "(MoEQuantConfig(SomeConfig) instead of MoEQuantConfig(SomeConfig())?)")
    if config.use_fake_extra_dim_tensor is UseFakeExtraDimTensor.TRUE:
        raise NotImplementedError(
            f"MoEQuantConfig(use_fake_extra_dim_tensor=TRUE): FakeExtraDimTensor is not served; "
            f"{_SERVED}")
    if not isinstance(base, _SERVED_BASE_CONFIGS):
        raise NotImplementedError(
            f"MoEQuantConfig(base_config={type(base).__name__}) is not served; {_SERVED}")
    for name in _WEIGHTS:
        param = getattr(module, name, None)
        if not isinstance(param, torch.Tensor) or param.dim() != 3:
            raise ValueError(
                f"MoEQuantConfig: expected a 3-D tensor for {name} of {type(module).__name__}, got "
                f"{None if param is None else tuple(param.shape)}")
    for name in _WEIGHTS:
        _quantize_expert_weight(getattr(module, name).detach()[:1], config)


@register_quantize_module_handler(MoEQuantConfig)
def moe_quant_fn(module: torch.nn.Module, config: MoEQuantConfig) -> torch.nn.Module:
    _moe_quant_precheck(module, config)
    if config.set_inductor_config:
        torchao.quantization.utils.recommended_inductor_config_setter()
    # all three quantized before the first is assigned: a raise leaves the module as it was
    new = {name: _quantize_expert_weight(getattr(module, name).detach(), config)
           for name in _WEIGHTS}
    for name, w in new.items():
        setattr(module, name, torch.nn.Parameter(w, requires_grad=False))
    return module


moe_quant_fn.precheck = _moe_quant_precheck


def moe_filter(module: torch.nn.Module, fqn: str) -> bool:
    return "MOEFeedForwardAOQuantizable" in str(type(module))


def cond_ffn_filter(module: torch.nn.Module, fqn: str) -> bool:
    return "ConditionalFeedForwardAOQuantizable" in str(type(module))
