"""``quantize_`` and the weight-only / dynamic-int8 workflow configs.

Reference: torchao/quantization/quant_api.py — ``quantize_`` (:482-546) walks the module tree
(:173-222) and swaps the weight of every module ``filter_fn`` selects (default ``_is_linear``,
:271-288) for a quantized tensor subclass, using the transform registered for the config type.
Configs on the MI355X hot path, with the reference defaults:

* ``Int4WeightOnlyConfig`` (:997-1158): uint4 asymmetric per-group, float zero point,
  ``TensorCoreTiledLayout(inner_k_tiles=8)`` -> gfx950 int4 kernels;
* ``Int8WeightOnlyConfig`` (:1200-1255): int8 symmetric per-channel -> int8 GEMV / MFMA;
* ``Int8DynamicActivationInt8WeightConfig`` (:1352-1449): int8 per-channel weight + per-token
  reduced-range int8 activation quantized on the fly -> HIP quant kernel + int8 MFMA GEMM;
* ``Int8DynamicActivationInt4WeightConfig`` (:608-708) with ``CutlassInt4PackedLayout()`` and
  symmetric activations: int4 per-channel weight packed two per byte + per-token int8 activation,
  fp32 scales -> HIP quant kernels + int8 GEMV / MFMA (``rowwise_scaled_linear_cutlass_s8s4``);
  its other layouts raise;
* ``Float8WeightOnlyConfig`` (:1465-1530): e4m3fn symmetric per-channel, fp32 scales,
  ``Float8Layout`` -> fp8 GEMV / MFMA. Its ``version`` defaults to 1 here (the
  ``AffineQuantizedTensor`` form); the reference's default 2 (``Float8Tensor``) raises.

Other workflows of the reference (float8 dynamic activation, ``Float8Tensor``, HQQ, fbgemm
"version 2" tensors, marlin, gemlite, intx, QAT, ...) are out of scope and raise.
"""

import logging
import types
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn

import torchao
from torchao.core.config import AOBaseConfig
from torchao.dtypes.affine_quantized_tensor import (
    AffineQuantizedTensor,
    to_affine_quantized_floatx,
    to_affine_quantized_intx,
)
from torchao.dtypes.floatx.float8_layout import Float8Layout, Float8MMConfig
from torchao.dtypes.uintx.cutlass_int4_packed_layout import CutlassInt4PackedLayout
from torchao.dtypes.uintx.plain_layout import PlainAQTTensorImpl
from torchao.dtypes.uintx.tensor_core_tiled_layout import TensorCoreTiledLayout
from torchao.dtypes.utils import Layout, PlainLayout
from torchao.quantization.granularity import Granularity, PerRow, PerTensor
from torchao.quantization.linear_activation_quantized_tensor import (
    LinearActivationQuantizedTensor,
    to_linear_activation_quantized,
)
from torchao.quantization.quant_primitives import MappingType, ZeroPointDomain
from torchao.quantization.transform_module import (
    _QUANTIZE_CONFIG_HANDLER,
    register_quantize_module_handler,
)
from torchao.quantization.utils import _get_per_token_block_size

logger = logging.getLogger(__name__)

__all__ = [
    "quantize_",
    "Int4WeightOnlyConfig",
    "int4_weight_only",
    "Int8WeightOnlyConfig",
    "int8_weight_only",
    "Int8DynamicActivationInt8WeightConfig",
    "int8_dynamic_activation_int8_weight",
    "Int8DynamicActivationInt4WeightConfig",
    "int8_dynamic_activation_int4_weight",
    "Float8WeightOnlyConfig",
    "float8_weight_only",
    "FPXWeightOnlyConfig",
    "fpx_weight_only",
    "Float8DynamicActivationFloat8WeightConfig",
    "float8_dynamic_activation_float8_weight",
    "ModuleFqnToConfig",
    "LAYOUT_TO_ZERO_POINT_DOMAIN",
    "LAYOUT_TO_PRESERVE_ZEROS",
]

LAYOUT_TO_ZERO_POINT_DOMAIN = {TensorCoreTiledLayout: [ZeroPointDomain.FLOAT]}
LAYOUT_TO_PRESERVE_ZEROS = {TensorCoreTiledLayout: False}


# ---------------------------------------------------------------------------------------------
# module walking
# ---------------------------------------------------------------------------------------------
def _replace_with_custom_fn_if_matches_filter(
    model,
    replacement_fn,
    filter_fn,
    cur_fqn: str = "",
    device=None,
    extra_args: Optional[Tuple[Any, ...]] = (),
):
    """Depth-first: replace ``model`` itself if ``filter_fn(model, fqn)``, else recurse into
    its children (re-attaching replaced children). Moves modules to ``device`` first."""
    if filter_fn(model, cur_fqn[:-1]):
        if device is not None:
            model.to(device=device)
        return replacement_fn(model, *extra_args)
    for name, child in list(model.named_children()):
        new_child = _replace_with_custom_fn_if_matches_filter(
            child, replacement_fn, filter_fn, f"{cur_fqn}{name}.", device, extra_args
        )
        if new_child is not None and new_child is not child:
            setattr(model, name, new_child)
    if device is not None:
        model.to(device=device)
    return model


def _is_linear(mod, *args) -> bool:
    """An ``nn.Linear`` whose weight is not already quantized."""
    return (
        isinstance(mod, nn.Linear)
        and hasattr(mod, "weight")
        and not isinstance(mod.weight, (AffineQuantizedTensor, LinearActivationQuantizedTensor))
        and not isinstance(mod, nn.modules.linear.NonDynamicallyQuantizableLinear)
    )


def _quantization_type(weight: torch.Tensor) -> str:
    if isinstance(weight, AffineQuantizedTensor):
        return f"{type(weight).__name__}({weight._quantization_type()})"
    if isinstance(weight, LinearActivationQuantizedTensor):
        return (
            f"{type(weight).__name__}(activation={weight.input_quant_func}, "
            f"weight={_quantization_type(weight.original_weight_tensor)})"
        )
    if type(weight) is torch.Tensor or isinstance(weight, nn.Parameter):
        return f"Tensor: {type(weight)}"
    return f"not recognized: {type(weight)}"


def _linear_extra_repr(self):
    return (
        f"in_features={self.weight.shape[1]}, out_features={self.weight.shape[0]}, "
        f"weight={_quantization_type(self.weight)}"
    )


@dataclass
class ModuleFqnToConfig(AOBaseConfig):
    """Per-module configs by fully qualified name; ``"_default"`` applies to the rest."""

    module_fqn_to_config: Dict[str, Optional[AOBaseConfig]] = field(default_factory=dict)


def quantize_(
    model: nn.Module,
    config: AOBaseConfig,
    filter_fn: Optional[Callable[[nn.Module, str], bool]] = None,
    device: Optional[torch.types.Device] = None,
):
    """Quantize, in place, the weights of the modules of ``model`` that ``filter_fn`` selects.

    Example::

        m = nn.Sequential(nn.Linear(4096, 4096)).to(torch.bfloat16).cuda()
        quantize_(m, Int4WeightOnlyConfig(group_size=32))   # gfx950 int4 kernels
    """
    torch._C._log_api_usage_once("torchao.quantization.quantize_")
    filter_fn = _is_linear if filter_fn is None else filter_fn

    if isinstance(config, ModuleFqnToConfig):
        table = config.module_fqn_to_config

        def by_fqn(mod, fqn):
            cfg = table.get(fqn, table.get("_default", None))
            if cfg is None:
                return mod
            return _QUANTIZE_CONFIG_HANDLER[type(cfg)](mod, cfg)

        def walk(mod, prefix=""):
            for name, child in list(mod.named_children()):
                fqn = f"{prefix}{name}"
                if filter_fn(child, fqn):
                    if device is not None:
                        child.to(device=device)
                    setattr(mod, name, by_fqn(child, fqn))
                else:
                    walk(child, fqn + ".")

        walk(model)
        return

    if not isinstance(config, AOBaseConfig):
        raise AssertionError(
            "Passing a generic Callable to `quantize_` is not supported; pass a workflow config"
        )
    handler = _QUANTIZE_CONFIG_HANDLER[type(config)]
    # a handler may bring a precheck(module, config): what it refuses is raised for every
    # selected module before the first weight is swapped
    precheck = getattr(handler, "precheck", None)
    if precheck is not None:
        for fqn, mod in model.named_modules():
            if filter_fn(mod, fqn):
                precheck(mod, config)
    _replace_with_custom_fn_if_matches_filter(
        model, handler, filter_fn, device=device, extra_args=(config,)
    )


# ---------------------------------------------------------------------------------------------
# int4 weight-only
# ---------------------------------------------------------------------------------------------
@dataclass
class Int4WeightOnlyConfig(AOBaseConfig):
    """uint4 asymmetric per-group weight-only quantization for the tinygemm-equivalent kernels.

    Args mirror the reference (quant_api.py:997-1040): ``group_size`` in {32, 64, 128, 256}
    (default 128), ``layout`` (default ``TensorCoreTiledLayout(inner_k_tiles=8)``),
    ``use_hqq`` (half-quadratic quantization: the same scales, zero points moved by a proximal
    iteration, in fp32 on every device; a fused HIP quantizer on bf16 GPU weights),
    ``zero_point_domain`` (NONE = layout default, FLOAT),
    ``set_inductor_config``, ``preserve_zero`` (None = layout default, False), ``version``
    (1 = AffineQuantizedTensor; 2 = fbgemm tensors, unsupported).
    """

    group_size: int = 128
    layout: Optional[TensorCoreTiledLayout] = TensorCoreTiledLayout(inner_k_tiles=8)
    use_hqq: bool = False
    zero_point_domain: Optional[ZeroPointDomain] = ZeroPointDomain.NONE
    set_inductor_config: bool = True
    preserve_zero: Optional[bool] = None
    packing_format: str = "plain"
    version: int = 1

    def __post_init__(self):
        torch._C._log_api_usage_once("torchao.quantization.Int4WeightOnlyConfig")


int4_weight_only = Int4WeightOnlyConfig


def _int4_weight_only_quantize_tensor(weight: torch.Tensor, config: Int4WeightOnlyConfig):
    group_size = config.group_size
    layout = config.layout
    if weight.shape[-1] % group_size != 0:
        logger.info(
            f"Skipping quantizing weight with int4 weight only quantization because the shape "
            f"of weight {weight.shape} is not compatible with group_size {group_size}"
        )
        return weight
    if config.version != 1:
        raise NotImplementedError("Int4WeightOnlyConfig(version=2) (fbgemm tensors) is out of scope")
    assert type(layout) in LAYOUT_TO_ZERO_POINT_DOMAIN, (
        f"Only support layout: {list(LAYOUT_TO_ZERO_POINT_DOMAIN)}"
    )
    zero_point_domain = config.zero_point_domain
    if zero_point_domain == ZeroPointDomain.NONE:
        zero_point_domain = LAYOUT_TO_ZERO_POINT_DOMAIN[type(layout)][0]
    assert zero_point_domain in LAYOUT_TO_ZERO_POINT_DOMAIN[type(layout)], (
        f"Layout only support {LAYOUT_TO_ZERO_POINT_DOMAIN[type(layout)]}"
    )
    preserve_zero = (
        config.preserve_zero
        if config.preserve_zero is not None
        else LAYOUT_TO_PRESERVE_ZEROS[type(layout)]
    )
    block_size = tuple([1] * (weight.ndim - 1) + [group_size])
    return to_affine_quantized_intx(
        weight,
        MappingType.ASYMMETRIC,
        block_size,
        torch.int32,
        0,
        15,
        1e-6,
        zero_point_dtype=torch.bfloat16,
        preserve_zero=preserve_zero,
        zero_point_domain=zero_point_domain,
        _layout=layout,
        use_hqq=config.use_hqq,
    )


def _swap_weight(module: nn.Module, new_weight: torch.Tensor) -> nn.Module:
    module.weight = nn.Parameter(new_weight, requires_grad=False)
    module.extra_repr = types.MethodType(_linear_extra_repr, module)
    return module


@register_quantize_module_handler(Int4WeightOnlyConfig)
def _int4_weight_only_transform(module: nn.Module, config: Int4WeightOnlyConfig) -> nn.Module:
    if config.set_inductor_config:
        torchao.quantization.utils.recommended_inductor_config_setter()
    assert hasattr(module, "weight"), "int4 weight-only quant requires a module with a weight"
    return _swap_weight(module, _int4_weight_only_quantize_tensor(module.weight, config))


# ---------------------------------------------------------------------------------------------
# int8 weight-only
# ---------------------------------------------------------------------------------------------
@dataclass
class Int8WeightOnlyConfig(AOBaseConfig):
    """int8 symmetric weight-only quantization, per channel (``group_size=None``) or per group."""

    group_size: Optional[int] = None
    set_inductor_config: bool = True

    def __post_init__(self):
        torch._C._log_api_usage_once("torchao.quantization.Int8WeightOnlyConfig")


int8_weight_only = Int8WeightOnlyConfig


def _int8_weight_only_quantize_tensor(weight: torch.Tensor, config: Int8WeightOnlyConfig):
    group_size = weight.shape[-1] if config.group_size is None else config.group_size
    block_size = tuple([1] * (weight.dim() - 1) + [group_size])
    return to_affine_quantized_intx(
        weight,
        MappingType.SYMMETRIC,
        block_size,
        torch.int8,
        eps=torch.finfo(torch.float32).eps,
        zero_point_dtype=torch.int64,
    )


@register_quantize_module_handler(Int8WeightOnlyConfig)
def _int8_weight_only_transform(module: nn.Module, config: Int8WeightOnlyConfig) -> nn.Module:
    if config.set_inductor_config:
        torchao.quantization.utils.recommended_inductor_config_setter()
    assert hasattr(module, "weight"), "int8 weight-only quant requires a module with a weight"
    return _swap_weight(module, _int8_weight_only_quantize_tensor(module.weight, config))


# ---------------------------------------------------------------------------------------------
# int8 dynamic activation x int8 weight
# ---------------------------------------------------------------------------------------------
def _int8_symm_per_token_reduced_range_quant(x: torch.Tensor) -> torch.Tensor:
    """Per-token symmetric int8 in [-127, 127], eps 1e-5 (reference quant_api.py:1258-1273).

    bf16 activations on the GPU run the fused HIP kernel (``torchao::int8_quantize_per_token``,
    bit-identical to the torch-op formulation); anything else uses the torch ops.
    """
    if x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 16 == 0:
        q, s = torch.ops.torchao.int8_quantize_per_token(x)
        impl = PlainAQTTensorImpl(q, s, None, PlainLayout())
        return AffineQuantizedTensor(
            impl,
            tuple(_get_per_token_block_size(x)),
            x.shape,
            -127,
            127,
            ZeroPointDomain.INT,
            dtype=x.dtype,
        )
    return to_affine_quantized_intx(
        x,
        MappingType.SYMMETRIC,
        _get_per_token_block_size(x),
        torch.int8,
        eps=1e-5,
        quant_min=-127,
        quant_max=127,
        scale_dtype=torch.float32 if x.dtype == torch.float16 else None,
    )


def _int8_symm_per_token_reduced_range_quant_noop_decode(x: torch.Tensor) -> torch.Tensor:
    if x.dim() > 1 and x.shape[1] == 1:
        return x
    return _int8_symm_per_token_reduced_range_quant(x)


@dataclass
class Int8DynamicActivationInt8WeightConfig(AOBaseConfig):
    """int8 per-token dynamic activation x int8 per-channel weight (reference :1352-1372)."""

    layout: Optional[Layout] = PlainLayout()
    act_mapping_type: Optional[MappingType] = MappingType.SYMMETRIC
    weight_only_decode: bool = False
    set_inductor_config: bool = True

    def __post_init__(self):
        torch._C._log_api_usage_once("torchao.quantization.Int8DynamicActivationInt8WeightConfig")


int8_dynamic_activation_int8_weight = Int8DynamicActivationInt8WeightConfig


def _int8_dynamic_activation_int8_weight_quantize_tensor(weight, config):
    if weight.shape[-1] <= 16:
        logger.info(
            f"Skipping applying int8_dynamic_activation_int8_weight to weight of shape "
            f"{weight.shape} because `in_feature` is <= 16: {weight.shape[-1]}"
        )
        return weight
    if not isinstance(config.layout, PlainLayout):
        raise NotImplementedError("only PlainLayout is supported for int8 dynamic quantization")
    if config.act_mapping_type != MappingType.SYMMETRIC:
        raise NotImplementedError("asymmetric activation quantization is out of scope")
    input_quant_func = (
        _int8_symm_per_token_reduced_range_quant_noop_decode
        if config.weight_only_decode
        else _int8_symm_per_token_reduced_range_quant
    )
    block_size = tuple([1] * (weight.dim() - 1) + [weight.shape[-1]])
    new_weight = to_affine_quantized_intx(
        weight,
        MappingType.SYMMETRIC,
        block_size,
        torch.int8,
        eps=torch.finfo(torch.float32).eps,
        zero_point_dtype=torch.int64,
        _layout=config.layout,
        zero_point_domain=ZeroPointDomain.NONE,
    )
    return to_linear_activation_quantized(new_weight, input_quant_func)


@register_quantize_module_handler(Int8DynamicActivationInt8WeightConfig)
def _int8_dynamic_activation_int8_weight_transform(
    module: nn.Module, config: Int8DynamicActivationInt8WeightConfig
) -> nn.Module:
    if config.set_inductor_config:
        torchao.quantization.utils.recommended_inductor_config_setter()
    assert hasattr(module, "weight"), "int8 dynamic quant requires a module with a weight"
    return _swap_weight(
        module, _int8_dynamic_activation_int8_weight_quantize_tensor(module.weight, config)
    )


# ---------------------------------------------------------------------------------------------
# int8 dynamic activation x int4 weight (W4A8, CutlassInt4PackedLayout)
# ---------------------------------------------------------------------------------------------
def _int8_symm_cutlass_quant(x: torch.Tensor) -> torch.Tensor:
    """Per-token symmetric int8 in [-128, 127] with a float32 scale, eps = finfo(float32).eps and
    no zero point (reference quant_api.py:1299-1308). bf16 activations on the GPU take the fused
    HIP kernel inside ``to_affine_quantized_intx`` (``torchao::int8_quantize_per_token_f32``),
    bit-identical to the torch-op formulation."""
    return to_affine_quantized_intx(
        x,
        mapping_type=MappingType.SYMMETRIC,
        block_size=_get_per_token_block_size(x),
        target_dtype=torch.int8,
        scale_dtype=torch.float32,
        eps=torch.finfo(torch.float32).eps,
        zero_point_domain=ZeroPointDomain.NONE,
    )


def _int4_symm_cutlass_quant(x: torch.Tensor) -> torch.Tensor:
    """Per-row symmetric int4 in [-8, 7], float32 scale, packed two per byte
    (reference quant_api.py:1311-1323); bf16 GPU weights take ``torchao::int4_quantize_rows_packed``."""
    return to_affine_quantized_intx(
        x,
        mapping_type=MappingType.SYMMETRIC,
        block_size=_get_per_token_block_size(x),
        target_dtype=torch.int8,
        quant_min=-8,
        quant_max=7,
        scale_dtype=torch.float32,
        eps=torch.finfo(torch.float32).eps,
        zero_point_domain=ZeroPointDomain.NONE,
        _layout=CutlassInt4PackedLayout(),
    )


@dataclass
class Int8DynamicActivationInt4WeightConfig(AOBaseConfig):
    """int8 per-token dynamic activation x int4 weight (reference :608-632, same fields and
    defaults). Served here: ``layout=CutlassInt4PackedLayout()`` with symmetric activations and
    weights, i.e. ``Int8DynamicActivationInt4WeightConfig(layout=CutlassInt4PackedLayout(),
    act_mapping_type=MappingType.SYMMETRIC)``, on 2-D bf16 weights with K % 32 == 0. As in the
    reference, with that layout ``group_size`` only decides whether a linear is skipped
    (``K % group_size != 0``); the scale is per output channel."""

    group_size: int = 32
    layout: Layout = PlainLayout()
    mapping_type: MappingType = MappingType.SYMMETRIC
    act_mapping_type: MappingType = MappingType.ASYMMETRIC
    set_inductor_config: bool = True

    def __post_init__(self):
        torch._C._log_api_usage_once("torchao.quantization.Int8DynamicActivationInt4WeightConfig")


int8_dynamic_activation_int4_weight = Int8DynamicActivationInt4WeightConfig

_W4A8_SERVED = (
    "served: Int8DynamicActivationInt4WeightConfig(layout=CutlassInt4PackedLayout(), "
    "act_mapping_type=MappingType.SYMMETRIC, mapping_type=MappingType.SYMMETRIC) on 2-D bfloat16 "
    "weights whose in_features is a multiple of 32"
)


def _w4a8_skips(weight, config) -> bool:
    group_size = config.group_size
    if group_size is None or group_size == -1:
        group_size = weight.shape[-1]
    return weight.shape[-1] % group_size != 0


def _w4a8_precheck(module: nn.Module, config) -> None:
    """Everything this config refuses, raised before ``quantize_`` swaps any weight."""
    if not isinstance(config.layout, CutlassInt4PackedLayout):
        raise NotImplementedError(
            f"Int8DynamicActivationInt4WeightConfig with layout {config.layout!r} is not "
            f"implemented on MI355X (the default PlainLayout's forward is dequantize + F.linear in "
            f"the reference; MarlinQQQLayout and Int8DynamicActInt4WeightCPULayout are other "
            f"kernels); {_W4A8_SERVED}")
    if config.act_mapping_type != MappingType.SYMMETRIC:
        raise NotImplementedError(
            f"CutlassInt4PackedLayout takes symmetric activations, got act_mapping_type="
            f"{config.act_mapping_type}; {_W4A8_SERVED}")
    if config.mapping_type != MappingType.SYMMETRIC:
        raise NotImplementedError(
            f"CutlassInt4PackedLayout takes symmetric weights, got mapping_type="
            f"{config.mapping_type}; {_W4A8_SERVED}")
    weight = getattr(module, "weight", None)
    if weight is None or _w4a8_skips(weight, config):
        return
    if weight.dim() != 2 or weight.dtype != torch.bfloat16:
        raise NotImplementedError(
            f"weight of shape {tuple(weight.shape)} and dtype {weight.dtype}; {_W4A8_SERVED}")
    if weight.shape[-1] % 32 != 0:
        raise NotImplementedError(
            f"in_features {weight.shape[-1]} is not a multiple of 32; {_W4A8_SERVED}")


@register_quantize_module_handler(Int8DynamicActivationInt4WeightConfig)
def _int8_dynamic_activation_int4_weight_transform(
    module: nn.Module, config: Int8DynamicActivationInt4WeightConfig
) -> nn.Module:
    _w4a8_precheck(module, config)
    if config.set_inductor_config:
        torchao.quantization.utils.recommended_inductor_config_setter()
    weight = module.weight
    if _w4a8_skips(weight, config):
        return module
    new_weight = to_linear_activation_quantized(
        _int4_symm_cutlass_quant(weight), _int8_symm_cutlass_quant
    )
    return _swap_weight(module, new_weight)


# quantize_ runs this over every selected module before the first swap
_int8_dynamic_activation_int4_weight_transform.precheck = _w4a8_precheck


# ---------------------------------------------------------------------------------------------
# float8 weight-only
# ---------------------------------------------------------------------------------------------
@dataclass
class Float8WeightOnlyConfig(AOBaseConfig):
    """float8 (e4m3fn) symmetric per-channel weight-only quantization with fp32 scales
    (reference :1465-1530); the matmul runs in the activation's precision (bf16).

    Args: ``weight_dtype`` (only ``torch.float8_e4m3fn``; anything else raises
    ``NotImplementedError``), ``set_inductor_config``, ``version``.

    Deviation from the reference: ``version`` defaults to **1**, the ``AffineQuantizedTensor`` +
    ``Float8Layout`` form, so that ``Float8WeightOnlyConfig()`` works. The reference defaults
    to 2, its ``Float8Tensor``, which is out of scope here: ``version=2`` raises
    ``NotImplementedError``. Checkpoints the reference saved with ``version=1`` load as they are.
    """

    weight_dtype: torch.dtype = torch.float8_e4m3fn
    set_inductor_config: bool = True
    version: int = 1

    def __post_init__(self):
        torch._C._log_api_usage_once("torchao.quantization.Float8WeightOnlyConfig")


float8_weight_only = Float8WeightOnlyConfig


def _float8_weight_only_quant_tensor(weight: torch.Tensor, config: Float8WeightOnlyConfig):
    if config.version != 1:
        raise NotImplementedError(
            f"Float8WeightOnlyConfig(version={config.version}) (Float8Tensor) is out of scope; "
            "use version=1"
        )
    if config.weight_dtype != torch.float8_e4m3fn:
        raise NotImplementedError(
            f"Float8WeightOnlyConfig(weight_dtype={config.weight_dtype}) is out of scope; only "
            "torch.float8_e4m3fn is supported"
        )
    block_size = tuple([1] * (weight.dim() - 1) + [weight.shape[-1]])
    return to_affine_quantized_floatx(
        input_float=weight,
        block_size=block_size,
        target_dtype=config.weight_dtype,
        scale_dtype=None,
        _layout=Float8Layout(mm_config=None),
    )


@register_quantize_module_handler(Float8WeightOnlyConfig)
def _float8_weight_only_transform(module: nn.Module, config: Float8WeightOnlyConfig) -> nn.Module:
    if config.set_inductor_config:
        torchao.quantization.utils.recommended_inductor_config_setter()
    assert hasattr(module, "weight"), "float8 weight-only quant requires a module with a weight"
    return _swap_weight(module, _float8_weight_only_quant_tensor(module.weight, config))


# ---------------------------------------------------------------------------------------------
# FP6 (floatx) weight-only
# ---------------------------------------------------------------------------------------------
@dataclass
class FPXWeightOnlyConfig(AOBaseConfig):
    """Sub-byte floating point weight-only quantization, floatx(``ebits``, ``mbits``) with one
    scale per output channel in the weight's dtype (reference :2090-2141, same fields and
    defaults; the FP6-LLM recipe). Served here: the two FP6 formats, (3, 2) and (2, 3); any other
    pair (the reference's fp5 forms included) raises ``NotImplementedError`` before ``quantize_``
    touches a module. As in the reference, a linear whose ``in_features % 64 != 0`` or
    ``out_features % 256 != 0`` is left as it is."""

    ebits: int
    mbits: int
    set_inductor_config: bool = True

    def __post_init__(self):
        torch._C._log_api_usage_once("torchao.quantization.FPXWeightOnlyConfig")


fpx_weight_only = FPXWeightOnlyConfig


def _fpx_precheck(module: nn.Module, config: FPXWeightOnlyConfig) -> None:
    """What this config refuses, raised before ``quantize_`` swaps any weight."""
    if (config.ebits, config.mbits) not in ((3, 2), (2, 3)):
        raise NotImplementedError(
            f"FPXWeightOnlyConfig(ebits={config.ebits}, mbits={config.mbits}) is not implemented "
            f"on MI355X; served: the FP6 formats FPXWeightOnlyConfig(3, 2) (e3m2) and "
            f"FPXWeightOnlyConfig(2, 3) (e2m3)")


@register_quantize_module_handler(FPXWeightOnlyConfig)
def _fpx_weight_only_transform(module: nn.Module, config: FPXWeightOnlyConfig) -> nn.Module:
    _fpx_precheck(module, config)
    ebits, mbits = config.ebits, config.mbits
    weight = module.weight
    if config.set_inductor_config:
        torchao.quantization.utils.recommended_inductor_config_setter()
    from torchao.dtypes import to_affine_quantized_fpx
    from torchao.dtypes.floatx import FloatxTensorCoreLayout

    assert weight.dim() == 2, f"floatx only works for 2-d Tensor, got: {weight.dim()}"
    out_dim, in_dim = weight.shape
    if (in_dim % 64 != 0) or (out_dim % 256 != 0):
        logger.info(
            f"Skipping floatx quantization float{ebits + mbits + 1}_{ebits}_{mbits} because "
            f"the shape is not compatible with the kernel: in_dim={in_dim}, out_dim={out_dim} "
            "expected in_dim % 64 == 0 and out_dim % 256 == 0"
        )
        return module
    new_weight = to_affine_quantized_fpx(weight, FloatxTensorCoreLayout(ebits, mbits))
    return _swap_weight(module, new_weight)


# quantize_ runs this over every selected module before the first swap
_fpx_weight_only_transform.precheck = _fpx_precheck


# ---------------------------------------------------------------------------------------------
# float8 dynamic activation x float8 weight
# ---------------------------------------------------------------------------------------------
_FP8_DYN_SUPPORTED = (
    "supported: granularity=PerRow() for both operands, torch.float8_e4m3fn activations and "
    "weights, version=1 (AffineQuantizedTensor + Float8Layout), no activation value bounds"
)


def _normalize_granularity(granularity) -> Tuple[Granularity, Granularity]:
    """``None`` -> per-tensor for both (the reference's default), one granularity -> both, a pair
    -> (activation, weight), which must be of one kind."""
    if granularity is None:
        return PerTensor(), PerTensor()
    if isinstance(granularity, (PerTensor, PerRow)):
        return granularity, granularity
    if isinstance(granularity, (tuple, list)) and len(granularity) == 2:
        act, weight = granularity
        if not all(isinstance(g, (PerTensor, PerRow)) for g in (act, weight)):
            raise ValueError(f"Invalid granularity types: {granularity}, only PerTensor or PerRow")
        if type(act) is not type(weight):
            raise ValueError(
                f"Different granularities for activation and weight are not supported: {granularity}"
            )
        return act, weight
    raise ValueError(f"Invalid granularity specification: {granularity}, only PerTensor or PerRow")


def _per_row_block_size(shape) -> Tuple[int, ...]:
    return (1,) * (len(shape) - 1) + (shape[-1],)


def _input_activation_quant_func_fp8(
    x: torch.Tensor,
    activation_granularity: Granularity,
    activation_dtype: torch.dtype,
    scale: Optional[torch.Tensor] = None,
    zero_point: Optional[torch.Tensor] = None,
):
    """Dynamic per-row float8 quantization of a linear's input (reference quant_api.py:1533-1571):
    an ``AffineQuantizedTensor`` with ``Float8Layout(mm_config=None)`` and block size
    (1, ..., K). bf16 activations on the GPU run the fused HIP quantizer
    (``torchao::fp8_quantize_rows``, rows = tokens) inside ``to_affine_quantized_floatx``."""
    assert zero_point is None, "Zero point is not supported for dynamic FP8 quantization"
    if not isinstance(activation_granularity, PerRow) or scale is not None:
        raise NotImplementedError(
            f"float8 activation quantization with {activation_granularity} / a static scale is "
            f"out of scope; {_FP8_DYN_SUPPORTED}"
        )
    assert x.dtype == torch.bfloat16, (
        "PerRow quantization only works for bfloat16 precision input activation"
    )
    return to_affine_quantized_floatx(
        input_float=x,
        block_size=_per_row_block_size(x.shape),
        target_dtype=activation_dtype,
        scale_dtype=torch.float32,
        _layout=Float8Layout(mm_config=None),  # the mm config is stored on the weight
    )


def _fp8_mm_compat(weight: torch.Tensor) -> bool:
    """Both weight dimensions multiples of 16, as the reference's scaled mm requires
    (quant_api.py:1574-1598); an incompatible weight is left unquantized and logged."""
    assert weight.dim() in (2, 3), (
        f"float8 quantization only works for 2/3-D tensors, got {weight.dim()}D tensor"
    )
    out_dim, in_dim = weight.shape[-2:]
    ok = in_dim % 16 == 0 and out_dim % 16 == 0
    if not ok:
        logger.info(
            f"Skipping float8 quantization: weight shape {weight.shape} is not compatible with "
            f"the scaled mm. Both input dimension ({in_dim}) and output dimension ({out_dim}) "
            "must be multiples of 16."
        )
    return ok


@dataclass
class Float8DynamicActivationFloat8WeightConfig(AOBaseConfig):
    """float8 (e4m3fn) dynamic per-row activation x float8 per-row weight (reference
    :1601-1738): the activation is quantized per token on every call, the product runs on the
    fp8 matrix cores (``torchao::fp8_scaled_mm``) and both fp32 scales are applied in the epilogue.

    Fields are the reference's, in its order, without ``kernel_preference`` (this package has
    one kernel). In scope: ``granularity=PerRow()`` (or a pair of them), e4m3fn for both operands,
    ``version=1``. Everything else raises ``NotImplementedError`` when the config is applied:
    ``PerTensor`` (which ``granularity=None`` means, as in the reference), ``version=2``
    (``Float8Tensor``), e5m2 and ``activation_value_lb`` / ``activation_value_ub``.

    Deviation from the reference: ``version`` defaults to **1**, for the reason given at
    ``Float8WeightOnlyConfig``. The working spelling is
    ``Float8DynamicActivationFloat8WeightConfig(granularity=PerRow())``.
    """

    activation_dtype: torch.dtype = torch.float8_e4m3fn
    weight_dtype: torch.dtype = torch.float8_e4m3fn
    granularity: Optional[Union[Granularity, List[Granularity]]] = None
    mm_config: Optional[Float8MMConfig] = None
    activation_value_lb: Optional[float] = None
    activation_value_ub: Optional[float] = None
    set_inductor_config: bool = True
    version: int = 1

    def __post_init__(self):
        torch._C._log_api_usage_once(
            "torchao.quantization.Float8DynamicActivationFloat8WeightConfig"
        )
        if self.mm_config is None:
            self.mm_config = Float8MMConfig(use_fast_accum=True)
        self.granularity = list(_normalize_granularity(self.granularity))


float8_dynamic_activation_float8_weight = Float8DynamicActivationFloat8WeightConfig


def _float8_dynamic_activation_float8_weight_quantize_tensor(weight, config):
    activation_granularity, weight_granularity = config.granularity
    refused = None
    if config.version != 1:
        refused = f"version={config.version} (Float8Tensor)"
    elif not (isinstance(activation_granularity, PerRow) and isinstance(weight_granularity, PerRow)):
        refused = f"granularity={config.granularity}"
    elif config.activation_dtype != torch.float8_e4m3fn:
        refused = f"activation_dtype={config.activation_dtype}"
    elif config.weight_dtype != torch.float8_e4m3fn:
        refused = f"weight_dtype={config.weight_dtype}"
    elif config.activation_value_lb is not None or config.activation_value_ub is not None:
        refused = "activation_value_lb / activation_value_ub"
    if refused is not None:
        raise NotImplementedError(
            f"Float8DynamicActivationFloat8WeightConfig({refused}) is out of scope; "
            f"{_FP8_DYN_SUPPORTED}"
        )
    if not _fp8_mm_compat(weight):
        return weight
    assert weight.dtype == torch.bfloat16, (
        "PerRow quantization only works for bfloat16 precision input weight"
    )
    quantized_weight = to_affine_quantized_floatx(
        input_float=weight,
        block_size=_per_row_block_size(weight.shape),
        target_dtype=config.weight_dtype,
        scale_dtype=torch.float32,
        _layout=Float8Layout(mm_config=config.mm_config),
    )
    return to_linear_activation_quantized(
        quantized_weight,
        _input_activation_quant_func_fp8,
        quant_kwargs={
            "activation_granularity": activation_granularity,
            "activation_dtype": config.activation_dtype,
        },
    )


@register_quantize_module_handler(Float8DynamicActivationFloat8WeightConfig)
def _float8_dynamic_activation_float8_weight_transform(
    module: nn.Module, config: Float8DynamicActivationFloat8WeightConfig
) -> nn.Module:
    assert hasattr(module, "weight"), (
        "applying float8 dynamic activation quant requires module to have weight attribute"
    )
    # refusals and the bf16 requirement are raised before anything is touched
    new_weight = _float8_dynamic_activation_float8_weight_quantize_tensor(module.weight, config)
    if config.set_inductor_config:
        torchao.quantization.utils.recommended_inductor_config_setter()
    if new_weight is module.weight:
        return module  # _fp8_mm_compat: left as it is
    return _swap_weight(module, new_weight)


torch.serialization.add_safe_globals([_input_activation_quant_func_fp8, Float8MMConfig])
torch.serialization.add_safe_globals([_int8_symm_cutlass_quant, _int4_symm_cutlass_quant])
