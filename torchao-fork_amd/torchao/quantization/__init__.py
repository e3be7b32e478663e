"""Quantization workflows on the MI355X weight-only linear path."""

from torchao.quantization.fuse import fuse_gate_up_
from torchao.quantization.granularity import PerAxis, PerRow, PerTensor
from torchao.quantization.linear_activation_quantized_tensor import (
    LinearActivationQuantizedTensor,
    to_linear_activation_quantized,
)
from torchao.quantization.linear_activation_scale import (
    WeightTensorWithLinearActivationScaleMetadata,
    to_weight_tensor_with_linear_activation_scale_metadata,
)
from torchao.quantization.quant_api import (
    Float8DynamicActivationFloat8WeightConfig,
    Float8WeightOnlyConfig,
    FPXWeightOnlyConfig,
    Int4WeightOnlyConfig,
    Int8DynamicActivationInt4WeightConfig,
    Int8DynamicActivationInt8WeightConfig,
    Int8WeightOnlyConfig,
    ModuleFqnToConfig,
    float8_dynamic_activation_float8_weight,
    float8_weight_only,
    fpx_weight_only,
    int4_weight_only,
    int8_dynamic_activation_int4_weight,
    int8_dynamic_activation_int8_weight,
    int8_weight_only,
    quantize_,
)
from torchao.quantization.quant_primitives import (
    MappingType,
    ZeroPointDomain,
    choose_qparams_affine,
    dequantize_affine,
    quantize_affine,
)
from torchao.quantization.transform_module import register_quantize_module_handler
from torchao.quantization.utils import compute_error

__all__ = [
    "quantize_",
    "fuse_gate_up_",
    "Int4WeightOnlyConfig",
    "Int8WeightOnlyConfig",
    "Int8DynamicActivationInt8WeightConfig",
    "Int8DynamicActivationInt4WeightConfig",
    "Float8WeightOnlyConfig",
    "Float8DynamicActivationFloat8WeightConfig",
    "FPXWeightOnlyConfig",
    "fpx_weight_only",
    "PerAxis",
    "PerRow",
    "PerTensor",
    "ModuleFqnToConfig",
    "int4_weight_only",
    "int8_weight_only",
    "int8_dynamic_activation_int8_weight",
    "int8_dynamic_activation_int4_weight",
    "float8_weight_only",
    "float8_dynamic_activation_float8_weight",
    "LinearActivationQuantizedTensor",
    "to_linear_activation_quantized",
    "WeightTensorWithLinearActivationScaleMetadata",
    "to_weight_tensor_with_linear_activation_scale_metadata",
    "MappingType",
    "ZeroPointDomain",
    "choose_qparams_affine",
    "quantize_affine",
    "dequantize_affine",
    "register_quantize_module_handler",
    "compute_error",
]
