from .float8_layout import Float8AQTTensorImpl, Float8Layout, Float8MMConfig
from .floatx_tensor_core_layout import (
    FloatxTensorCoreAQTTensorImpl,
    FloatxTensorCoreLayout,
    convert_from_floatx_tensor_core,
    convert_to_floatx_tensor_core,
)

__all__ = [
    "Float8AQTTensorImpl",
    "Float8Layout",
    "Float8MMConfig",
    "FloatxTensorCoreAQTTensorImpl",
    "FloatxTensorCoreLayout",
    "convert_from_floatx_tensor_core",
    "convert_to_floatx_tensor_core",
]
