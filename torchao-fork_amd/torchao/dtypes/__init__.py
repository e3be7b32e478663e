"""Quantized tensor subclasses and layouts of the MI355X weight-only linear path."""

from . import affine_quantized_tensor_ops  # noqa: F401  (registers the op overrides)
from .affine_quantized_tensor import (
    AffineQuantizedTensor,
    register_layout,
    to_affine_quantized_floatx,
    to_affine_quantized_fpx,
    to_affine_quantized_intx,
    to_affine_quantized_intx_static,
)
from .affine_quantized_tensor_ops import (
    QuantizedLinearNotImplementedError,
    deregister_aqt_quantized_linear_dispatch,
    register_aqt_quantized_linear_dispatch,
)
from .nf4tensor import NF4Tensor, to_nf4
from .floatx import (
    Float8AQTTensorImpl,
    Float8Layout,
    Float8MMConfig,
    FloatxTensorCoreAQTTensorImpl,
    FloatxTensorCoreLayout,
)
from .uintx import (
    CutlassInt4PackedLayout,
    Int4PackedTensorImpl,
    PlainAQTTensorImpl,
    TensorCoreTiledAQTTensorImpl,
    TensorCoreTiledLayout,
)
from .utils import AQTTensorImpl, Layout, PlainLayout

__all__ = [
    "AffineQuantizedTensor",
    "AQTTensorImpl",
    "Layout",
    "PlainLayout",
    "PlainAQTTensorImpl",
    "TensorCoreTiledLayout",
    "TensorCoreTiledAQTTensorImpl",
    "CutlassInt4PackedLayout",
    "Int4PackedTensorImpl",
    "Float8Layout",
    "Float8AQTTensorImpl",
    "Float8MMConfig",
    "QuantizedLinearNotImplementedError",
    "register_aqt_quantized_linear_dispatch",
    "deregister_aqt_quantized_linear_dispatch",
    "register_layout",
    "FloatxTensorCoreLayout",
    "FloatxTensorCoreAQTTensorImpl",
    "to_affine_quantized_floatx",
    "to_affine_quantized_fpx",
    "to_affine_quantized_intx",
    "to_affine_quantized_intx_static",
    "NF4Tensor",
    "to_nf4",
]
