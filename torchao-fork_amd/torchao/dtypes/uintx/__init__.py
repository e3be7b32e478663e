from .cutlass_int4_packed_layout import CutlassInt4PackedLayout, Int4PackedTensorImpl
from .plain_layout import PlainAQTTensorImpl
from .tensor_core_tiled_layout import TensorCoreTiledAQTTensorImpl, TensorCoreTiledLayout

__all__ = ["CutlassInt4PackedLayout", "Int4PackedTensorImpl", "PlainAQTTensorImpl",
           "TensorCoreTiledAQTTensorImpl", "TensorCoreTiledLayout"]
