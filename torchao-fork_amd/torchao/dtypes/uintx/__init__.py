from .cutlass_int4_packed_layout import CutlassInt4PackedLayout, Int4PackedTensorImpl
from .marlin_sparse_layout import MarlinSparseAQTTensorImpl, MarlinSparseLayout
from .plain_layout import PlainAQTTensorImpl
from .semi_sparse_layout import SemiSparseAQTTensorImpl, SemiSparseLayout
from .tensor_core_tiled_layout import TensorCoreTiledAQTTensorImpl, TensorCoreTiledLayout
from .uintx_layout import UintxAQTTensorImpl, UintxLayout, UintxTensor, to_uintx

__all__ = ["CutlassInt4PackedLayout", "Int4PackedTensorImpl", "MarlinSparseAQTTensorImpl",
           "MarlinSparseLayout", "PlainAQTTensorImpl",
           "SemiSparseAQTTensorImpl", "SemiSparseLayout", "TensorCoreTiledAQTTensorImpl",
           "TensorCoreTiledLayout", "UintxAQTTensorImpl",
           "UintxLayout", "UintxTensor", "to_uintx"]
