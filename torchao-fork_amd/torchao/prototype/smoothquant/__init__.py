"""SmoothQuant (reference torchao/prototype/smoothquant) over the int8 dynamic / static linear."""

from .api import (
    SmoothQuantConfig,
    _ActQuantizer,
    insert_smooth_quant_observer_,
    load_smooth_quant_recipe,
    save_smooth_quant_recipe,
)
from .core import SmoothQuantObservedLinear, SmoothQuantObserver

__all__ = [
    "insert_smooth_quant_observer_",
    "load_smooth_quant_recipe",
    "save_smooth_quant_recipe",
    "SmoothQuantConfig",
    "SmoothQuantObservedLinear",
    "SmoothQuantObserver",
]
