"""Activation-aware weight quantization (reference torchao/prototype/awq)."""

from .api import AWQConfig
from .core import AWQObservedLinear, AWQObserver, AWQStep

__all__ = ["AWQConfig", "AWQObservedLinear", "AWQObserver", "AWQStep"]
