"""Quantization granularities of the float8 configs and of the min/max observers.

Reference: torchao/quantization/granularity.py. Only the two granularities the float8 dynamic
config names and the ``PerAxis`` of torchao.quantization.observer (SmoothQuant) are defined; class
paths and field sets are the reference's, so a
``quant_kwargs`` dict it pickled (``{"activation_granularity": PerRow(), ...}``) loads here with
``torch.load(weights_only=True)``.
"""

from dataclasses import dataclass

import torch

__all__ = ["Granularity", "PerTensor", "PerRow", "PerAxis"]


@dataclass(frozen=True)
class Granularity:
    """Base class of the granularity markers."""


@dataclass(frozen=True)
class PerTensor(Granularity):
    """One scale for the whole tensor."""


class PerRow(Granularity):
    """One scale per row: block size (1, ..., 1, shape[-1]), for activations and weights alike."""


@dataclass(frozen=True)
class PerAxis(Granularity):
    """One scale per index along ``axis`` (the observers of torchao.quantization.observer)."""

    axis: int


torch.serialization.add_safe_globals([Granularity, PerTensor, PerRow, PerAxis])
