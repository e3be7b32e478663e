"""Quantization granularities of the float8 configs.

Reference: torchao/quantization/granularity.py. Only the two granularities the float8 dynamic
config names are defined; class paths and (empty) field sets are the reference's, so a
``quant_kwargs`` dict it pickled (``{"activation_granularity": PerRow(), ...}``) loads here with
``torch.load(weights_only=True)``.
"""

from dataclasses import dataclass

import torch

__all__ = ["Granularity", "PerTensor", "PerRow"]


@dataclass(frozen=True)
class Granularity:
    """Base class of the granularity markers."""


@dataclass(frozen=True)
class PerTensor(Granularity):
    """One scale for the whole tensor."""


class PerRow(Granularity):
    """One scale per row: block size (1, ..., 1, shape[-1]), for activations and weights alike."""


torch.serialization.add_safe_globals([Granularity, PerTensor, PerRow])
