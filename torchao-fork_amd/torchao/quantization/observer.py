"""Min/max observer for affine quantization: the part of the reference's
torchao/quantization/observer.py that SmoothQuant's calibration needs.

``AffineQuantizedMinMaxObserver`` keeps the running per-block ``min_val`` / ``max_val`` of what it
has seen (attribute names and dtypes the reference's, observer.py:144-193) and turns them into
qparams with ``choose_qparams_affine_with_min_max``. min and max are exact, so the statistics are
the same on whichever device the observed tensors live; nothing is moved.

Granularities: ``PerTensor``, ``PerAxis`` and ``PerRow``, all defined in ``granularity.py`` and
re-exported here as the reference does.
"""

from typing import Optional, Tuple

import torch

from .granularity import Granularity, PerAxis, PerRow, PerTensor
from .quant_primitives import (
    MappingType,
    ZeroPointDomain,
    _get_reduction_params,
    choose_qparams_affine_with_min_max,
)

__all__ = ["AffineQuantizedMinMaxObserver", "PerAxis", "PerRow", "PerTensor", "get_block_size"]


def get_block_size(input_shape: Tuple[int, ...], granularity: Granularity) -> Tuple[int, ...]:
    """The quantization block of ``granularity`` on a tensor of ``input_shape``."""
    if isinstance(granularity, PerTensor):
        return tuple(input_shape)
    if isinstance(granularity, PerAxis):
        block_size = list(input_shape)
        block_size[granularity.axis] = 1
        return tuple(block_size)
    if isinstance(granularity, PerRow):
        return (1,) * (len(input_shape) - 1) + (input_shape[-1],)
    raise ValueError(f"Unsupported Granularity: {granularity}")


class AffineQuantizedMinMaxObserver(torch.nn.Module):
    """Tracks the running min / max per quantization block; arguments as
    ``choose_qparams_affine``'s, with ``granularity`` in place of a block size."""

    def __init__(
        self,
        mapping_type: MappingType,
        target_dtype: torch.dtype,
        granularity: Granularity,
        quant_min: Optional[int] = None,
        quant_max: Optional[int] = None,
        eps: Optional[float] = None,
        scale_dtype: Optional[torch.dtype] = None,
        zero_point_dtype: Optional[torch.dtype] = None,
        preserve_zero: bool = True,
        zero_point_domain: ZeroPointDomain = ZeroPointDomain.INT,
    ):
        super().__init__()
        assert granularity is not None, "granularity is None"
        if zero_point_domain is None:
            raise ValueError("Please use ZeroPointDomain.NONE instead of None")
        self.mapping_type = mapping_type
        self.target_dtype = target_dtype
        self.granularity = granularity
        self.quant_min = quant_min
        self.quant_max = quant_max
        self.eps = eps
        self.scale_dtype = scale_dtype
        self.zero_point_dtype = zero_point_dtype
        self.preserve_zero = preserve_zero
        self.zero_point_domain = zero_point_domain

    @torch.no_grad()
    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if input.numel() == 0:
            return input
        x = input.detach()
        block_size = get_block_size(x.shape, self.granularity)
        view, red = _get_reduction_params(block_size, x.size())
        x = x.view(view)
        min_val = torch.amin(x, dim=red, keepdim=False)
        max_val = torch.amax(x, dim=red, keepdim=False)
        if not hasattr(self, "min_val") or not hasattr(self, "max_val"):
            self.min_val = min_val
            self.max_val = max_val
        else:
            assert self.min_val.shape == min_val.shape and self.max_val.shape == max_val.shape, (
                f"observed shape changed: {tuple(self.min_val.shape)} -> {tuple(min_val.shape)}")
            self.min_val.copy_(torch.min(self.min_val, min_val))
            self.max_val.copy_(torch.max(self.max_val, max_val))
        return input

    def calculate_qparams(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        assert hasattr(self, "min_val") and hasattr(self, "max_val"), (
            "run the observer on data before calculate_qparams")
        return choose_qparams_affine_with_min_max(
            self.min_val,
            self.max_val,
            self.mapping_type,
            [],  # the statistics are already reduced per block
            self.target_dtype,
            self.quant_min,
            self.quant_max,
            self.eps,
            self.scale_dtype,
            self.zero_point_dtype,
            self.preserve_zero,
            self.zero_point_domain,
        )
