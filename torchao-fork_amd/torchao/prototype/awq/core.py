"""AWQ observer and observed linear (reference torchao/prototype/awq/core.py).

The observer records a linear's inputs during calibration; ``calculate_qparams`` then searches
the per-input-channel equalization scale the reference searches (core.py:64-94):

1. ``m`` = the per-channel mean of ``|x|`` over all recorded tokens;
2. candidate ``i`` of ``n``: ``s = m.pow(i / n)`` cast to the weight dtype, clamped at 1e-4 and
   divided by ``sqrt(max(s) * min(s))``;
3. loss = mean squared difference between the float linear and the base config's quantized linear
   of ``weight * s`` applied to ``x / s``;
4. the first strict minimum wins.

The quantized linear of step 3 runs on this package's kernels, so calibration runs where they
run: on the GPU. On CPU tensors the inner op raises; there is no fallback.

One addition to the reference's surface: after ``calculate_qparams`` the observer keeps the loss
table as ``losses``, one Python float per candidate, for tests and for debugging a calibration.
"""

from enum import Enum
from typing import List, Optional

import torch
import torch.nn.functional as F

from torchao.core.config import AOBaseConfig
from torchao.quantization.transform_module import _QUANTIZE_CONFIG_HANDLER
from torchao.utils import DummyModule

__all__ = ["AWQStep", "AWQObserver", "AWQObservedLinear", "get_act_scale"]


class AWQStep(str, Enum):
    PREPARE = "prepare"
    CONVERT = "convert"
    PREPARE_FOR_LOADING = "prepare_for_loading"


@torch.no_grad()
def get_act_scale(x: torch.Tensor) -> torch.Tensor:
    return x.abs().view(-1, x.shape[-1]).mean(0)


def _served_base_configs():
    from torchao.quantization.quant_api import (
        Float8WeightOnlyConfig,
        Int4WeightOnlyConfig,
        Int8WeightOnlyConfig,
    )

    return (Int4WeightOnlyConfig, Int8WeightOnlyConfig, Float8WeightOnlyConfig)


def check_awq_served(weight: torch.Tensor, base_config: AOBaseConfig) -> None:
    """AWQ applies to weight-only quantization of a 2-D linear weight."""
    served = _served_base_configs()
    names = ", ".join(c.__name__ for c in served)
    if not isinstance(base_config, served):
        raise NotImplementedError(
            f"AWQ over {type(base_config).__name__} is not served: the activation scale applies to "
            f"weight-only base configs ({names})")
    if weight.dim() != 2:
        raise NotImplementedError(
            f"AWQ over a {weight.dim()}-D weight {tuple(weight.shape)} is not served: 2-D linear "
            f"weights with a weight-only base config ({names}) are")


class AWQObserver(torch.nn.Module):
    """Records the inputs of one linear and searches its equalization scale."""

    def __init__(
        self,
        weight: torch.Tensor,
        bias: Optional[torch.Tensor],
        base_config: AOBaseConfig,
        scale_search_space_size: int = 20,
    ):
        super().__init__()
        self.base_config = base_config
        self.weight = weight
        self.bias = bias
        self.inputs: List[torch.Tensor] = []
        self.scale_options = scale_search_space_size
        self.device = self.weight.device
        self.losses: List[float] = []

    @torch.no_grad()
    def forward(self, input: torch.Tensor, output: torch.Tensor):
        self.inputs.append(input.to("cpu"))

    @torch.no_grad()
    def calculate_qparams(self) -> torch.Tensor:
        assert self.inputs, "calibrate observer first by running model on exemplar data"
        bias = None if self.bias is None else self.bias.to(self.device)
        acc = torch.cat([x.to(self.device) for x in self.inputs], dim=-2)
        x_mean = get_act_scale(acc)
        handler = _QUANTIZE_CONFIG_HANDLER[type(self.base_config)]
        orig_out = F.linear(acc, self.weight, bias)

        best_loss = float("inf")
        best_scales = None
        self.losses = []
        for i in range(self.scale_options):
            ratio = i * 1 / self.scale_options
            scales = x_mean.pow(ratio).to(self.weight.dtype).clamp(min=1e-4).view(-1)
            if best_scales is None:
                best_scales = scales
            scales = scales / (scales.max() * scales.min()).sqrt()
            w = handler(DummyModule(self.weight * scales), self.base_config).weight
            q_out = F.linear(acc / scales, w, bias)
            loss = (orig_out - q_out).pow(2).mean().item()
            self.losses.append(loss)
            if loss < best_loss:
                best_scales = scales
                best_loss = loss
        return best_scales.detach()


class AWQObservedLinear(torch.nn.Linear):
    """A linear that computes the float output and hands its input to the observer."""

    def __init__(self, in_features: int, out_features: int, act_obs: torch.nn.Module,
                 bias: bool = True, device=None, dtype=None):
        super().__init__(in_features, out_features, bias, device, dtype)
        self.act_obs = act_obs

    def forward(self, input: torch.Tensor):
        output = F.linear(input, self.weight, self.bias)
        self.act_obs(input, output)
        return output

    @classmethod
    def from_float(cls, float_linear: torch.nn.Linear, act_obs: AWQObserver):
        observed_linear = cls(
            float_linear.in_features,
            float_linear.out_features,
            act_obs,
            False,
            device=float_linear.weight.device,
            dtype=float_linear.weight.dtype,
        )
        observed_linear.weight = float_linear.weight
        observed_linear.bias = float_linear.bias
        return observed_linear
