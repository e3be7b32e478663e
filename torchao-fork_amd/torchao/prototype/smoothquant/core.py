"""SmoothQuant observer and observed linear (reference torchao/prototype/smoothquant/core.py).

The observer tracks the per-input-channel min / max of a linear's inputs during calibration and
of its weight; ``calculate_qparams`` turns them into (core.py:80-128)

1. ``smoothing_factor = xmax ** alpha / wmax ** (1 - alpha)`` per input channel, where ``xmax`` and
   ``wmax`` are the absolute maxima plus ``eps`` (ones when ``alpha`` is None), in the dtype of the
   observed activations;
2. static mode only: ``act_scales``, the per-tensor symmetric scale of the smoothed activation
   range, ``max(-min(min / factor, 0), max(max / factor, 0)) / ((quant_max - quant_min) / 2)``;
3. ``wei_scales``, the per-output-channel symmetric scales of ``weight * smoothing_factor``.

One difference from the reference: the running min / max stay on the device of the observed
tensors (the reference copies every batch to the CPU first). min and max are exact on every
device, so the statistics are the same and calibration on the GPU does no host transfer per
batch; ``calculate_qparams`` brings the four per-channel vectors to the CPU once.
"""

from typing import Optional

import torch
import torch.nn.functional as F

from torchao.quantization.observer import AffineQuantizedMinMaxObserver, PerAxis
from torchao.quantization.quant_primitives import MappingType

__all__ = ["SmoothQuantObserver", "SmoothQuantObservedLinear", "check_smoothquant_served"]


def check_smoothquant_served(weight: torch.Tensor) -> None:
    """SmoothQuant is served on 2-D linear weights with in_features % 16 == 0 (the int8 kernels'
    vector width; there is no leave-unquantized rule for other K, the linear is refused), in any
    float dtype on the CPU (convert is plain torch) and in bfloat16 on the GPU."""
    served = ("served: 2-D linear weights with in_features % 16 == 0, bfloat16 on the GPU "
              "(int8 dynamic or static activation x int8 per-channel weight)")
    if weight.dim() != 2:
        raise NotImplementedError(
            f"SmoothQuant over a {weight.dim()}-D weight {tuple(weight.shape)} is not served; "
            + served)
    if weight.shape[1] % 16 != 0:
        raise NotImplementedError(
            f"SmoothQuant over in_features = {weight.shape[1]} is not served; " + served)
    if weight.is_cuda and weight.dtype != torch.bfloat16:
        raise NotImplementedError(
            f"SmoothQuant over a {weight.dtype} module on the GPU is not served; " + served)


class SmoothQuantObserver(torch.nn.Module):
    """``alpha``: the migration strength (None: a factor of ones, conventional quantization).
    ``quant_mode``: "static" or "dynamic" activation quantization. ``quant_min`` / ``quant_max``:
    the weight's (and the static activation's) integer range. ``eps``: added to the absolute
    maxima and the lower bound of the weight scales."""

    def __init__(
        self,
        weight: torch.Tensor,
        alpha: Optional[float] = 0.5,
        quant_mode: str = "static",
        quant_min: Optional[int] = None,
        quant_max: Optional[int] = None,
        eps: Optional[float] = None,
    ):
        super().__init__()
        assert weight.ndim == 2
        assert quant_mode in ["static", "dynamic"]
        self.weight = weight
        self.inputs = []
        self.device = self.weight.device
        self.alpha = alpha
        self.quant_mode = quant_mode
        self.quant_min = quant_min
        self.quant_max = quant_max
        self.eps = eps
        # activations [tokens, ic], weight [oc, ic]: the *_ic_obs pair gives the smoothing factor,
        # wei_oc_obs the weight's quantization scales
        self.act_ic_obs = AffineQuantizedMinMaxObserver(
            MappingType.SYMMETRIC, torch.int8, PerAxis(-1), eps=eps)
        self.wei_ic_obs = AffineQuantizedMinMaxObserver(
            MappingType.SYMMETRIC, torch.int8, PerAxis(-1), eps=eps)
        self.wei_oc_obs = AffineQuantizedMinMaxObserver(
            MappingType.SYMMETRIC, torch.int8, PerAxis(0), quant_min=quant_min,
            quant_max=quant_max, eps=eps)
        self.wei_ic_obs(self.weight)

    @torch.no_grad()
    def forward(self, input: torch.Tensor):
        self.act_ic_obs(input)
        return input

    @torch.no_grad()
    def calculate_qparams(self):
        """(smoothing_factor [ic], act_scales (0-d) or None, wei_scales [oc]) on ``device``."""
        # The four [ic] statistics go to the CPU, where the reference holds them, so the factor
        # and the activation scale are formed by the same pow / division kernels as there; the
        # weight-sized work below runs on the module's device.
        act_min, act_max = self.act_ic_obs.min_val.cpu(), self.act_ic_obs.max_val.cpu()
        wei_min, wei_max = self.wei_ic_obs.min_val.cpu(), self.wei_ic_obs.max_val.cpu()
        x_abs_max = torch.max(torch.abs(act_min), torch.abs(act_max)) + self.eps
        w_abs_max = torch.max(torch.abs(wei_min), torch.abs(wei_max)) + self.eps
        if self.alpha is None:
            smoothing_factor = torch.ones_like(x_abs_max)
        else:
            smoothing_factor = (torch.pow(x_abs_max, self.alpha)
                                / torch.pow(w_abs_max, 1 - self.alpha))
        act_scales = None
        if self.quant_mode == "static":
            factor = smoothing_factor.reshape(act_min.shape)
            min_val = torch.min(act_min / factor)
            max_val = torch.max(act_max / factor)
            min_neg = torch.min(min_val, torch.zeros_like(min_val))
            max_pos = torch.max(max_val, torch.zeros_like(max_val))
            max_pos = torch.max(-min_neg, max_pos)
            act_scales = (max_pos / (float(self.quant_max - self.quant_min) / 2)).to(self.device)
        self.wei_oc_obs(self.weight * smoothing_factor.to(self.device))
        wei_scales, _ = self.wei_oc_obs.calculate_qparams()
        return smoothing_factor.to(self.device), act_scales, wei_scales.to(self.device)


class SmoothQuantObservedLinear(torch.nn.Linear):
    """A linear that shows its input to the observer and computes the float output."""

    def __init__(self, in_features: int, out_features: int, bias: bool,
                 obs: SmoothQuantObserver, device=None, dtype=None):
        super().__init__(in_features, out_features, bias, device, dtype)
        assert isinstance(obs, SmoothQuantObserver)
        self.obs = obs

    def forward(self, input: torch.Tensor):
        input = self.obs(input)
        return F.linear(input, self.weight, self.bias)

    @classmethod
    def from_float(cls, float_linear: torch.nn.Linear, obs: SmoothQuantObserver):
        observed_linear = cls(
            float_linear.in_features,
            float_linear.out_features,
            float_linear.bias is not None,
            obs,
            device=float_linear.weight.device,
            dtype=float_linear.weight.dtype,
        )
        observed_linear.weight = float_linear.weight
        observed_linear.bias = float_linear.bias
        return observed_linear
