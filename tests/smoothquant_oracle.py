"""Plain-torch restatement of SmoothQuant's activation side and int8 linear, shared by
tests/test_smoothquant_cpu.py (which pins it to the reference's recorded codes, scales and outputs,
tests/golden/smoothquant_*.npz) and tests/test_gpu_smoothquant.py (which uses it as the oracle of
the kernels). Every step is a torch CPU op in bf16, in the reference's order:

  t  = x / factor                                           linear_activation_scale.py:61-70
  dynamic: s = clamp(amax|t| / 127.0, min=2^-7) per token   choose_qparams_affine, eps = finfo(bf16).eps
  static:  s = the calibrated per-tensor scale
  q  = clamp(round(t * (1.0 / s)), -127, 127) -> int8       quantize_affine
  y  = bf16(int32 xq @ wq^T) * s_x, * s_w, + bias           plain_layout.py:281-315, intmm.py:133-137

It imports nothing from the package under test.
"""

import torch

BF16 = torch.bfloat16
EPS_BF16 = torch.finfo(BF16).eps  # 2^-7: what _ActQuantizer.dynamic_quantize's missing eps becomes


def smooth(x: torch.Tensor, factor: torch.Tensor) -> torch.Tensor:
    assert x.dtype == BF16 and factor.dtype == BF16
    return x / factor


def _codes(t: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return torch.clamp(torch.round(t * (1.0 / s)), -127, 127).to(torch.int8)


def dynamic_quant(t: torch.Tensor):
    """(q int8 like t, s bf16 [M]) of a smoothed activation t [M, K]."""
    s = torch.clamp(t.abs().amax(dim=-1) / 127.0, min=EPS_BF16)
    assert s.dtype == BF16
    return _codes(t, s.unsqueeze(-1)), s


def static_quant(t: torch.Tensor, act_scale: torch.Tensor):
    """(q int8 like t, s bf16 [M] filled with the per-tensor scale)."""
    assert act_scale.dtype == BF16 and act_scale.numel() == 1
    return _codes(t, act_scale.reshape(())), act_scale.reshape(1).expand(t.shape[0]).contiguous()


def quant(x, factor, act_scale=None):
    t = smooth(x, factor)
    return dynamic_quant(t) if act_scale is None else static_quant(t, act_scale)


def int8_linear(xq, xs, wq, ws, bias=None):
    """The int8 x int8 linear's epilogue on exact integer dot products (|acc| < 2^53 in float64)."""
    acc = (xq.double() @ wq.double().t()).to(torch.int32)
    y = acc.to(BF16) * xs.reshape(-1, 1).to(BF16)
    y = y * ws.reshape(-1).to(BF16)
    if bias is not None:
        y = y + bias
    return y


def linear(x, factor, act_scale, wq, ws, bias=None):
    xq, xs = quant(x, factor, act_scale)
    return int8_linear(xq, xs, wq, ws, bias)
