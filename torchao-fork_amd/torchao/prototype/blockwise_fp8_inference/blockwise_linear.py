"""``BlockwiseQuantLinear``: a linear layer on blockwise float8 weights (e4m3fn codes, one fp32 scale
per 128 x 128 block) with the activation quantized per 1 x 128 block on the fly. Constructor,
parameter names and ``state_dict`` keys are the reference's
(torchao/prototype/blockwise_fp8_inference/blockwise_linear.py), so a Hugging Face ``weight`` +
``weight_scale_inv`` pair loads as ``weight`` + ``scale``. ``from_float`` is the one addition."""

import torch
from torch import nn

from torchao.prototype.blockwise_fp8_inference.blockwise_quantization import (
    _blockwise_mm_cpu,
    _check_k,
    _check_served,
    fp8_blockwise_act_quant,
    fp8_blockwise_weight_quant,
)


class BlockwiseQuantLinear(nn.Module):
    """
    Args:
        in_features (int): Number of input features (a multiple of 128).
        out_features (int): Number of output features.
        bias (bool): Whether to include a bias term. Defaults to False.
        block_size (int): Block size for quantization; 128 only.
        dtype (torch.dtype): Data type of the weight codes; torch.float8_e4m3fn only.

    The activation is always quantized to e4m3fn (the reference's ``forward`` passes the class
    attribute ``dtype = torch.bfloat16`` to its activation quantizer, which asserts on it). The
    output is bf16.
    """

    dtype = torch.bfloat16

    def __init__(
        self,
        in_features: int,
        out_features: int,
        bias: bool = False,
        block_size: int = 128,
        dtype: torch.dtype = torch.float8_e4m3fn,
    ):
        super().__init__()
        _check_served(block_size, dtype)
        _check_k(in_features)
        scale_in_features = (in_features + block_size - 1) // block_size
        scale_out_features = (out_features + block_size - 1) // block_size
        self.in_features = in_features
        self.out_features = out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features, dtype=dtype),
                                   requires_grad=False)
        self.weight.scale = self.scale = nn.Parameter(
            torch.empty(scale_out_features, scale_in_features, dtype=torch.float32),
            requires_grad=False)
        self.block_size = block_size

        if bias:
            self.bias = nn.Parameter(torch.empty(out_features), requires_grad=False)
        else:
            self.register_parameter("bias", None)

    @classmethod
    def from_float(cls, linear: nn.Linear) -> "BlockwiseQuantLinear":
        """Quantize an ``nn.Linear`` (bf16 weight on a HIP device; any float dtype on the CPU)."""
        mod = cls(linear.in_features, linear.out_features, bias=linear.bias is not None)
        wq, ws = fp8_blockwise_weight_quant(linear.weight.detach().contiguous())
        mod.weight = nn.Parameter(wq, requires_grad=False)
        mod.weight.scale = mod.scale = nn.Parameter(ws, requires_grad=False)
        if linear.bias is not None:
            mod.bias = nn.Parameter(linear.bias.detach().clone(), requires_grad=False)
        return mod

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        bias = self.bias
        if bias is not None and bias.dtype is not torch.bfloat16:
            bias = bias.to(torch.bfloat16)
        if x.is_cuda:
            return torch.ops.torchao.blockfp8_dyn_linear(x, self.weight, self.scale, bias)
        xq, xs = fp8_blockwise_act_quant(x, self.block_size)
        return _blockwise_mm_cpu(xq, xs, self.weight, self.scale, bias)
