"""Blockwise float8 inference (e4m3fn codes, fp32 scales per 1 x 128 activation block and per
128 x 128 weight block) on the gfx950 kernels of csrc/block_fp8.hip."""

from .blockwise_linear import BlockwiseQuantLinear
from .blockwise_quantization import (
    blockwise_fp8_gemm,
    fp8_blockwise_act_quant,
    fp8_blockwise_weight_dequant,
    fp8_blockwise_weight_quant,
)

__all__ = [
    "BlockwiseQuantLinear",
    "blockwise_fp8_gemm",
    "fp8_blockwise_act_quant",
    "fp8_blockwise_weight_dequant",
    "fp8_blockwise_weight_quant",
]
