"""MoE quantization (reference torchao/prototype/moe_quant): ``MoEQuantConfig`` over a base
weight-only config, and the quantizable MoE feed-forward module it applies to."""

from .quantizable_moe_modules import (
    ConditionalFeedForwardAOQuantizable,
    MOEFeedForwardAOQuantizable,
)
from .utils import (
    MoEQuantConfig,
    UseFakeExtraDimTensor,
    cond_ffn_filter,
    moe_filter,
    moe_quant_fn,
)

__all__ = ["MoEQuantConfig", "UseFakeExtraDimTensor", "moe_filter", "cond_ffn_filter",
           "moe_quant_fn", "MOEFeedForwardAOQuantizable", "ConditionalFeedForwardAOQuantizable"]
