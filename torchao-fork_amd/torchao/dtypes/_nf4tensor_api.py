"""``NF4WeightOnlyConfig`` / ``nf4_weight_only``: ``quantize_`` workflow of the NF4 (QLoRA) weight
format (the reference's torchao/dtypes/_nf4tensor_api.py, same module path). The module's weight
becomes an ``NF4Tensor`` parameter without grad; a bf16 weight on a HIP device is quantized by the
gfx950 block quantizer (torchao/dtypes/nf4tensor.py)."""

from dataclasses import dataclass

from torch import nn

from torchao.core.config import AOBaseConfig
from torchao.dtypes.nf4tensor import to_nf4
from torchao.quantization.transform_module import register_quantize_module_handler


@dataclass
class NF4WeightOnlyConfig(AOBaseConfig):
    block_size: int = 64
    scaler_block_size: int = 256


nf4_weight_only = NF4WeightOnlyConfig  # the older spelling


@register_quantize_module_handler(NF4WeightOnlyConfig)
def _quantize_linear_to_nf4(module: nn.Module, config: NF4WeightOnlyConfig) -> nn.Module:
    weight = to_nf4(module.weight, config.block_size, config.scaler_block_size)
    module.weight = nn.Parameter(weight, requires_grad=False)
    return module
