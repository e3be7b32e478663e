"""``MXFPInferenceConfig`` and its ``quantize_`` handler.

Reference: torchao/prototype/mx_formats/inference_workflow.py:37-126, which asserts
``is_sm_at_least_100()`` and carries ``# TODO handle AMD``. Here the handler has no such assertion:
the product runs on gfx950's block-scaled fp8 MFMA (csrc/mx_fp8.hip).
"""

import types
from dataclasses import dataclass

import torch

from torchao.core.config import AOBaseConfig
from torchao.prototype.mx_formats.config import SERVED, MXGemmKernelChoice, _check_pair
from torchao.prototype.mx_formats.mx_tensor import MXTensor, QuantizeTensorToMXKwargs
from torchao.quantization.quant_api import _swap_weight
from torchao.quantization.transform_module import register_quantize_module_handler


@dataclass
class MXFPInferenceConfig(AOBaseConfig):
    """MX dynamic-activation inference, 32-element blocks with E8M0 scales: float8_e4m3fn
    activations with float8_e4m3fn (MXFP8) or float4_e2m1fn_x2 (MXFP4) weights. The reference asserts
    equal dtypes; the mixed pair is this project's fp4 recipe (the block-scaled MFMA of gfx950 mixes
    operand formats), and fp4 activations are not built. ``gemm_kernel_choice`` is kept and round-trips for API and checkpoint
    compatibility; it does not pick a kernel (every value runs the HIP path). Every other dtype
    and block size of the reference raises ``NotImplementedError``."""

    block_size: int = 32
    activation_dtype: torch.dtype = torch.float8_e4m3fn
    weight_dtype: torch.dtype = torch.float8_e4m3fn
    gemm_kernel_choice: MXGemmKernelChoice = MXGemmKernelChoice.CUBLAS

    def __post_init__(self):
        _check_pair(self.activation_dtype, self.weight_dtype, self.block_size)
        if not isinstance(self.gemm_kernel_choice, MXGemmKernelChoice):
            raise TypeError(f"gemm_kernel_choice must be an MXGemmKernelChoice, got "
                            f"{self.gemm_kernel_choice!r}")


class NVFP4InferenceConfig:
    """NVFP4 (reference inference_workflow.py:129) is not built."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"NVFP4 is not built. {SERVED}")


def _mx_extra_repr(self):
    """The reference's extra_repr for this workflow: the weight's own repr."""
    n, k = self.weight.shape
    return f"in_features={k}, out_features={n}, weight={self.weight!r}"


@register_quantize_module_handler(MXFPInferenceConfig)
def _mx_inference_linear_transform(module: torch.nn.Module, config: MXFPInferenceConfig):
    # a config's fields can be reassigned after construction: refuse before touching the weight
    _check_pair(config.activation_dtype, config.weight_dtype, config.block_size)
    assert module.weight.dtype == torch.bfloat16, (
        f"Only supporting bf16 out dtype for now, got {module.weight.dtype}")
    recipe = dict(block_size=config.block_size, gemm_kernel_choice=config.gemm_kernel_choice)
    activation = QuantizeTensorToMXKwargs(elem_dtype=config.activation_dtype, **recipe)
    _swap_weight(module, MXTensor.to_mx(module.weight, config.weight_dtype,
                                        act_quant_kwargs=activation, **recipe))
    module.extra_repr = types.MethodType(_mx_extra_repr, module)
    return module
