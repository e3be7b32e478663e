"""``MXFPInferenceConfig`` and ``NVFP4InferenceConfig`` with their ``quantize_`` handlers.

Reference: torchao/prototype/mx_formats/inference_workflow.py:37-126, which asserts
``is_sm_at_least_100()`` and carries ``# TODO handle AMD``. Here the handler has no such assertion:
the product runs on gfx950's block-scaled fp8 MFMA (csrc/mx_fp8.hip). ``NVFP4InferenceConfig``
(:129-192) has none either: both of its modes run csrc/nvfp4.hip.
"""

import types
from dataclasses import dataclass

import torch

from torchao.core.config import AOBaseConfig
from torchao.prototype.mx_formats.config import SERVED, MXGemmKernelChoice, _check_pair
from torchao.prototype.mx_formats.mx_tensor import MXTensor, QuantizeTensorToMXKwargs
from torchao.prototype.mx_formats.nvfp4_tensor import (
    NVFP4MMConfig,
    NVFP4Tensor,
    QuantizeTensorToNVFP4Kwargs,
)
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


NVFP4_SERVED = ("NVFP4 inference is served with the HIP activation quantizer: "
                "NVFP4InferenceConfig(mm_config=NVFP4MMConfig.WEIGHT_ONLY, use_triton_kernel=False) "
                "and NVFP4InferenceConfig(mm_config=NVFP4MMConfig.DYNAMIC, use_triton_kernel=False). "
                "use_triton_kernel=True (the reference's default) selects a Triton quantizer that is "
                f"not built. {SERVED}")


def _check_nvfp4(config):
    if not isinstance(config.mm_config, NVFP4MMConfig):
        raise TypeError(f"mm_config must be an NVFP4MMConfig, got {config.mm_config!r}")
    if config.use_triton_kernel:
        raise NotImplementedError(NVFP4_SERVED)


@dataclass
class NVFP4InferenceConfig(AOBaseConfig):
    """NVFP4 inference (reference inference_workflow.py:129): float4_e2m1fn_x2 codes, one
    float8_e4m3fn scale per 16 elements along K. ``mm_config`` WEIGHT_ONLY multiplies bf16
    activations with the quantized weight; DYNAMIC quantizes the activation to NVFP4 too. The
    fields and defaults are the reference's, and the default ``use_triton_kernel=True`` raises, as
    the Triton activation quantizer it selects does not exist here: pass ``False``."""

    mm_config: NVFP4MMConfig = NVFP4MMConfig.DYNAMIC
    use_triton_kernel: bool = True

    def __post_init__(self):
        _check_nvfp4(self)


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


@register_quantize_module_handler(NVFP4InferenceConfig)
def _nvfp4_inference_linear_transform(module: torch.nn.Module, config: NVFP4InferenceConfig):
    # a config's fields can be reassigned after construction: refuse before touching the weight
    _check_nvfp4(config)
    weight = module.weight
    if weight.shape[0] % 16 != 0 or weight.shape[1] % 16 != 0:
        raise RuntimeError(f"NVFP4 only supports weight shape divisible by 16, got {weight.shape}")
    if module.bias is not None and weight.dtype == torch.float32:
        raise RuntimeError(
            "Bias is not supported when module weight is in fp32 (out_dtype=Float32). "
            "Please use bfloat16 or float16 weights, or remove the bias from the linear layer.")
    act = QuantizeTensorToNVFP4Kwargs() if config.mm_config == NVFP4MMConfig.DYNAMIC else None
    _swap_weight(module, NVFP4Tensor.to_nvfp4(weight.detach().contiguous(), is_swizzled_scales=True,
                                              act_quant_kwargs=act))
    module.extra_repr = types.MethodType(_mx_extra_repr, module)
    return module


def _auto_filter_for_nfp4(mod: torch.nn.Module, fqn: str) -> bool:
    """The reference's generic filter for NVFP4: linears only, no embeddings, both dimensions
    multiples of 16, and not the small layers (N <= 64, or N and K both <= 1024)."""
    if not isinstance(mod, torch.nn.Linear):
        return False
    if any(name in fqn for name in ("embedder", "embed", "embedding", "time_text_embed")):
        return False
    N, K = mod.weight.shape
    if K % 16 != 0 or N % 16 != 0 or N <= 64:
        return False
    return not (K <= 1024 and N <= 1024)
