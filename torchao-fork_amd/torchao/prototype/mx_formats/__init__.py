"""MX formats (reference torchao/prototype/mx_formats), the part served on gfx950: MXFP8, MXFP4-weight
and NVFP4 inference.

``quantize_(model, MXFPInferenceConfig())`` turns the bf16 weight of every ``nn.Linear`` into an
``MXTensor`` (float8_e4m3fn codes, one float8_e8m0fnu scale per 32 elements along K); the forward
quantizes the activation the same way and runs the product on the block-scaled fp8 MFMA
(``torch.ops.torchao.mx_dyn_linear``; csrc/mx_fp8.hip).
``quantize_(model, NVFP4InferenceConfig(mm_config=..., use_triton_kernel=False))`` turns it into an
``NVFP4Tensor`` (e2m1 codes, one float8_e4m3fn scale per 16 elements; csrc/nvfp4.hip), weight-only or
with NVFP4 activations. Everything else of the reference package
(e5m2, fp6, fp4 activations, the Triton NVFP4 quantizer, ``MXLinear`` training, the EVEN / CEIL / RCEIL scale modes, fp6 packing,
DTensor) is not built and raises ``NotImplementedError``.
"""

from torchao.prototype.mx_formats.config import (
    MXGemmKernelChoice,
    MXLinearConfig,
    ScaleCalculationMode,
)
from torchao.prototype.mx_formats.inference_workflow import (
    MXFPInferenceConfig,
    NVFP4InferenceConfig,
    _auto_filter_for_nfp4,
)
from torchao.prototype.mx_formats.nvfp4_tensor import (
    NVFP4MMConfig,
    NVFP4Tensor,
    QuantizeTensorToNVFP4Kwargs,
)

__all__ = [
    "MXGemmKernelChoice",
    "MXLinearConfig",
    "ScaleCalculationMode",
    "MXFPInferenceConfig",
    "NVFP4InferenceConfig",
    "NVFP4MMConfig",
    "NVFP4Tensor",
    "QuantizeTensorToNVFP4Kwargs",
    "_auto_filter_for_nfp4",
]
