"""MX formats (reference torchao/prototype/mx_formats), the part served on gfx950: MXFP8 inference.

``quantize_(model, MXFPInferenceConfig())`` turns the bf16 weight of every ``nn.Linear`` into an
``MXTensor`` (float8_e4m3fn codes, one float8_e8m0fnu scale per 32 elements along K); the forward
quantizes the activation the same way and runs the product on the block-scaled fp8 MFMA
(``torch.ops.torchao.mx_dyn_linear``; csrc/mx_fp8.hip). Everything else of the reference package
(e5m2, fp6, fp4, NVFP4, ``MXLinear`` training, the EVEN / CEIL / RCEIL scale modes, fp6 packing,
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
)

__all__ = [
    "MXGemmKernelChoice",
    "MXLinearConfig",
    "ScaleCalculationMode",
    "MXFPInferenceConfig",
    "NVFP4InferenceConfig",
]
