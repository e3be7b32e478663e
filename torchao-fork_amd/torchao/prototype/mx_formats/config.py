"""Enums and validation of the MX formats (reference torchao/prototype/mx_formats/config.py)."""

from enum import Enum

import torch

SERVED = ("MXFP8 inference is served: MXFPInferenceConfig with activation_dtype = weight_dtype = "
          "torch.float8_e4m3fn, block_size = 32, ScaleCalculationMode.FLOOR, bf16 modules. "
          "MXFP4 weights are served under float8 activations: activation_dtype = "
          "torch.float8_e4m3fn with weight_dtype = torch.float4_e2m1fn_x2")


class MXGemmKernelChoice(Enum):
    """Kept for API and checkpoint compatibility, and it round-trips; it does not pick a kernel
    here: every value runs the HIP path (csrc/mx_fp8.hip)."""

    EMULATED = "emulated"
    CUTLASS = "cutlass"
    CUBLAS = "cublas"


class ScaleCalculationMode(Enum):
    """How a block's power-of-two scale is derived from its amax. FLOOR is served."""

    FLOOR = "floor"
    RCEIL = "rceil"
    CEIL = "ceil"
    EVEN = "even"


def _check_served(elem_dtype, block_size, scaling_mode=ScaleCalculationMode.FLOOR,
                  pack_fp6=False, weight=False):
    """NotImplementedError, naming what is served, for every MX recipe that is not. e2m1 is an
    element dtype of a weight (``weight=True``) only."""
    if elem_dtype != torch.float8_e4m3fn and not (weight and elem_dtype == torch.float4_e2m1fn_x2):
        raise NotImplementedError(f"MX element dtype {elem_dtype} is not built. {SERVED}")
    if block_size != 32:
        raise NotImplementedError(f"MX block_size {block_size} is not built. {SERVED}")
    if scaling_mode != ScaleCalculationMode.FLOOR:
        raise NotImplementedError(f"MX {scaling_mode} is not built. {SERVED}")
    if pack_fp6:
        raise NotImplementedError(f"fp6 packing is not built. {SERVED}")


def _check_pair(activation_dtype, weight_dtype, block_size):
    """The two served (activation, weight) pairs: e4m3fn x e4m3fn and e4m3fn x e2m1."""
    _check_served(weight_dtype, block_size, weight=True)
    if activation_dtype != torch.float8_e4m3fn:
        raise NotImplementedError(
            f"MX activation_dtype {activation_dtype} with weight_dtype {weight_dtype} is not "
            f"built. {SERVED}")


class MXLinearConfig:
    """MXLinear training (reference config.py:124) is not built."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"MXLinear training is not built. {SERVED}")


torch.serialization.add_safe_globals([MXGemmKernelChoice, ScaleCalculationMode])
