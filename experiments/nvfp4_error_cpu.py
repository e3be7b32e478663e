"""Rel-L2 of the NVFP4 product against the unquantized one, beside MXFP4's, on the CPU: Gaussian
weights (4096 x 4096, sigma 0.02) and activations (16 x 4096), float64 products of the plain-torch
quantizers' codes. Prints one line per recipe; no GPU, no timing.

python experiments/nvfp4_error_cpu.py
"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchao-fork_amd"))
import torch  # noqa: E402

from torchao.prototype.mx_formats.mx_tensor import F4_E2M1, to_dtype, to_mx  # noqa: E402
from torchao.prototype.mx_formats.nvfp4_tensor import (  # noqa: E402
    NVFP4Tensor,
    _snap,
    per_tensor_amax_to_scale,
)


def rel_l2(y, ref):
    return float((y - ref).norm() / ref.norm())


def main():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(4096, 4096, generator=g) * 0.02).to(torch.bfloat16)
    x = torch.randn(16, 4096, generator=g).to(torch.bfloat16)
    ref = x.double() @ w.double().t()
    nv = NVFP4Tensor.to_nvfp4(w).to_dtype(torch.float32).double()
    # sigma 0.02 puts amax / 6 of most blocks below 2^-6, the smallest scale e4m3 is clamped to; the
    # per-tensor scale (which quantize_ does not set, as in the reference) moves the block scales
    # into e4m3's range
    pts = per_tensor_amax_to_scale(w.abs().max())
    nvp = NVFP4Tensor.to_nvfp4(w.float(), per_tensor_scale=pts).to_dtype(torch.float32).double()
    s4, q4 = to_mx(w, F4_E2M1, 32)
    m4 = to_dtype(q4, s4, F4_E2M1, 32, torch.float32).double()
    s8, q8 = to_mx(x, torch.float8_e4m3fn, 32)
    x8 = to_dtype(q8, s8, torch.float8_e4m3fn, 32, torch.float32).double()
    for name, y in (("NVFP4 weight-only", x.double() @ nv.t()),
                    ("NVFP4 dynamic", _snap(x, None).double() @ nv.t()),
                    ("NVFP4 weight-only, per-tensor scale", x.double() @ nvp.t()),
                    ("NVFP4 dynamic, per-tensor scale", _snap(x, None).double() @ nvp.t()),
                    ("MXFP4 weights, bf16 activations", x.double() @ m4.t()),
                    ("MXFP4 weights, MXFP8 activations", x8 @ m4.t())):
        print(f"{name:36s} rel-L2 {rel_l2(y, ref):.3f}")


if __name__ == "__main__":
    main()
