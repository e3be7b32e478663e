"""rel-L2 of the uintx-quantized product against the unquantized one, per bit width, on the CPU.

Definition: W is 1024 x 4096 of N(0, 0.02^2) and x is 16 x 4096 of N(0, 1), both rounded to bf16
(torch.manual_seed(0), W drawn first), no bias; W^ = dequantize(UIntXWeightOnlyConfig's
quantization of W at group size 64); the figure is |x W^T - x W^^T|_2 / |x W^T|_2 in float64.
Asymmetric min / max quantization of a Gaussian group of 64 spans about +-2.4 sigma, so uint2's
four levels sit 1.6 sigma apart: hence 0.46 (a clipped or MSE-optimal range, or a smaller group,
gives a smaller figure).

python experiments/uintx_error_table.py
"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchao-fork_amd"))
import torch  # noqa: E402

import torchao  # noqa: E402,F401
from torchao.dtypes import UintxLayout, to_affine_quantized_intx  # noqa: E402
from torchao.quantization import MappingType, ZeroPointDomain  # noqa: E402

torch.manual_seed(0)
w = (torch.randn(1024, 4096) * 0.02).to(torch.bfloat16)
x = torch.randn(16, 4096).to(torch.bfloat16)
ref = x.double() @ w.double().t()
for bits in range(1, 8):
    dt = getattr(torch, f"uint{bits}")
    t = to_affine_quantized_intx(
        w, MappingType.ASYMMETRIC, (1, 64), dt, eps=torch.finfo(torch.float32).eps,
        zero_point_dtype=torch.int32, zero_point_domain=ZeroPointDomain.INT,
        _layout=UintxLayout(dt))
    y = x.double() @ t.dequantize().double().t()
    print(f"uint{bits} {((y - ref).norm() / ref.norm()).item():.3f}")
