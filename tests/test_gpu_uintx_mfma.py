"""The uintx linear's MFMA route (tuning(uintx_mfma=1)) on the committed fixtures' weights and
through quantize_(UIntXWeightOnlyConfig).

Bar: rel-L2 <= 3e-3 against the float64 product on the fixture's codes, zero points and scales,
tests/test_gpu_uintx.py's bar for this linear (one bf16 rounding per output bounds it by 2^-9; the
reference's own linear sits at 1.8e-3 to 2.4e-3 on these weights).
"""

import os

import pytest
import torch

from test_gpu_uintx import FIXTURES, bf16, last_kernel, load, op_args

from torchao.kernel.tuning import tuning
from torchao.quantization import UIntXWeightOnlyConfig, quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_fixture_weights(path):
    d, bits, g = load(path)
    q, zp = torch.from_numpy(d["codes"]).double(), torch.from_numpy(d["zero_point"]).double()
    w64 = (q - zp.repeat_interleave(g, 1)) * bf16(d["scale"]).double().repeat_interleave(g, 1)
    x = torch.randn(16, q.shape[1], generator=torch.Generator().manual_seed(bits)).to(torch.bfloat16)
    y64 = x.double() @ w64.t()
    with tuning(uintx_mfma=1):
        y = torch.ops.torchao.uintx_weight_only_linear(x.to(DEV), *op_args(d, bits, g))
    assert last_kernel() == "gemm_mfma_kernel"
    err = ((y.cpu().double() - y64).norm() / y64.norm()).item()
    print(f"uint{bits} mfma M=16: rel-L2 {err:.3e}")
    assert err <= 3e-3


def test_quantized_module():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(256, 128), torch.nn.Linear(128, 256))
    m = m.to(torch.bfloat16).to(DEV)
    quantize_(m, UIntXWeightOnlyConfig(torch.uint3, 64))
    x = torch.randn(16, 256, device=DEV).to(torch.bfloat16)
    with tuning(uintx_mfma=1):
        y, h = m(x), x
        assert last_kernel() == "gemm_mfma_kernel"
        for lin in m:
            w = lin.weight
            ops = w.tensor_impl._hip_operands(w.block_size, w.zero_point_domain)
            assert ops[-2:] == (3, 64)
            h = torch.ops.torchao.uintx_weight_only_linear(h, *ops, lin.bias)
            assert last_kernel() == "gemm_mfma_kernel"
    assert torch.equal(y, h)
