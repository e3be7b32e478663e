"""UIntXWeightOnlyConfig on the GPU against the fixtures recorded from the reference
(experiments/gen_golden_uintx.py), on both routes of the linear.

Bar of the linear: rel-L2 <= 3e-3 against y64 (float64, unrounded products) without bias. One bf16
rounding per output bounds rel-L2 by 2^-9 = 1.95e-3 and the fp32 accumulation at K <= 384 adds far
less. With a bias the module and the op must agree bit for bit.
"""

import glob
import os

import numpy as np
import pytest
import torch

from torchao import _lib
from torchao.dtypes.uintx.uintx_layout import _linear_bf16_act_uintx_weight_check
from torchao.kernel.tuning import tuning
from torchao.quantization import quantize_, uintx_weight_only

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "uintx_b*.npz")))
SHARDS = ("int4_shard", "int2_shard", "int1_shard")
KERNEL = {1: "uintx_gemv_kernel", 2: "uintx_dequant_kernel"}


def bf16(a):
    return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)


def load(path):
    d = np.load(path)
    name = os.path.basename(path)[:-4].split("_")
    return d, int(name[1][1:]), int(name[4][1:])  # bits, group size


def op_args(d, bits, g):
    return (*(torch.from_numpy(d[n]).to(DEV) if n in d else None for n in SHARDS),
            bf16(d["scale"]).to(DEV), torch.from_numpy(d["zero_point"]).to(DEV), bits, g)


def last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def quantized_module(d, bits, g, dtype=torch.bfloat16):
    N, K = d["w"].shape
    m = torch.nn.Linear(K, N)
    with torch.no_grad():
        m.weight.copy_(bf16(d["w"]))
        m.bias.copy_(bf16(d["bias"]))
    m = m.to(dtype).to(DEV)
    quantize_(m, uintx_weight_only(getattr(torch, f"uint{bits}"), group_size=g))
    return m


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_dequantizer_and_device_bits(path):
    d, bits, g = load(path)
    w = torch.ops.torchao.uintx_dequantize(*op_args(d, bits, g))
    assert last_kernel() == "uintx_dequant_kernel"
    assert torch.equal(w.cpu(), bf16(d["w_hat"]))
    impl = quantized_module(d, bits, g).weight.tensor_impl
    for n in SHARDS:
        if n in d:
            assert torch.equal(getattr(impl.int_data, n).cpu(), torch.from_numpy(d[n])), n
    assert torch.equal(impl.scale.cpu(), bf16(d["scale"]))
    assert torch.equal(impl.zero_point.cpu(), torch.from_numpy(d["zero_point"]))
    m = quantized_module(d, bits, g)
    assert torch.equal(m.weight.dequantize().cpu(), bf16(d["w_hat"]))
    assert last_kernel() == "uintx_dequant_kernel"


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_linear(path, route):
    d, bits, g = load(path)
    m = quantized_module(d, bits, g)
    args = op_args(d, bits, g)
    x8 = torch.cat([bf16(d["x"]), bf16(d["x"])[:3]])
    y64 = torch.cat([torch.from_numpy(d["y64"]), torch.from_numpy(d["y64"])[:3]])
    with tuning(uintx=(route, 0, 0, 0, 0, 0, 0)):
        for M in (1, 2, 3, 5, 8):
            x = x8[:M].to(DEV)
            for y in (torch.nn.functional.linear(x, m.weight),
                      torch.ops.torchao.uintx_weight_only_linear(x, *args)):
                assert last_kernel() == KERNEL[route]
                err = ((y.cpu().double() - y64[:M]).norm() / y64[:M].norm()).item()
                print(f"uint{bits} route {route} M={M}: rel-L2 {err:.3e}")
                assert err <= 3e-3
            y_op = torch.ops.torchao.uintx_weight_only_linear(x, *args, m.bias)
            assert torch.equal(m(x), y_op)


def test_input_shapes_and_fp16():
    d, bits, g = load(FIXTURES[2])
    m = quantized_module(d, bits, g)
    N, K = d["w"].shape
    x = bf16(d["x"])[:4].to(DEV)
    assert torch.equal(m(x.reshape(2, 2, K)), m(x).reshape(2, 2, N))
    assert last_kernel() == "uintx_gemv_kernel"
    assert m(x[:0]).shape == (0, N)
    h = quantized_module(d, bits, g, torch.float16)
    xh = x.to(torch.float16)
    assert not _linear_bf16_act_uintx_weight_check(xh, h.weight, h.bias)
    want = torch.nn.functional.linear(xh, h.weight.dequantize(), h.bias)
    assert want.dtype == torch.float16 and torch.equal(h(xh), want)


def test_opcheck():
    d, bits, g = load(FIXTURES[-1])
    args = op_args(d, bits, g)
    x = bf16(d["x"]).to(DEV)
    torch.library.opcheck(torch.ops.torchao.uintx_dequantize.default, args)
    torch.library.opcheck(torch.ops.torchao.uintx_weight_only_linear.default,
                          (x, *args, bf16(d["bias"]).to(DEV)))
