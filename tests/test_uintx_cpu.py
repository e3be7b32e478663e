"""UIntXWeightOnlyConfig on the CPU against fixtures recorded from the reference
(experiments/gen_golden_uintx.py): packing, quantization, dequantization and the plain-torch linear
bit for bit for all seven widths; checkpoints; refusals; the route rule through the C ABI."""

import glob
import os

import numpy as np
import pytest
import torch

from torchao import _lib
from torchao.dtypes import AffineQuantizedTensor, UintxLayout, UintxTensor, to_affine_quantized_intx
from torchao.dtypes.uintx.bitpacking import pack, unpack
from torchao.kernel.tuning import tuning
from torchao.quantization import (
    MappingType,
    UIntXWeightOnlyConfig,
    ZeroPointDomain,
    quantize_,
    uintx_weight_only,
)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "uintx_b*.npz")))
SHARDS = ("int4_shard", "int2_shard", "int1_shard")


def bf16(a):
    return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)


def load(path):
    d = np.load(path)
    name = os.path.basename(path)[:-4].split("_")
    return d, int(name[1][1:]), int(name[4][1:])  # bits, group size


def test_all_seven_widths_have_a_fixture():
    assert sorted(load(p)[1] for p in FIXTURES) == [1, 2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_pack_quantize_dequantize_linear_match_the_reference(path):
    d, bits, g = load(path)
    codes = torch.from_numpy(d["codes"])
    want = [torch.from_numpy(d[n]) for n in SHARDS if n in d]
    got = pack(codes, bits)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(unpack(want, bits), codes)

    t = to_affine_quantized_intx(
        bf16(d["w"]), MappingType.ASYMMETRIC, (1, g), getattr(torch, f"uint{bits}"),
        eps=torch.finfo(torch.float32).eps, zero_point_dtype=torch.int32,
        zero_point_domain=ZeroPointDomain.INT, preserve_zero=True,
        _layout=UintxLayout(getattr(torch, f"uint{bits}")))
    impl = t.tensor_impl
    assert isinstance(impl.int_data, UintxTensor) and impl.int_data.bit_width == bits
    assert all(torch.equal(a, b) for a, b in zip(impl.int_data.get_shards(), want))
    assert torch.equal(impl.scale, bf16(d["scale"]))
    assert impl.zero_point.dtype == torch.int32
    assert torch.equal(impl.zero_point, torch.from_numpy(d["zero_point"]))
    assert torch.equal(t.dequantize(), bf16(d["w_hat"]))
    y = torch.nn.functional.linear(bf16(d["x"]), t, bf16(d["bias"]))
    assert torch.equal(y, bf16(d["y_ref"]))


def test_checkpoints(tmp_path):
    stem = os.path.join(GOLDEN, "uintx_refckpt_b3_N32_K128_g64")
    d = np.load(stem + ".npz")
    sd = torch.load(stem + ".pt", weights_only=True)
    assert isinstance(sd["weight"], AffineQuantizedTensor)
    assert torch.equal(sd["weight"].dequantize(), bf16(d["w_hat"]))
    m = torch.nn.Linear(128, 32).to(torch.bfloat16)
    with torch.no_grad():
        m.weight.copy_(bf16(d["w"]))
        m.bias.copy_(bf16(d["bias"]))
    quantize_(m, uintx_weight_only(torch.uint3, group_size=64))
    torch.save(m.state_dict(), tmp_path / "own.pt")
    own = torch.load(tmp_path / "own.pt", weights_only=True)
    for a, b in zip(own["weight"].tensor_impl.int_data.get_shards(),
                    sd["weight"].tensor_impl.int_data.get_shards()):
        assert torch.equal(a, b)
    assert torch.equal(own["weight"].dequantize(), bf16(d["w_hat"]))
    m2 = torch.nn.Linear(128, 32).to(torch.bfloat16)
    m2.load_state_dict(sd, assign=True)
    x = torch.ones(2, 128, dtype=torch.bfloat16)
    assert torch.equal(m2(x), m(x))


class Stacked(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(2, 8, 64, dtype=torch.bfloat16))


@pytest.mark.parametrize("config,module,error", [
    (UIntXWeightOnlyConfig(torch.uint4, use_hqq=True), None, NotImplementedError),
    (UIntXWeightOnlyConfig(torch.uint8), None, NotImplementedError),
    (UIntXWeightOnlyConfig(torch.uint3, pack_dim=0), None, NotImplementedError),
    (UIntXWeightOnlyConfig(torch.uint3), Stacked(), NotImplementedError),
    (UIntXWeightOnlyConfig(torch.uint3, group_size=64), torch.nn.Linear(96, 8), AssertionError),
])
def test_refusals_leave_the_model_untouched(config, module, error):
    first = torch.nn.Linear(128, 8)
    model = torch.nn.Sequential(first, module or torch.nn.Linear(128, 8)).to(torch.bfloat16)
    with pytest.raises(error, match="served: torch.uint1" if error is NotImplementedError
                       else "divisible by block_size"):
        quantize_(model, config, filter_fn=lambda m, fqn: hasattr(m, "weight"))
    assert type(first.weight) is torch.nn.Parameter


def test_route_rule_and_tuning_hook():
    """csrc/uintx_host.h through the C ABI: GEMV up to the built-in boundary (at least one token,
    at most the 8 one launch serves) for every width, dequantize + matmul above; the hook forces a
    route and moves the boundary."""
    route = _lib.lib().tao_uintx_linear_route
    _lib.call("tao_tune_reset")
    for bits in range(1, 8):
        boundary = max(m for m in range(0, 10) if m == 0 or route(m, 4096, 4096, bits) == 1)
        assert 1 <= boundary <= 8
        assert [route(m, 14336, 4096, bits) for m in (1, boundary, boundary + 1, 512)] == [1, 1, 2, 2]
    with tuning(uintx=(2, 0, 0, 0, 0, 0, 0)):
        assert route(1, 4096, 4096, 3) == 2
    with tuning(uintx=(1, 0, 0, 0, 0, 0, 0)):
        assert route(512, 4096, 4096, 3) == 1
    with tuning(uintx=(0, 2, 0, 0, 0, 0, 0)):
        assert [route(m, 256, 128, 3) for m in (2, 3)] == [1, 2]
    for bad in ((3, 0, 0, 0, 0, 0, 0), (0, -1, 0, 0, 0, 0, 0), (0, 0, 3, 0, 0, 0, 0),
                (0, 0, 0, 4, 4, 0, 0), (0, 0, 0, 0, 0, 12, 0), (0, 0, 0, 0, 0, 0, 3)):
        with pytest.raises(RuntimeError, match="tune: uintx"):
            _lib.call("tao_tune_uintx", *bad)
    assert route(1, 4096, 4096, 3) == 1
    # the lane unit: the measured rule on (K, bits, M) of csrc/uintx_host.h, and the hook
    unit = _lib.lib().tao_uintx_gemv_unit
    assert [unit(1, 4096, b) for b in range(1, 8)] == [8, 8, 8, 4, 4, 4, 8]
    assert [unit(2, 4096, b) for b in range(1, 8)] == [8, 4, 4, 4, 4, 8, 8]
    assert [unit(4, 4096, b) for b in range(1, 8)] == [8, 8, 8, 8, 4, 4, 4]
    assert {unit(m, 4096, b) for m in (5, 8, 64) for b in range(1, 8)} == {8}
    assert {unit(m, 14336, b) for m in (1, 2) for b in range(1, 8)} == {16}
    assert [unit(4, 14336, b) for b in range(1, 8)] == [16, 8, 8, 16, 16, 16, 16]
    assert [unit(8, 14336, b) for b in range(1, 8)] == [16, 8, 16, 16, 16, 8, 8]
    assert unit(1, 384, 3) == 4
    for u in (4, 8, 16):
        with tuning(uintx=(0, 0, 0, 0, 0, u, 0)):
            assert unit(1, 4096, 5) == u
    # x staged in LDS: only the 4- and 8-token tiles, only while [MT][K] bf16 fits 128 KiB
    x_lds = _lib.lib().tao_uintx_gemv_x_lds
    with tuning(uintx=(0, 0, 0, 0, 0, 0, 2)):
        assert [x_lds(m, k, 2) for m, k in ((1, 4096), (2, 4096), (3, 4096), (8, 4096), (8, 8192),
                                            (4, 14336), (8, 14336))] == [0, 0, 1, 1, 1, 1, 0]
    with tuning(uintx=(0, 0, 0, 0, 0, 0, 1)):
        assert {x_lds(m, 4096, 7) for m in (1, 4, 8)} == {0}
    # built-in: the measured rule, 3 to 4 tokens of uint4 .. uint7 at 4096 <= K < 8192
    assert [x_lds(4, 4096, b) for b in range(1, 8)] == [0, 0, 0, 1, 1, 1, 1]
    assert x_lds(3, 4096, 5) == 1
    assert {x_lds(m, k, 7) for m, k in ((1, 4096), (2, 4096), (8, 4096), (4, 14336), (4, 2176))} == {0}
    with tuning(uintx=(0, 0, 8, 0, 0, 16, 0)):  # 8 rows per wave hold at most an 8-byte unit
        assert (unit(1, 14336, 7), unit(4, 14336, 7)) == (8, 16)
