"""Bit-exact GPU tests of torch.ops.torchao.uintx_weight_only_linear on both routes.

x holds integers in [-8, 8], scales are 1, 2 or 4, every code of the width is present and zero
points are arbitrary in-range integers, so every product x (q - zp) s is an integer of magnitude
<= 4 * 8 * 127 and every partial sum, in any order, an exact fp32 number:
|sum| <= 4 * 8 * 127 * K < 2^24 for K <= 4096. The output must therefore equal the float64 formula
rounded once to bf16 (with a bias: rounded, added in fp32, rounded again) under torch.equal,
whatever the route, tile, lane unit and launch shape. The reference is computed on the CPU in
float64 and never uses the code under test.
"""

import pytest
import torch

from torchao import _lib
from torchao.dtypes.uintx.bitpacking import pack
from torchao.kernel.tuning import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
# one unit per row; segment boundaries inside groups; a group size that is no power of two (the
# multiply-high group index); an odd unit count and several waves along K with a row tail; a full
# line
SHAPES = [(5, 128, 32), (37, 384, 64), (37, 384, 48), (37, 2176, 128), (256, 4096, 64)]


def make(bits, N, K, g, M):
    gen = torch.Generator().manual_seed(bits * 1000 + N + K + M)
    codes = torch.randint(0, 2**bits, (N, K), generator=gen, dtype=torch.uint8)
    codes[0, : 2**bits] = torch.arange(2**bits, dtype=torch.uint8)
    zp = torch.randint(0, 2**bits, (N, K // g), generator=gen, dtype=torch.int32)
    scale = (2.0 ** torch.randint(0, 3, (N, K // g), generator=gen)).to(torch.bfloat16)
    x = torch.randint(-8, 9, (M, K), generator=gen).to(torch.bfloat16)
    bias = torch.randint(-64, 65, (N,), generator=gen).to(torch.bfloat16)
    w64 = (codes.double() - zp.double().repeat_interleave(g, 1)) * scale.double().repeat_interleave(g, 1)
    want = (x.double() @ w64.t()).to(torch.bfloat16)
    want_b = (want.float() + bias.float()).to(torch.bfloat16)
    shards = {w: None for w in (4, 2, 1)}
    for w, s in zip([w for w in (4, 2, 1) if bits & w], pack(codes, bits)):
        shards[w] = s.to(DEV)
    args = (shards[4], shards[2], shards[1], scale.to(DEV), zp.to(DEV), bits, g)
    return x.to(DEV), args, bias.to(DEV), want, want_b


def check(bits, N, K, g, M, kernel):
    x, args, bias, want, want_b = make(bits, N, K, g, M)
    for b, ref in ((None, want), (bias, want_b)):
        got = torch.ops.torchao.uintx_weight_only_linear(x, *args, b).cpu()
        assert _lib.lib().tao_last_kernel().decode() == kernel
        bad = (got != ref).nonzero()
        assert torch.equal(got, ref), (
            f"uint{bits} N={N} K={K} g={g} M={M} bias={b is not None}: {len(bad)} differ, first at "
            f"{bad[0].tolist()}: got {got[tuple(bad[0])].item()} want {ref[tuple(bad[0])].item()}")


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N,K,g", SHAPES)
@pytest.mark.parametrize("bits", range(1, 8))
def test_gemv(bits, N, K, g, M):
    with tuning(uintx=(1, 0, 0, 0, 0, 0, 0)):
        check(bits, N, K, g, M, "uintx_gemv_kernel")


@pytest.mark.parametrize("bits,N,K,g,M,rpw,wk,rg,unit", [
    (7, 37, 2176, 128, 1, 0, 0, 0, 4), (5, 37, 2176, 128, 3, 0, 0, 0, 8),
    (3, 37, 2176, 128, 8, 0, 0, 0, 16), (6, 256, 4096, 64, 1, 0, 0, 0, 16),
    (7, 37, 2176, 128, 1, 8, 1, 1, 8), (2, 37, 384, 64, 1, 2, 2, 4, 4),
    (6, 37, 2176, 128, 3, 0, 2, 2, 4),
])
def test_gemv_forced_units_and_launch_shapes(bits, N, K, g, M, rpw, wk, rg, unit):
    with tuning(uintx=(1, 0, rpw, wk, rg, unit, 0)):
        assert _lib.lib().tao_uintx_gemv_unit(M, K, bits) == unit  # the forced unit is what runs
        check(bits, N, K, g, M, "uintx_gemv_kernel")


@pytest.mark.parametrize("unit", [4, 8, 16])
@pytest.mark.parametrize("bits,N,K,g,M", [
    (2, 5, 128, 32, 4), (3, 37, 384, 48, 3), (6, 37, 2176, 128, 5), (7, 37, 2176, 128, 8),
    (5, 256, 4096, 64, 8),  # 64 KiB of x and the partials: past the default dynamic LDS limit
])
def test_gemv_x_staged_in_lds(bits, N, K, g, M, unit):
    with tuning(uintx=(1, 0, 0, 0, 0, unit, 2)):
        assert _lib.lib().tao_uintx_gemv_x_lds(M, K, bits) == 1
        check(bits, N, K, g, M, "uintx_gemv_kernel")
    with tuning(uintx=(1, 0, 0, 0, 0, unit, 1)):
        assert _lib.lib().tao_uintx_gemv_x_lds(M, K, bits) == 0
        check(bits, N, K, g, M, "uintx_gemv_kernel")


@pytest.mark.parametrize("bits", range(1, 8))
def test_route_boundary(bits):
    route = _lib.lib().tao_uintx_linear_route
    boundary = max(m for m in range(1, 10) if route(m, 37, 2176, bits) == 1)
    check(bits, 37, 2176, 128, boundary, "uintx_gemv_kernel")
    check(bits, 37, 2176, 128, boundary + 1, "uintx_dequant_kernel")
