"""Bit-exact GPU tests of every route of torch.ops.torchao.fp6_weight_only_linear, and of the
dequantizer.

On the inputs of tests/exact_inputs_fp6.py every partial sum is an exact fp32 number, so the
output must equal bf16(fp32(sum * scale)) (+ bias -> bf16) of the float64 sum bit for bit, whatever
the route and launch shape. No tolerance: a mismatch is a kernel bug.

Routes: the GEMV at M = 1..8 for both formats and families, under forced launch shapes with both
lane-chunk sizes and forced beyond 8 tokens (a sequence of 8-token launches); dequantize + bf16
matmul at M = 9 and 48 on the dense family. Each case asserts the route it meant to take through
tao_last_kernel.
"""

import functools

import pytest
import torch

import exact_inputs_fp6 as E

from torchao import _lib
from torchao.kernel.tuning import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = sorted(E.FORMATS)


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@functools.lru_cache(maxsize=32)
def _inputs(fmt, family, M, N, K, pow2=False):
    seed = (M * 31 + N * 7 + K) % 1000
    codes, scale, bias, x = E.make_fp6_exact(fmt, M, N, K, seed, family, pow2_scale=pow2)
    want = E.ref_fp6(fmt, x, codes, scale)
    return (x.to(DEV), E.pack_native(codes).to(DEV), scale.to(DEV), bias.to(DEV), want,
            E.add_bias(want, bias))


def check(route, fmt, family, M, N, K, kernel, pow2=False):
    x, packed, scale, bias, want, want_b = _inputs(fmt, family, M, N, K, pow2)
    ebits, mbits = E.FORMATS[fmt]
    for b, ref in ((None, want), (bias, want_b)):
        got = torch.ops.torchao.fp6_weight_only_linear(x, packed, scale, ebits, mbits, b).cpu()
        assert _last_kernel() == kernel, (route, _last_kernel())
        where = f"{route} {fmt} {family} M={M} N={N} K={K} bias={'on' if b is not None else 'off'}"
        assert got.shape == ref.shape, where
        assert torch.equal(got, ref), E.describe_mismatch(
            f"{where} kernel={_last_kernel()}", got, ref)


@pytest.mark.parametrize("K", E.GEMV_K)
@pytest.mark.parametrize("N", E.GEMV_N)
@pytest.mark.parametrize("M", E.GEMV_M)
@pytest.mark.parametrize("fmt", FMTS)
def test_gemv(fmt, M, N, K):
    with tuning(fp6=(1, 0, 0, 0, 0, 0)):
        for family in E.FAMILIES:
            check("fp6 gemv", fmt, family, M, N, K, "fp6wo_gemv_kernel")


@pytest.mark.parametrize("rpw,wk,rg,grp", E.GEMV_FORCED)
@pytest.mark.parametrize("fmt", FMTS)
def test_gemv_forced_launch_shapes(fmt, rpw, wk, rg, grp):
    with tuning(fp6=(1, 0, rpw, wk, rg, grp)):
        for M, N, K in ((1, 37, 4160), (1, 37, 64), (3, 37, 2112), (8, 37, 8256)):
            for family in E.FAMILIES:
                check(f"fp6 gemv forced {rpw}x{wk}x{rg} chunk {grp}", fmt, family, M, N, K,
                      "fp6wo_gemv_kernel")


@pytest.mark.parametrize("grp", (1, 2))
@pytest.mark.parametrize("fmt", FMTS)
def test_gemv_both_chunk_sizes(fmt, grp):
    with tuning(fp6=(1, 0, 0, 0, 0, grp)):
        for M in (1, 2, 4, 8):
            for K in E.GEMV_K:
                check(f"fp6 gemv chunk {grp}", fmt, "probe", M, 37, K, "fp6wo_gemv_kernel")


@pytest.mark.parametrize("fmt", FMTS)
def test_gemv_forced_beyond_eight_tokens(fmt):
    with tuning(fp6=(1, 0, 0, 0, 0, 0)):
        check("fp6 gemv forced, 8 + 8 + 1 tokens", fmt, "dense", 17, 37, 2112, "fp6wo_gemv_kernel")


@pytest.mark.parametrize("M", E.MM_M)
@pytest.mark.parametrize("fmt", FMTS)
def test_dequant_mm(fmt, M):
    """The matmul sums over the dequantized weight: power-of-two scales keep that weight, and with
    it the sum, exact (exact_inputs_fp6's header)."""
    with tuning(fp6=(2, 0, 0, 0, 0, 0)):
        for N, K in ((37, 2112), (256, 4160)):
            check("fp6 dequant + mm forced", fmt, "dense", M, N, K, "fp6_dequant_kernel", pow2=True)


def test_route_boundary():
    route = _lib.lib().tao_fp6_linear_route
    boundary = max(m for m in range(1, 10) if route(m, 37, 2112) == 1)
    assert 1 <= boundary <= 8
    check("fp6 at the boundary", "e3m2", "dense", boundary, 37, 2112, "fp6wo_gemv_kernel", pow2=True)
    check("fp6 above the boundary", "e3m2", "dense", boundary + 1, 37, 2112, "fp6_dequant_kernel",
          pow2=True)
    with tuning(fp6=(0, 2, 0, 0, 0, 0)):  # the GEMV boundary moved to 2 tokens
        check("fp6 boundary 2", "e2m3", "dense", 2, 37, 2112, "fp6wo_gemv_kernel", pow2=True)
        check("fp6 boundary 2", "e2m3", "dense", 3, 37, 2112, "fp6_dequant_kernel", pow2=True)


@pytest.mark.parametrize("N,K", [(1, 64), (37, 2112), (256, 4160)])
@pytest.mark.parametrize("fmt", FMTS)
def test_dequantize(fmt, N, K):
    ebits, mbits = E.FORMATS[fmt]
    for family in E.FAMILIES:
        codes, scale, _, _ = E.make_fp6_exact(fmt, 1, N, K, 5, family)
        w = torch.ops.torchao.fp6_dequantize(E.pack_native(codes).to(DEV), scale.to(DEV), ebits,
                                             mbits)
        assert _last_kernel() == "fp6_dequant_kernel"
        assert w.dtype is torch.bfloat16 and w.shape == (N, K)
        assert torch.equal(w.cpu().double(), E.dequant64(fmt, codes, scale))
