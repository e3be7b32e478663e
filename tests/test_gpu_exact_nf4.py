"""Bit-exact GPU tests of every route of torch.ops.torchao.nf4_linear, and of the dequantizer.

On the inputs of tests/exact_inputs_nf4.py every block scaler is a power of two, every w^ a
shifted level and every partial sum an exact fp32 number, so the output must equal bf16(sum)
(+ bias -> bf16) of the float64 sum bit for bit, whatever the route and launch shape. No
tolerance: a mismatch is a kernel bug.

Routes: the GEMV at M = 1..8, under forced launch shapes (one of which clamps) and forced beyond
8 tokens (a sequence of 8-token launches), a K tail next to non-finite scalers included;
dequantize + bf16 matmul at M = 130, at M = 3 and on both sides of the built-in boundary. Each
case asserts the route it meant to take through tao_last_kernel.
"""

import functools

import pytest
import torch

import exact_inputs_nf4 as E

from torchao import _lib
from torchao.kernel import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@functools.lru_cache(maxsize=16)
def _inputs(M, N, K):
    seed = (M * 31 + N * 7 + K) % 1000
    codes, qs, qf, mean, levels, bias, x = E.make_nf4_exact(M, N, K, seed)
    want = E.ref_nf4(x, codes, qs, qf, mean, levels, N)
    parts = tuple(t.to(DEV) for t in (codes, qs, qf, mean, levels))
    return x.to(DEV), parts, bias.to(DEV), want, E.add_bias(want, bias)


def check(route, M, N, K, kernel):
    x, parts, bias, want, want_b = _inputs(M, N, K)
    for b, ref in ((None, want), (bias, want_b)):
        got = torch.ops.torchao.nf4_linear(x, *parts, N, b).cpu()
        if kernel is not None:
            assert kernel in _last_kernel(), (route, _last_kernel())
        where = f"{route} M={M} N={N} K={K} bias={'on' if b is not None else 'off'}"
        assert got.shape == ref.shape, where
        assert torch.equal(got, ref), E.describe_mismatch(
            f"{where} kernel={_last_kernel()}", got, ref)


@pytest.mark.parametrize("K", E.GEMV_K)
@pytest.mark.parametrize("N", E.GEMV_N)
@pytest.mark.parametrize("M", E.GEMV_M)
def test_gemv(M, N, K):
    with tuning(nf4=(1, 0, 0, 0, 0)):  # (M > 4 would dequantize + matmul)
        check("nf4 gemv", M, N, K, "nf4_gemv_kernel")


@pytest.mark.parametrize("route,M,kernel", [(1, 3, "nf4_gemv_kernel"), (1, 8, "nf4_gemv_kernel"),
                                            (2, 16, "nf4_dequant_kernel")])
def test_k_tail_next_to_non_finite_scalers(route, M, kernel):
    """K = 320: the GEMV's tail lanes load clamped chunks and scalers of their own row's end. With the second group's factor 0 (blocks 256.. have scalers
    +-inf: rows 52.. and the end of row 51) only those rows' outputs may be non-finite; rows 0..50
    must still equal the formula bit for bit."""
    N, K = 60, 320
    codes, qs, qf, mean, levels, bias, x = E.make_nf4_exact(M, N, K, 11)
    want = E.ref_nf4(x, codes, qs, qf, mean, levels, N)
    assert qf.numel() == 2 and (50 * 5 + 4) < 256 <= 51 * 5 + 4
    qf = qf.clone()
    qf[1] = 0
    parts = tuple(t.to(DEV) for t in (codes, qs, qf, mean, levels))
    with tuning(nf4=(route, 0, 0, 0, 0)):
        got = torch.ops.torchao.nf4_linear(x.to(DEV), *parts, N, None).cpu()
    assert kernel in _last_kernel()
    assert torch.equal(got[:, :51], want[:, :51]), E.describe_mismatch(
        f"route {route} next to inf scalers", got[:, :51], want[:, :51])
    assert not bool(got[:, 52:].isfinite().any())


@pytest.mark.parametrize("rpw,wk,rg", E.GEMV_FORCED)
def test_gemv_forced_launch_shapes(rpw, wk, rg):
    with tuning(nf4=(1, 0, rpw, wk, rg)):
        for M, N, K in ((1, 37, 4160), (1, 37, 128), (3, 37, 4160), (8, 37, 1088)):
            check(f"nf4 gemv forced {rpw}x{wk}x{rg}", M, N, K, "nf4_gemv_kernel")


def test_gemv_forced_beyond_eight_tokens():
    with tuning(nf4=(1, 0, 0, 0, 0)):
        check("nf4 gemv forced, 8 + 8 + 1 tokens", 17, 37, 1088, "nf4_gemv_kernel")


def test_dequant_mm():
    with tuning(nf4=(2, 0, 0, 0, 0)):
        check("nf4 dequant + mm forced", 130, 37, 1088, None)
        check("nf4 dequant + mm forced", 3, 37, 1088, None)


def test_route_boundary():
    lib = _lib.lib()
    route = lib.tao_nf4_linear_route
    assert [route(m, 37, 1088) for m in (1, 4, 5, 8, 4096)] == [1, 1, 2, 2, 2]
    M = 9
    codes, qs, qf, mean, levels, bias, x = E.make_nf4_exact(M, 37, 1088, 3)
    want = E.ref_nf4(x, codes, qs, qf, mean, levels, 37)
    parts = tuple(t.to(DEV) for t in (codes, qs, qf, mean, levels))
    for m, kernel in ((4, "nf4_gemv_kernel"), (5, "nf4_dequant_kernel"), (9, "nf4_dequant_kernel")):
        got = torch.ops.torchao.nf4_linear(x[:m].to(DEV), *parts, 37, None)
        assert _last_kernel() == kernel
        assert torch.equal(got.cpu(), want[:m])
    with tuning(nf4=(0, 2, 0, 0, 0)):  # the GEMV boundary moved to 2 tokens
        assert route(2, 37, 1088) == 1 and route(3, 37, 1088) == 2
    assert route(3, 37, 1088) == 1
    with tuning(nf4=(0, 8, 0, 0, 0)):  # ... and to the GEMV's largest launch
        got = torch.ops.torchao.nf4_linear(x[:8].to(DEV), *parts, 37, None)
        assert _last_kernel() == "nf4_gemv_kernel" and torch.equal(got.cpu(), want[:8])


@pytest.mark.parametrize("N,K", [(1, 64), (37, 1088), (37, 4160)])
def test_dequantize(N, K):
    x, parts, bias, want, _ = _inputs(1, N, K)
    codes, qs, qf, mean, levels = (t.cpu() for t in parts)
    w = torch.ops.torchao.nf4_dequantize(*parts, [N, K])
    assert _last_kernel() == "nf4_dequant_kernel"
    assert w.dtype is torch.bfloat16 and w.shape == (N, K)
    assert torch.equal(w.cpu().double(), E.dequant64(codes, qs, qf, mean, levels, (N, K)))
