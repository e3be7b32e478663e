"""Bit-exact GPU tests of every route of torch.ops.torchao.fp8_scaled_mm and of the fused
one-token torch.ops.torchao.fp8_dyn_linear.

On the inputs of tests/exact_inputs_fp8dyn.py every product and partial sum is an exact fp32 number
inside the matrix instruction's own exact window, so the output must equal
bf16(fp32(fp32(sum * xs) * ws) + bias) of the float64 sum bit for bit, for both input families
("dense": arbitrary fp32 scales; "probe": one wrong code at a probed k changes the bits, which is
what settles the operand lane map of v_mfma_scale_f32_16x16x128_f8f6f4: x and w are unrelated
random data, so a k permutation that differed between the operands would show). No tolerance: a
mismatch is a kernel bug. Each case asserts the route it meant to take through tao_last_kernel.
"""

import functools

import pytest
import torch

import exact_inputs_fp8dyn as E

from torchao import _lib
from torchao.kernel import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
MFMA, GEMV = "gemm_mfma", "fp8dyn_gemv"


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@functools.lru_cache(maxsize=32)
def _inputs(M, N, K, family):
    seed = (M * 31 + N * 7 + K) % 1000
    xq, xs, wq, ws, bias = E.make_fp8dyn_exact(M, N, K, seed, family)
    want = E.ref_fp8dyn(xq, xs, wq, ws)
    want_b = E.ref_fp8dyn(xq, xs, wq, ws, bias)
    return (xq.view(FP8).to(DEV), xs.to(DEV), wq.view(FP8).to(DEV), ws.to(DEV), bias.to(DEV),
            want, want_b)


def _mm(xq, xs, wq, ws, bias):
    return torch.ops.torchao.fp8_scaled_mm(xq, xs, wq, ws, bias)


def check(route, M, N, K, kernel):
    for family in E.FAMILIES:
        xq, xs, wq, ws, bias, want, want_b = _inputs(M, N, K, family)
        for b, ref in ((None, want), (bias, want_b)):
            got = _mm(xq, xs, wq, ws, b).cpu()
            assert kernel in _last_kernel(), (route, _last_kernel())
            where = f"{route} {family} M={M} N={N} K={K} bias={'on' if b is not None else 'off'}"
            assert got.shape == ref.shape, where
            assert torch.equal(got, ref), E.describe_mismatch(
                f"{where} kernel={_last_kernel()}", got, ref)


# ---- the MFMA kernel ------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", E.MFMA_K)
@pytest.mark.parametrize("N", E.MFMA_N)
def test_mfma_every_m(N, K):
    """Built-in tiles; the MFMA route at every M (below the crossover too)."""
    with tuning(fp8dyn_mfma=1):
        for M in E.MFMA_M:
            check("fp8dyn mfma", M, N, K, MFMA)


def test_mfma_is_the_built_in_route_above_the_crossover():
    for M in (5, 16, 33):
        check("fp8dyn mfma built-in", M, 37, 272, MFMA)


@pytest.mark.parametrize("bm,kg,splits", E.FORCED_TILES)
def test_mfma_forced_tiles_and_split_k(bm, kg, splits):
    with tuning(gemm=(bm, kg, splits), fp8dyn_mfma=1):
        for M, N, K in E.FORCED_MNK:
            check(f"fp8dyn mfma bm={bm} kg={kg} splits={splits}", M, N, K, MFMA)


@pytest.mark.parametrize("K", (272, 1040, 112))
def test_k_tail_next_to_nan_codes(K):
    """The last step reads past the row into the next row's codes, on both operands. With the
    next token / weight row all NaN codes (what an all-zero row quantises to), only its own output
    row / column may be NaN: both operands are zeroed past K (NaN * 0 is NaN)."""
    M, N = 33, 37
    xq, xs, wq, ws, bias, want, _ = _inputs(M, N, K, "dense")
    x2 = xq.view(torch.uint8).clone()
    w2 = wq.view(torch.uint8).clone()
    x2[3], x2[M - 1] = 0x7F, 0xFF
    w2[5], w2[N - 1] = 0x7F, 0xFF
    rows = [m for m in range(M) if m not in (3, M - 1)]
    cols = [n for n in range(N) if n not in (5, N - 1)]

    def verify(got, m_rows, tag):
        nan = got.isnan()
        assert bool(nan[:, [5, N - 1]].all()), tag
        fin = got[m_rows][:, cols]
        assert not bool(fin.isnan().any()), f"{tag}: a NaN code past the K tail reached the sum"
        assert torch.equal(fin, want[m_rows][:, cols]), tag

    with tuning(fp8dyn_mfma=1):
        got = _mm(x2.view(FP8), xs, w2.view(FP8), ws, None).cpu()
        assert MFMA in _last_kernel()
    assert bool(got[[3, M - 1]].isnan().all())
    verify(got, rows, "mfma")
    with tuning(linear_crossover=8):  # and the GEMV's clamped tail lanes
        got = _mm(x2.view(FP8)[:5], xs[:5], w2.view(FP8), ws, None).cpu()
        assert GEMV in _last_kernel()
    assert bool(got[3].isnan().all())
    verify(got, [0, 1, 2, 4], "gemv")


# ---- the GEMV -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", E.GEMV_K)
@pytest.mark.parametrize("N", E.GEMV_N)
def test_gemv(N, K):
    with tuning(linear_crossover=8):
        for M in E.GEMV_M:
            check("fp8dyn gemv", M, N, K, GEMV)


@pytest.mark.parametrize("rpw,wk,rg", E.GEMV_FORCED)
def test_gemv_forced_launch_shapes(rpw, wk, rg):
    with tuning(fp8_gemv=(rpw, wk, rg)):
        for K in E.GEMV_K:
            check(f"fp8dyn gemv forced rpw={rpw} wk={wk} g={rg}", 1, 37, K, GEMV)


def test_crossover_moved_both_ways():
    """Each M near the built-in crossover (GEMV up to M = 2, and M <= 4 on small weights) runs on
    both kernels and gives the same bits."""
    N, K = 37, 1040
    for M in (1, 2, 3, 4, 5, 8):
        with tuning(linear_crossover=8):
            check("crossover 8", M, N, K, GEMV)
        if M > 1:
            with tuning(linear_crossover=1):
                check("crossover 1", M, N, K, MFMA)
    check("built-in", 2, N, K, GEMV)
    check("built-in", 5, N, K, MFMA)


# ---- the fused one-token launch --------------------------------------------------------------------------

@pytest.mark.parametrize("K", E.GEMV_K)
@pytest.mark.parametrize("N", (37, 80))
def test_fused_one_token_equals_quantize_then_scaled_mm(N, K):
    for seed in (1, 2, 6):
        xb, codes, scale, wq, ws, bias = E.make_identity_token(N, K, seed + K % 5)
        x, w, wsd, b = xb.to(DEV), wq.view(FP8).to(DEV), ws.to(DEV), bias.to(DEV)
        q, s = torch.ops.torchao.fp8_quantize_rows(x)
        assert torch.equal(q.view(torch.uint8).cpu(), codes) and torch.equal(s.cpu().reshape(-1), scale)
        for bb in (None, b):
            two = _mm(q, s, w, wsd, bb)
            assert GEMV in _last_kernel()
            one = torch.ops.torchao.fp8_dyn_linear(x, w, wsd, bb)
            assert GEMV in _last_kernel()
            assert torch.equal(one, two)
            ref = E.ref_fp8dyn(codes, scale, wq, ws, None if bb is None else bias)
            assert torch.equal(one.cpu(), ref), E.describe_mismatch(f"fused N={N} K={K}", one.cpu(), ref)


@pytest.mark.parametrize("rpw,wk,rg", E.GEMV_FORCED)
def test_fused_one_token_forced_launch_shapes(rpw, wk, rg):
    for K in E.GEMV_K:
        xb, codes, scale, wq, ws, bias = E.make_identity_token(37, K, 3)
        ref = E.ref_fp8dyn(codes, scale, wq, ws, bias)
        with tuning(fp8_gemv=(rpw, wk, rg)):
            got = torch.ops.torchao.fp8_dyn_linear(xb.to(DEV), wq.view(FP8).to(DEV), ws.to(DEV),
                                                   bias.to(DEV)).cpu()
            assert GEMV in _last_kernel()
        assert torch.equal(got, ref), E.describe_mismatch(f"fused forced K={K}", got, ref)
