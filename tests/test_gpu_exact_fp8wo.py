"""Bit-exact GPU tests of every route of torch.ops.torchao.fp8_weight_only_linear.

Same construction as test_gpu_exact_int8wo.py, on the inputs of tests/exact_inputs_fp8.py: every
product and partial sum is an exact fp32 number, so the output must equal
bf16(fp32(sum * scale)) (+ bias -> bf16) of the float64 sum bit for bit, for both input families
("dense": arbitrary fp32 scales; "probe": one wrong code at a probed k changes the bits).
No tolerance: a mismatch is a kernel bug.

Routes: the GEMV at M = 1..8 and under forced launch shapes, the MFMA kernel on its built-in and
forced tiles / K slices. The entry takes K % 32 == 0; the GEMV's K list (16, 1040, 8208, 16400)
is checked to be refused with its message and each K rounded up to a multiple of 32 runs in its
place. Each case asserts the route it meant to take through tao_last_kernel.
"""

import functools

import pytest
import torch

import exact_inputs_fp8 as E

from torchao import _lib
from torchao.kernel import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@functools.lru_cache(maxsize=16)
def _inputs(M, N, K, family):
    seed = (M * 31 + N * 7 + K) % 1000
    codes, scale, bias, x = E.make_fp8wo_exact(M, N, K, seed, family)
    want = E.ref_fp8wo(x, codes, scale)
    return (x.to(DEV), codes.view(FP8).to(DEV), scale.to(DEV), bias.to(DEV), want,
            E.add_bias(want, bias))


def _linear(x, w, scale, bias):
    return torch.ops.torchao.fp8_weight_only_linear(x, w, scale, bias)


def check(route, M, N, K, kernel):
    for family in E.FAMILIES:
        x, w, scale, bias, want, want_b = _inputs(M, N, K, family)
        for b, ref in ((None, want), (bias, want_b)):
            got = _linear(x, w, scale, b).cpu()
            assert kernel in _last_kernel(), (route, _last_kernel())
            where = f"{route} {family} M={M} N={N} K={K} bias={'on' if b is not None else 'off'}"
            assert got.shape == ref.shape, where
            assert torch.equal(got, ref), E.describe_mismatch(
                f"{where} kernel={_last_kernel()}", got, ref)


# ---- the GEMV -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", E.INT8_GEMV_K)
@pytest.mark.parametrize("N", E.INT8_GEMV_N)
@pytest.mark.parametrize("M", E.INT8_GEMV_M)
def test_gemv(M, N, K):
    with tuning(linear_crossover=8):  # (M > 4 would take the MFMA kernel)
        check("fp8 gemv", M, N, E.round_up(K, 32), "fp8wo_gemv")


@pytest.mark.parametrize("K", E.INT8_GEMV_K)
def test_k_not_a_multiple_of_32_is_refused(K):
    assert K % 32
    x = torch.zeros(1, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(37, K, dtype=torch.uint8, device=DEV).view(FP8)
    scale = torch.ones(37, device=DEV)
    for M in (1, 8, 48):
        with pytest.raises(RuntimeError, match="must be a multiple of 32"):
            _linear(x.expand(M, K), w, scale, None)


@pytest.mark.parametrize("rpw,wk,rg", E.INT8_GEMV_FORCED)
def test_gemv_forced_launch_shapes(rpw, wk, rg):
    with tuning(fp8_gemv=(rpw, wk, rg)):
        for K in E.INT8_GEMV_K:
            check(f"fp8 gemv forced rpw={rpw} wk={wk} g={rg}", 1, 37, E.round_up(K, 32),
                  "fp8wo_gemv")


# ---- the MFMA kernel ------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", E.MFMA_NK)
@pytest.mark.parametrize("M", E.INT8_MFMA_M)
def test_mfma_built_in_routing(M, N, K):
    check("fp8 mfma built-in", M, N, K, "gemm_mfma")


@pytest.mark.parametrize("bm,kg,splits", E.FORCED_TILES)
@pytest.mark.parametrize("M,N,K", E.FORCED_MNK)
def test_mfma_forced_tiles_and_split_k(bm, kg, splits, M, N, K):
    with tuning(gemm=(bm, kg, splits)):
        check(f"fp8 mfma bm={bm} kg={kg} splits={splits}", M, N, K, "gemm_mfma")


def test_mfma_k_tail_next_to_nan_codes():
    """K = 32 mod 128: the MFMA kernel's last step reads past the row into the next row's codes.
    With that next row all NaN codes (what an all-zero weight row quantizes to), only its own
    output column may be NaN."""
    M, N, K = 48, 72, 1056
    x, w, scale, bias, want, _ = _inputs(M, N, K, "dense")
    w2 = w.view(torch.uint8).clone()
    w2[5] = 0x7F
    w2[N - 1] = 0xFF
    got = _linear(x, w2.view(FP8), scale, None).cpu()
    assert "gemm_mfma" in _last_kernel()
    keep = [n for n in range(N) if n not in (5, N - 1)]
    assert bool(got[:, [5, N - 1]].isnan().all())
    assert torch.equal(got[:, keep], want[:, keep])
    with tuning(linear_crossover=8):  # and the GEMV's clamped tail lanes (K = 32 mod 1024)
        got = _linear(x[:3], w2.view(FP8), scale, None).cpu()
        assert "fp8wo_gemv" in _last_kernel()
    assert bool(got[:, [5, N - 1]].isnan().all())
    assert torch.equal(got[:, keep], want[:3, keep])
