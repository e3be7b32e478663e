"""Bit-exact GPU tests of every route of torch.ops.torchao.int8_weight_only_linear.

Same construction as test_gpu_exact_int4.py (tests/exact_inputs.py): integer x in [-4, 4] against
int8 weights gives integer products and partial sums below K * 4 * 128 < 2^24, exact in fp32 in any
order, so the output must equal bf16(bf16(sum) * scale) (+ bias -> bf16) of the float64 sum bit
for bit, for arbitrary bf16 scales and biases. No tolerance: a mismatch is a kernel bug.

Routes: the GEMV at M = 1..8 and under forced launch shapes, the MFMA kernel on its built-in and
forced tiles / K slices, the weight-shared tile kernel. The public entry takes K % 32 == 0; the
GEMV's K list (16, 1040, 8208, 16400: each ends in a half 32-k chunk) is therefore checked to be
refused there with its message, run through the one-token decode entry (which takes K % 16 == 0,
M = 1), and each K rounded up to a multiple of 32 runs through the linear in its place.
"""

import functools

import pytest
import torch

import exact_inputs as E

from torchao import _lib
from torchao.kernel import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@functools.lru_cache(maxsize=8)
def _inputs(M, N, K):
    seed = (M * 31 + N * 7 + K) % 1000
    w, scale, bias, x = E.make_int8wo_exact(M, N, K, seed)
    want = E.ref_int8wo(x, w, scale)
    return x.to(DEV), w.to(DEV), scale.to(DEV), bias.to(DEV), want, E.add_bias(want, bias)


def _linear(x, w, scale, bias):
    return torch.ops.torchao.int8_weight_only_linear(x, w, scale, bias)


def check(route, M, N, K, run=_linear, with_bias=True):
    x, w, scale, bias, want, want_b = _inputs(M, N, K)
    for b, ref in ((None, want), (bias, want_b)) if with_bias else ((None, want),):
        got = run(x, w, scale, b).cpu()
        where = f"{route} M={M} N={N} K={K} bias={'on' if b is not None else 'off'}"
        assert got.shape == ref.shape, where
        assert torch.equal(got, ref), E.describe_mismatch(f"{where} kernel={_last_kernel()}",
                                                          got, ref)


# ---- the GEMV -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", E.INT8_GEMV_K)
@pytest.mark.parametrize("N", E.INT8_GEMV_N)
@pytest.mark.parametrize("M", E.INT8_GEMV_M)
def test_gemv(M, N, K):
    with tuning(linear_crossover=8):  # (M > 4 would take the MFMA kernel)
        if K % 32:
            x, w, scale, bias, _, _ = _inputs(M, N, K)
            with pytest.raises(RuntimeError, match="must be a multiple of 32"):
                _linear(x, w, scale, None)
        check("int8 gemv", M, N, E.round_up(K, 32))
        assert "gemv" in _last_kernel()


@pytest.mark.parametrize("K", E.INT8_GEMV_K)
@pytest.mark.parametrize("N", E.INT8_GEMV_N)
def test_decode_entry_takes_half_chunk_k(N, K):
    """K = 16 mod 32 at M = 1 through tao_int8wo_decode_bf16 (no norm, no epilogue, no bias): the
    last 16-k chunk of every row is a half 32-k chunk."""
    from torchao._models.llama import kernels

    check("int8wo_decode", 1, N, K, with_bias=False,
          run=lambda x, w, scale, b: kernels.int8wo_decode(x, w, scale))


@pytest.mark.parametrize("rpw,wk,rg", E.INT8_GEMV_FORCED)
def test_gemv_forced_launch_shapes(rpw, wk, rg):
    with tuning(int8_gemv=(rpw, wk, rg)):
        for K in E.INT8_GEMV_K:
            check(f"int8 gemv forced rpw={rpw} wk={wk} g={rg}", 1, 37, E.round_up(K, 32))
            assert "gemv" in _last_kernel()


@pytest.mark.parametrize("K", [8224, 16416])  # 9 and 17 slices: 8 waves along K
@pytest.mark.parametrize("rpw,wk,rg", [(4, 0, 8), (2, 0, 2)])
def test_gemv_row_groups_clamped_to_the_workgroup(rpw, wk, rg, K):
    """A tuning with waves_k = 0 passes tao_tune_int8_gemv whatever its row_groups, and the built-in
    waves along K (min(slices, 8) here) times those row groups can exceed the 8 waves of a
    workgroup: every int8 GEMV launcher halves the row groups until the workgroup fits, so the
    linear runs (and stays exact) instead of failing its launch."""
    from torchao._models.llama import kernels

    with tuning(int8_gemv=(rpw, wk, rg)):
        check(f"int8 gemv clamped rpw={rpw} wk={wk} g={rg}", 1, 37, K)
        assert "gemv" in _last_kernel()
        check(f"int8wo_decode clamped rpw={rpw} wk={wk} g={rg}", 1, 37, K, with_bias=False,
              run=lambda x, w, scale, b: kernels.int8wo_decode(x, w, scale))


@pytest.mark.parametrize("rpw,wk,rg", [(4, 0, 8), (2, 0, 2)])
def test_int8dq_row_groups_clamped_to_the_workgroup(rpw, wk, rg):
    """The same two tunings through the int8 dynamic-activation fused entry (its launcher makes
    (4, 0, 8) 4 waves along K x 8 row groups at 9 slices) against its unfused chain on the built-in
    shape: the int32 sums are exact, so any launch shape gives the same bits."""
    import torch.nn as nn
    from torchao._models.llama import kernels
    from torchao._models.llama.model import _int8dq_parts
    from torchao.quantization import Int8DynamicActivationInt8WeightConfig, quantize_

    K = 8224
    torch.manual_seed(K)
    lin = nn.Linear(K, 38, bias=False, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.uniform_(-1 / K ** 0.5, 1 / K ** 0.5)
    quantize_(lin, Int8DynamicActivationInt8WeightConfig())
    parts = _int8dq_parts(lin)
    assert parts is not None
    x = torch.randn(1, 1, K, device=DEV, dtype=torch.bfloat16)
    want_plain = lin(x)
    # (the unfused SiLU-mul kernel takes an even number of outputs: run it on the 38 rows twice)
    want_swiglu = kernels.silu_mul(torch.cat([want_plain, want_plain], -1))[..., :19]
    with tuning(int8_gemv=(rpw, wk, rg)):
        assert torch.equal(kernels.int8dq_decode(x, *parts), want_plain)
        assert torch.equal(kernels.int8dq_decode(x, *parts, epilogue="swiglu"), want_swiglu)


# ---- the MFMA kernel ------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", E.MFMA_NK)
@pytest.mark.parametrize("M", E.INT8_MFMA_M)
def test_mfma_built_in_routing(M, N, K):
    check("int8 mfma built-in", M, N, K)
    assert "gemm_mfma" in _last_kernel()


@pytest.mark.parametrize("bm,kg,splits", E.FORCED_TILES)
@pytest.mark.parametrize("M,N,K", E.FORCED_MNK)
def test_mfma_forced_tiles_and_split_k(bm, kg, splits, M, N, K):
    with tuning(gemm=(bm, kg, splits)):
        check(f"int8 mfma bm={bm} kg={kg} splits={splits}", M, N, K)


# ---- the weight-shared tile kernel ------------------------------------------------------------------------

@pytest.mark.parametrize("splits", E.INT8_TILE_SPLITS)
@pytest.mark.parametrize("M,N,K", E.TILE_MNK)
def test_tile_kernel(splits, M, N, K):
    with tuning(gemm_tile=(2, splits)):
        check(f"int8 tile splits={splits}", M, N, K)
        assert "tile" in _last_kernel()
