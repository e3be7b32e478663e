"""Bit-exact GPU tests of the FP6 linear's MFMA route: the Fp6WO policy of gemm_mfma_kernel, reached
with tuning(fp6_mfma=1).

On the inputs of tests/exact_inputs_fp6.py every partial sum is an exact fp32 number, so the output
must equal bf16(fp32(sum * scale)) (+ bias -> bf16) of the float64 sum bit for bit whatever the
launch shape, k-group and split-K order. No tolerance: a mismatch is a kernel bug. The shapes are the
smallest at which this kernel can go wrong: M = 9 (a partial 16-row tile), 17 (a tile plus a row),
65 (a second M block at BM = 64); N = 37 (a partial column block and workgroup) and 256; K = 64
(less than one 256-code step), 320 (a step plus a 64-code tail), 2112 (eight steps plus a tail),
8256 (split-K territory, still inside the dense family's exactness bound).
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
BAR64 = 4e-3  # tests/test_gpu_fp6.py's bar for this linear against float64


@functools.lru_cache(maxsize=32)
def _inputs(fmt, family, M, N, K):
    seed = (M * 31 + N * 7 + K) % 1000
    codes, scale, bias, x = E.make_fp6_exact(fmt, M, N, K, seed, family)
    want = E.ref_fp6(fmt, x, codes, scale)
    return (x.to(DEV), E.pack_native(codes).to(DEV), scale.to(DEV), bias.to(DEV), want,
            E.add_bias(want, bias))


def check(what, fmt, M, N, K):
    """Both families, with and without bias, under the tuning the caller has set."""
    ebits, mbits = E.FORMATS[fmt]
    for family in E.FAMILIES:
        x, packed, scale, bias, want, want_b = _inputs(fmt, family, M, N, K)
        for b, ref in ((None, want), (bias, want_b)):
            got = torch.ops.torchao.fp6_weight_only_linear(x, packed, scale, ebits, mbits, b).cpu()
            kernel = _lib.lib().tao_last_kernel().decode()
            assert kernel == "gemm_mfma_kernel", (what, kernel)
            where = f"{what} {fmt} {family} M={M} N={N} K={K} bias={'on' if b is not None else 'off'}"
            assert got.shape == ref.shape, where
            assert torch.equal(got, ref), E.describe_mismatch(where, got, ref)


@pytest.mark.parametrize("N,K", [(37, 64), (37, 320), (256, 2112), (37, 8256)])
@pytest.mark.parametrize("M", (9, 17, 65))
@pytest.mark.parametrize("fmt", FMTS)
def test_mfma_route(fmt, M, N, K):
    with tuning(fp6_mfma=1):
        check("fp6 mfma", fmt, M, N, K)


@pytest.mark.parametrize("nw", (1, 2))
@pytest.mark.parametrize("splits", (1, 3))
@pytest.mark.parametrize("bm,kg", [(16, 1), (16, 2), (32, 2), (64, 1)])
def test_forced_launch_shapes(bm, kg, splits, nw):
    with tuning(gemm=(bm, kg, splits), gemm_nw=nw, fp6_mfma=1):
        for fmt in FMTS:
            check(f"fp6 mfma forced {bm}x{kg}x{splits} nw {nw}", fmt, 65, 37, 2112)


@pytest.mark.parametrize("M", (2, 8))
@pytest.mark.parametrize("fmt", FMTS)
def test_below_the_gemv_boundary(fmt, M):
    with tuning(fp6=(0, 1, 0, 0, 0, 0), fp6_mfma=1):  # the GEMV keeps one token only
        check("fp6 mfma, boundary 1", fmt, M, 37, 2112)


@pytest.mark.parametrize("fmt", FMTS)
def test_gaussian_weights(fmt):
    ebits, mbits = E.FORMATS[fmt]
    gen = torch.Generator().manual_seed(6)
    w = (torch.randn(256, 2112, generator=gen) * 0.02).to(E.BF16).to(DEV)
    x = torch.randn(48, 2112, generator=gen).to(E.BF16).to(DEV)
    codes, scale = torch.ops.torchao.fp6_quantize_rows(w, ebits, mbits)
    w_hat = torch.ops.torchao.fp6_dequantize(codes, scale, ebits, mbits)
    ref = x.double().cpu() @ w_hat.double().cpu().t()
    with tuning(fp6_mfma=1):
        y = torch.ops.torchao.fp6_weight_only_linear(x, codes, scale, ebits, mbits, None)
        assert _lib.lib().tao_last_kernel().decode() == "gemm_mfma_kernel"
    err = float((y.double().cpu() - ref).norm() / ref.norm())
    print(f"fp6 mfma {fmt} gaussian rel-L2 {err:.3e}")
    assert err <= BAR64, err
