"""The byte-weight weight-only decode kernel shared by int8 and float8 (wo8_decode_kernel in
csrc/tao_gemv.h, behind tao_int8wo_decode_bf16 / tao_fp8wo_decode_bf16): the RMSNorm prologue at
1, 2 and 4 pieces per thread, live tail lanes and the three epilogues, under forced launch shapes.

The bar is equality. The call with the norm fused must equal kernels.rmsnorm followed by the same
wrapper without the norm under the same forced shape: x is made of integers in [-8, 8] times a
power of two (test_gpu_decode_fused_fp8._norm_inputs), so the sum of squares is an exact fp32
number in any order and the normalised bf16 token is bit-identical on both sides; with all three
tuning values forced and a K that adds no row group, both calls use one launch shape and one slice
order, so the dot products are the same fp32 sums.

K = 480, 992, 2016: multiples of 32 that do not fill their last slice (tail lanes live); with one
wave they take 1, 2 and 4 pieces per thread; (4, 2, 2) at K = 2016 has two waves along K (the
cross-wave sum of squares and wg_combine).
"""

import functools

import pytest
import torch

from test_gpu_decode_fused_fp8 import _caches, _freqs, _norm_inputs

from torchao import _lib
from torchao.kernel import tuning

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
EPS = 1e-5
SHAPES = ((2, 1, 1), (4, 1, 1), (8, 1, 1), (4, 2, 2))  # (rows per wave, waves along K, groups)
KS = (480, 992, 2016)
H = HKV = 4
D, T, POS = 128, 64, 17
N_OF = {"none": 37, "swiglu": 38, "rope_kv": (H + 2 * HKV) * D}


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@functools.lru_cache(maxsize=None)
def _weights(fmt, N, K):
    """(w [N, K], scale [N]) as the format's kernel reads them; made once, left unchanged."""
    g = torch.Generator().manual_seed(N * 31 + K)
    if fmt == "int8wo":
        w = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8)
        s = (torch.rand(N, generator=g) * 0.01 + 0.001).to(BF16)
    else:
        w = (torch.randn(N, K, generator=g) * 0.05).to(torch.float8_e4m3fn)  # finite codes
        s = torch.rand(N, generator=g) * 0.5 + 0.25
    return w.to(DEV), s.to(DEV)


def _fn(fmt):
    from torchao._models.llama import kernels

    return kernels.int8wo_decode if fmt == "int8wo" else kernels.fp8wo_decode


def _run(fmt, x, w, s, nw, epilogue):
    """(output, k cache, v cache) of one call; fresh caches from one seed for rope_kv."""
    kw = {} if nw is None else dict(norm_weight=nw, eps=EPS)
    if epilogue != "rope_kv":
        y = _fn(fmt)(x, w, s, epilogue=epilogue, **kw)
        assert f"{fmt}_decode" in _last_kernel(), _last_kernel()
        return y, None, None
    kc, vc = _caches(HKV, T, seed=3)
    p = torch.tensor([POS], device=DEV)
    y = _fn(fmt)(x, w, s, epilogue=epilogue, rope=(_freqs(H, HKV, T), p, kc, vc, H), **kw)
    assert f"{fmt}_decode" in _last_kernel(), _last_kernel()
    return y, kc, vc


@pytest.mark.parametrize("epilogue", ["none", "swiglu", "rope_kv"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmt", ["int8wo", "fp8wo"])
def test_fused_norm_equals_rmsnorm_then_plain(fmt, shape, epilogue):
    from torchao._models.llama import kernels

    N = N_OF[epilogue]
    knob = "int8_gemv" if fmt == "int8wo" else "fp8_gemv"
    for K in KS:
        w, s = _weights(fmt, N, K)
        x, nw = _norm_inputs(K)
        with tuning(**{knob: shape}):
            got = _run(fmt, x, w, s, nw, epilogue)
            ref = _run(fmt, kernels.rmsnorm(x, nw, EPS), w, s, None, epilogue)
        assert got[0].shape == ref[0].shape
        assert bool(ref[0].float().abs().sum() > 0)
        for a, b, what in zip(got, ref, ("output", "k cache", "v cache")):
            if a is None:
                continue
            diff = int((a != b).sum())
            print(f"{fmt} {shape} {epilogue} K={K} {what}: {diff} of {a.numel()} differ")
            assert torch.equal(a, b), (K, what, diff)
    kernels.check_decode_status()


def test_int8wo_norm_past_the_prologue_limit_runs_as_its_own_launch():
    """K = 16400 > 16384 (512 threads x 4 pieces x 8) with a norm weight: the wrapper runs
    rmsnorm as its own launch and the fused kernel without the norm, instead of raising."""
    from torchao._models.llama import kernels

    N, K = 37, 16400
    w, s = _weights("int8wo", N, K)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 1, K, generator=g).to(BF16).to(DEV)
    nw = (torch.rand(K, generator=g) + 0.5).to(BF16).to(DEV)
    got = kernels.int8wo_decode(x, w, s, norm_weight=nw, eps=EPS)
    assert "int8wo_decode" in _last_kernel()
    ref = kernels.int8wo_decode(kernels.rmsnorm(x, nw, EPS), w, s)
    assert got.shape == (1, 1, N) and bool(ref.float().abs().sum() > 0)
    assert torch.equal(got, ref)
