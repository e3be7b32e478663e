"""Bit-exact GPU tests of the uintx linear's MFMA route: the UintxWO policy of gemm_mfma_kernel,
reached with tuning(uintx_mfma=1).

The construction of tests/test_gpu_exact_uintx.py: integer x in [-8, 8], scales 1, 2, 4, every code
present, arbitrary in-range zero points, so every partial sum is an exact fp32 number for K <= 4096
and the output must equal the float64 formula rounded once (with a bias: rounded, added in fp32,
rounded again) under torch.equal. The kernel's own intermediates are exact too: an MFMA's product
against 128 + q is at most 32 * 8 * 255 and its zero-point correction is applied per group. The
shapes: one partial step and a partial column block; K / 8 an odd multiple of 16 (the odd segments'
shifted windows) with a served and an unserved group size; 8.5 steps; 16 steps, four column tiles,
split-K. M: a partial tile, a full one, two tiles and a row, a third 64-row block.
"""

import functools

import pytest
import torch

from test_gpu_exact_uintx import SHAPES, make

from torchao import _lib
from torchao.kernel.tuning import tuning

pytestmark = pytest.mark.gpu
KERNEL = {2: "uintx_dequant_kernel", 3: "gemm_mfma_kernel"}
inputs = functools.lru_cache(maxsize=None)(make)


def last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def check(bits, N, K, g, M, kernel):
    x, args, bias, want, want_b = inputs(bits, N, K, g, M)
    for b, ref in ((None, want), (bias, want_b)):
        got = torch.ops.torchao.uintx_weight_only_linear(x, *args, b).cpu()
        assert last_kernel() == kernel
        bad = (got != ref).nonzero()
        assert torch.equal(got, ref), (
            f"uint{bits} N={N} K={K} g={g} M={M} bias={b is not None}: {len(bad)} differ, first at "
            f"{bad[0].tolist()}: got {got[tuple(bad[0])].item()} want {ref[tuple(bad[0])].item()}")


@pytest.mark.parametrize("M", [9, 16, 33, 130])
@pytest.mark.parametrize("N,K,g", SHAPES)
@pytest.mark.parametrize("bits", range(1, 8))
def test_mfma_route(bits, N, K, g, M):
    with tuning(uintx_mfma=1):
        route = _lib.lib().tao_uintx_linear_route_g(M, N, K, bits, g)
        assert route == (3 if g % 32 == 0 else 2)  # g = 48: the documented fallback
        check(bits, N, K, g, M, KERNEL[route])


def test_without_the_hook():
    assert _lib.lib().tao_uintx_linear_route_g(9, 37, 2176, 3, 128) == 2
    check(3, 37, 2176, 128, 9, "uintx_dequant_kernel")


def test_leaving_tuning_clears_the_hook():
    with tuning(uintx_mfma=1):
        check(3, 37, 2176, 128, 9, "gemm_mfma_kernel")
    assert _lib.lib().tao_uintx_linear_route_g(9, 37, 2176, 3, 128) == 2  # tuning() cleared it
    check(3, 37, 2176, 128, 9, "uintx_dequant_kernel")


def test_graph_replays_equal_eager():
    bits, N, K, g, M = 5, 256, 4096, 64, 33  # four K slices: the split-K workspace is captured too
    x, args, bias, _, want_b = inputs(bits, N, K, g, M)
    static_x = x.clone()
    with tuning(uintx_mfma=1):
        eager = torch.ops.torchao.uintx_weight_only_linear(x, *args, bias)
        assert last_kernel() == "gemm_mfma_kernel" and torch.equal(eager.cpu(), want_b)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            torch.ops.torchao.uintx_weight_only_linear(static_x, *args, bias)  # warm-up
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = torch.ops.torchao.uintx_weight_only_linear(static_x, *args, bias)
        for sign in (1, -1, 1):
            static_x.copy_(x * sign)
            graph.replay()
            want = torch.ops.torchao.uintx_weight_only_linear(x * sign, *args, bias)
            assert torch.equal(out, want)
