"""The static-shape int4 GEMV kernels (int4wo_gemv_static_kernel) against the generic kernel and
against the exact reference.

The plain M = 1 linear runs a kernel with its launch shape (rows per wave, Wk, G) as compile-time
constants when m1_shape's choice is one of the instantiated tuples; tao_tune_int4_gemv overrides,
M > 1 and every other shape run int4wo_gemv_kernel with the shape as arguments. Same loads, same
arithmetic and the same summation order (wave 0's partial first, ascending wk), so

  * on ordinary random bf16 data the static kernel's output must be torch.equal to the generic
    kernel's on the identical forced (rpw, wk, g, occupancy), bias on and off, and
  * on the exact inputs (tests/exact_inputs.py) it must be torch.equal to the float64 reference, at
    the smallest shapes that reach each tuple and its edges: K with one slice, two, tail lanes in
    the last slice, an odd slice count over two waves and four slices; N short of and past a
    multiple of the workgroup's rows in each N class of m1_shape.

Each case asserts the kernel it meant to run through tao_last_kernel.
"""

import functools

import pytest
import torch

import exact_inputs as E

from torchao import _lib
from torchao.kernel import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATIC = "int4wo_gemv_static_kernel"
GENERIC = "int4wo_gemv_kernel"


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _linear(x, packed, sz, g, bias):
    return torch.ops.torchao.int4_weight_only_linear(x, packed, sz, g, bias)


# (rows per wave, Wk, G, occupancy) of every static instantiation and the smallest (N, K) that
# m1_shape sends there (S = slices of 2048 k; PAIR = S > Wk)
# (thousands of rows each: a difference in one fp32 rounding flips about one bf16 output in a
# thousand on such data, and a few hundred rows can miss it)
STATIC_TUPLES = [
    ((2, 2, 1, 8), 4094, 4096),    # N <= 4096, S = 2 (wo)
    ((2, 1, 4, 8), 6146, 4096),    # 6144 <= N < 8192, S = 2, PAIR (wqkv)
    ((4, 1, 4, 4), 16390, 4096),   # 16384 <= N < 32768, S = 2, PAIR (w1 || w3)
    ((4, 2, 1, 4), 4094, 14336),   # K > 4096, 2048 < N <= 4096, S = 7, PAIR (w2)
    ((4, 2, 2, 8), 32770, 4096),   # N >= 32768, S = 2 (head)
    ((2, 2, 2, 8), 8194, 4096),    # 8192 < N < 16384, S = 2
    ((2, 2, 4, 8), 4100, 4096),    # 4096 < N < 6144, S = 2
    ((4, 1, 1, 4), 4100, 8192),    # K = 8192, 4096 < N < 10240, S = 4, PAIR
    ((4, 2, 2, 4), 10246, 8192),   # K = 8192, 10240 <= N < 16384, PAIR
    ((8, 2, 1, 4), 32770, 4128),   # K > 4096, N >= 32768, S = 3, PAIR
]


@pytest.mark.parametrize("shape,N,K", STATIC_TUPLES)
def test_static_equals_generic_bit_for_bit(shape, N, K):
    g = 32
    gen = torch.Generator(device=DEV).manual_seed(N * 13 + K)
    q = torch.randint(0, 16, (N, K), dtype=torch.int32, device=DEV, generator=gen)
    packed = torch.ops.torchao.int4_pack(q)
    del q
    s = (torch.rand(N, K // g, device=DEV, generator=gen) * 0.02 + 1e-3).to(torch.bfloat16)
    z = (torch.randn(N, K // g, device=DEV, generator=gen) * 0.05).to(torch.bfloat16)
    sz = torch.stack([s, z], dim=-1).contiguous()
    x = torch.randn(1, K, device=DEV, generator=gen).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV, generator=gen).to(torch.bfloat16)
    for b in (None, bias):
        got = _linear(x, packed, sz, g, b)
        assert _last_kernel() == STATIC, (shape, _last_kernel())
        with tuning(int4_gemv=shape):  # resets the tuning on exit, also on a failure
            want = _linear(x, packed, sz, g, b)
            assert _last_kernel() == GENERIC, (shape, _last_kernel())
        assert bool(torch.isfinite(want.float()).all())
        assert torch.equal(got, want), E.describe_mismatch(
            f"static vs generic {shape} N={N} K={K} bias={'on' if b is not None else 'off'}",
            got.cpu(), want.cpu())
    # the built-in choice is back: the static kernel again
    _linear(x, packed, sz, g, None)
    assert _last_kernel() == STATIC


# ---- exact inputs ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def _exact(M, N, K, g=32):
    seed = (M * 31 + N * 7 + K + g) % 1000
    q = E.make_q(N, K, seed)
    packed = torch.ops.torchao.int4_pack(q.to(DEV))
    bias = E.make_bias(N, seed)
    out = []
    for family in E.FAMILIES:
        _, s, z, x = E.make_int4_exact(M, N, K, g, seed, family, q=q)
        want = E.ref_int4(x, q, s, z, g)
        sz = torch.stack([s, z], dim=-1).contiguous().to(DEV)
        out.append((family, x.to(DEV), packed, sz, bias.to(DEV), want, E.add_bias(want, bias)))
    return tuple(out)


def _check_exact(route, M, N, K, kernel, g=32):
    for family, x, packed, sz, bias, want, want_b in _exact(M, N, K, g):
        for b, ref in ((None, want), (bias, want_b)):
            got = _linear(x, packed, sz, g, b).cpu()
            where = f"{route} M={M} N={N} K={K} {family} bias={'on' if b is not None else 'off'}"
            assert _last_kernel() == kernel, (where, _last_kernel())
            assert torch.equal(got, ref), E.describe_mismatch(where, got, ref)


# K: 2048 (S = 1: one wave per row whatever m1_shape asks, no static tuple), 4096, 4096 - 96 (tail
# lanes in the last slice), 14336 (S = 7, an odd slice count over two waves), 8192 (S = 4).
# N: a row group short of / a row or a row group past a multiple of the workgroup's g * rpw rows in
# each N class of m1_shape at K <= 4096 (<= 4096: 2 rows; 4096..6143: 8; 6144..8191: 8;
# 8192..16383: 4; >= 16384: 16; >= 32768: 8), and in the classes the long-K tuples cover.
EXACT_CASES = (
    [(N, 2048, GENERIC) for N in (4094, 6146, 8194, 16390, 32770)]
    + [(N, 4096, STATIC) for N in (4094, 4095, 4098, 6146, 6150, 8194, 8197, 16390)]
    + [(N, 4096 - 96, STATIC) for N in (4094, 6146, 16396)]
    + [(32770, 2080, STATIC)]
    + [(N, 14336, STATIC) for N in (2050, 4094, 4095)]
    + [(4094, 8192, STATIC), (4097, 8192, STATIC), (10246, 8192, STATIC)]
)


@pytest.mark.parametrize("N,K,kernel", EXACT_CASES)
def test_static_shapes_exact(N, K, kernel):
    _check_exact("gemv m1", 1, N, K, kernel)


# ---- the fallback still routes --------------------------------------------------------------------

def test_m2_takes_the_generic_kernel():
    _check_exact("gemv m2", 2, 4094, 4096, GENERIC)


def test_forced_shape_without_instantiation_takes_the_generic_kernel():
    with tuning(int4_gemv=(1, 2, 2, 0)):
        _check_exact("gemv m1 forced 1x2x2", 1, 4094, 4096, GENERIC)
    _check_exact("gemv m1", 1, 4094, 4096, STATIC)
