"""Bit-exact GPU tests of torch.ops.torchao.int4_prescaled_linear on the inputs of
tests/exact_inputs.py.

The activation is fed as x * p with p[k] = 2^e_k, e_k in -2..2 drawn per column, and p is the
activation scale: x holds small integers, so x * p is a bf16 number and every quotient is exactly
the original x. The output must then be the float64 reference of the original x rounded once to
bf16 (exact_inputs.ref_int4), bit for bit, whichever route the op takes: the fused one-token
launch, the pre-scale then the GEMV at 2..8 tokens, the pre-scale then the MFMA kernels at 70. A
scale applied to the wrong column, a piece of x staged in the wrong LDS slot or a lane past K that
leaks a quotient changes output bits.
"""

import functools

import pytest
import torch

import exact_inputs as E

from torchao import _lib
from torchao.kernel import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def _col_scale(K, seed):
    gen = torch.Generator().manual_seed(seed * 977 + K)
    e = torch.randint(-2, 3, (K,), generator=gen)
    return torch.pow(2.0, e.double()).to(BF16)


@functools.lru_cache(maxsize=8)
def _inputs(M, N, K, g):
    """[(label, x * p, p, packed, sz, bias, want, want_with_bias, x, q, s, z)], made once per shape."""
    seed = (M * 31 + N * 7 + K + g) % 1000
    q = E.make_q(N, K, seed)
    packed = torch.ops.torchao.int4_pack(q.to(DEV))
    bias = E.make_bias(N, seed)
    p = _col_scale(K, seed)
    out = []
    for family in E.FAMILIES:
        _, s, z, x = E.make_int4_exact(M, N, K, g, seed, family, q=q)
        xp = (x.double() * p.double()).to(BF16)
        assert torch.equal(xp.double(), x.double() * p.double())       # x * p is a bf16 number
        assert torch.equal((xp / p), x)                                # and the quotient is x
        want = E.ref_int4(x, q, s, z, g)
        sz = torch.stack([s, z], dim=-1).contiguous().to(DEV)
        out.append((family, xp.to(DEV), p.to(DEV), packed, sz, bias.to(DEV), want,
                    E.add_bias(want, bias), x, q, s, z))
    return tuple(out)


def _op(xp, p, packed, sz, g, b):
    return torch.ops.torchao.int4_prescaled_linear(xp, p, packed, sz, g, b)


def _one_launch(xp, p, packed, sz, g, b):
    """tao_int4wo_prescaled_linear_bf16 itself: the op routes K > 4096 (and any bias) to the two
    launches, which the same inputs check through `_op`."""
    if b is not None:
        return _op(xp, p, packed, sz, g, b)
    N, K = packed.shape[0], packed.shape[1] * 8
    y = torch.empty(1, N, dtype=BF16, device=DEV)
    _lib.call("tao_int4wo_prescaled_linear_bf16", xp.data_ptr(), p.data_ptr(), packed.data_ptr(),
              sz.data_ptr(), None, y.data_ptr(), 1, N, K, g,
              torch.cuda.current_stream().cuda_stream)
    return y


def check(route, M, N, K, g, kernel=None, run=_op):
    for label, xp, p, packed, sz, bias, want, want_b, *_ in _inputs(M, N, K, g):
        for b, ref in ((None, want), (bias, want_b)):
            got = run(xp, p, packed, sz, g, b).cpu()
            last = _lib.lib().tao_last_kernel().decode()
            where = f"{route} M={M} N={N} K={K} g={g} {label} bias={'on' if b is not None else 'off'}"
            assert got.shape == ref.shape, where
            assert torch.equal(got, ref), E.describe_mismatch(f"{where} kernel={last}", got, ref)
            if kernel is not None and b is None:
                assert kernel in last, (where, last)


@pytest.mark.parametrize("N,K", E.XLDS_NK)
def test_fused_one_token(N, K):
    check("fused", 1, N, K, 32, kernel="int4wo_gemv_prescale_kernel", run=_one_launch)
    check("op, one token", 1, N, K, 32)


@pytest.mark.parametrize("M,N,K,g", E.GEMV_MULTI_M)
def test_prescale_then_gemv(M, N, K, g):
    with tuning(linear_crossover=8):
        check("prescale + gemv", M, N, K, g, kernel="gemv")


@pytest.mark.parametrize("N,K", E.MFMA_NK)
def test_prescale_then_mfma(N, K):
    check("prescale + mfma", 70, N, K, 32)


@pytest.mark.parametrize("M,N,K", [(1, 37, 2080), (3, 200, 352), (70, 200, 352)])
def test_a_scale_from_the_wrong_column_changes_output_bits(M, N, K):
    """Probe family: halve the scale of ONE probed column k0 (what a kernel reading a neighbouring
    column's scale amounts to there). The quotient at k0 doubles, the output must equal the reference
    of that x, and it differs from the intact reference in exactly the rows whose dequantised weight
    at k0 is not zero: a per-column scale slip reaches the output bits, so the equalities above
    would flag it."""
    g = 32
    _, xp, p, packed, sz, _, want, _, x, q, s, z = _inputs(M, N, K, g)[E.FAMILIES.index("probe")]
    k0 = int(x[0].nonzero()[1])                      # a probed column of row 0
    p2 = p.clone()
    p2[k0] = p[k0] / 2
    x2 = x.clone()
    x2[0, k0] = x[0, k0] * 2
    hit = x[:, k0] != 0                              # rows of x probing k0 (row 0 at least)
    x2[hit, k0] = x[hit, k0] * 2
    got = torch.ops.torchao.int4_prescaled_linear(xp, p2, packed, sz, g, None).cpu()
    assert torch.equal(got, E.ref_int4(x2, q, s, z, g))
    w_k0 = (q[:, k0].double() - 8) * s[:, k0 // g].double() + z[:, k0 // g].double()
    changed = (got != want)
    expect = hit.view(-1, 1) & (w_k0 != 0).view(1, -1)
    assert bool(expect.any())
    assert torch.equal(changed, expect)
