"""Inputs on which the NF4 linear can be checked BIT FOR BIT.

Same idea as tests/exact_inputs.py. The stored components are built directly: zero mean, a
power-of-two factor per group of 256 blocks and power-of-two int8 scalers (either sign), so every
block scaler s[b] = bf16(bf16(q / qf) + 0) is +-2^e exactly and w^ = bf16(level * s[b]) is a level
with its exponent shifted: no rounding anywhere. The sixteen bf16 levels are multiples of 2^-11
(the smallest non-zero one, 0.0796, lies in [2^-4, 2^-3) and has 8 significant bits) of at most
2^11 such units. With e in [-3, -3 + R] and integer x, every term x * w^ of a row is a multiple of
unit = 2^-14, and the maker asserts sum_k |term| < 2^24 units for every (m, n): every partial sum
is then an exact fp32 number whatever the order (GEMV lanes and waves, the matmul's k blocks),
and the output is bf16(sum) (+ bias -> bf16), one rounding each.

The reference is written from the format's formulas in float64 and calls no code under test.
"""

import torch

from exact_inputs import (  # noqa: F401
    BF16,
    INT8_GEMV_FORCED,
    _randint,
    add_bias,
    describe_mismatch,
    round_bf16_once,
)

LEVELS = (-1.0, -0.6962, -0.5251, -0.3949, -0.2844, -0.1848, -0.0911, 0.0,
          0.0796, 0.1609, 0.2461, 0.3379, 0.4407, 0.5626, 0.7230, 1.0)
GEMV_M = (1, 2, 3, 4, 5, 8)
GEMV_N = (1, 37)
GEMV_K = (64, 128, 1024, 1088, 4160)
GEMV_FORCED = INT8_GEMV_FORCED  # (rows per wave, waves along K, row groups); (*, 8, 1) clamps
UNIT = 2.0 ** -14


def levels_bf16():
    lv = torch.tensor(LEVELS).to(BF16)
    u = lv.double() * 2.0 ** 11
    assert torch.equal(u, u.round()) and float(u.abs().max()) == 2.0 ** 11
    return lv


def make_nf4_exact(M, N, K, seed):
    """(codes uint8 [N K / 2], qscalers int8 [N K / 64], qfactor bf16 [ceil(N K / 16384)],
    mean bf16 [], levels bf16 [16], bias bf16 [N], x bf16 [M, K]); asserts exactness."""
    assert K % 64 == 0
    gen = torch.Generator().manual_seed(977 * seed + 5)
    xmax, R = (3, 1) if K <= 1088 else (1, 0)
    nb = N * K // 64
    ng = (N * K + 16383) // 16384
    j0 = _randint(0, 5, (ng,), gen)  # the group's smallest scaler exponent
    qfactor = torch.pow(2.0, (j0 + 3).double()).to(BF16)
    grp = torch.arange(nb) // 256
    j = j0[grp] + _randint(0, R, (nb,), gen)
    sign = _randint(0, 1, (nb,), gen) * 2 - 1
    qs = (sign * (1 << j)).to(torch.int8)
    assert int(qs.abs().max()) <= 64
    nib = _randint(0, 15, (N * K,), gen)
    codes = ((nib[0::2] << 4) | nib[1::2]).to(torch.uint8)
    mean = torch.zeros((), dtype=BF16)
    x = _randint(-xmax, xmax, (M, K), gen).to(BF16)
    bias = (torch.randn(N, generator=gen) * 8).to(BF16)
    w = dequant64(codes, qs, qfactor, mean, levels_bf16(), (N, K))
    assert torch.equal(w.to(BF16).double(), w), "w^ is not a bf16 number"
    wu = w / UNIT
    assert torch.equal(wu, wu.round())
    T = float((x.double().abs() @ wu.abs().t()).max())
    assert T < 2 ** 24, f"partial sums can leave the exact fp32 range: {T:.3g} units"
    return codes, qs, qfactor, mean, levels_bf16(), bias, x


def dequant64(codes, qs, qfactor, mean, levels, shape):
    """w^ from the format's formulas, float64 [shape]; each step rounded to bf16 as the format
    says (here every rounding is exact, which make_nf4_exact asserts on the result)."""
    c = torch.stack([codes >> 4, codes & 0xF], -1).flatten().long()
    grp = torch.arange(qs.numel()) // 256
    d = (qs.double() / qfactor.double()[grp]).to(BF16)
    s = (d.double() + mean.double()).to(BF16).double()
    w = (levels.double()[c] * s.repeat_interleave(64)).to(BF16).double()
    return w.reshape(shape)


def ref_nf4(x, codes, qs, qfactor, mean, levels, N, bias=None):
    """bf16(sum_k x w^) (+ bias -> bf16), the sum exact in float64."""
    w = dequant64(codes, qs, qfactor, mean, levels, (N, x.shape[-1]))
    return add_bias(round_bf16_once(x.double() @ w.t()), bias)
