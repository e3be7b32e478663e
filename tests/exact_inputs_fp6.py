"""Inputs on which the FP6 (e3m2 / e2m3) weight-only linear can be checked BIT FOR BIT.

Same construction as tests/exact_inputs_fp8.py: every product x * value(code) and every partial
sum is an exactly representable fp32 number, so the order of accumulation (GEMV lanes, waves,
the matmul's k blocks) cannot matter, and what is left is the epilogue of
include/torchao_mi355x.h: o = bf16(fp32(acc * scale)) (+ bias -> bf16), deterministic for any
bf16 scale and bias.

Families:
  "dense"  codes uniform over all 64 codes: every value is a multiple of 2^-4 (e3m2, at most 448
           units) or 2^-3 (e2m3, at most 60 units); integer x in [-4, 4]. K <= 8256 keeps every
           partial sum below 8256 * 4 * 448 = 1.48e7 < 2^24 units. Scales are arbitrary positive
           bf16. With ``pow2_scale`` the scales are powers of two instead: then the dequantized
           weight bf16(value * scale) is exact too, and the dequantize + matmul route, whose sum
           runs over the dequantized weight, computes the same number (with an arbitrary scale
           its result would depend on the matmul's summation order).
  "probe"  each x row is +-1 at 8 positions (exact_inputs.probe_positions). Row n draws its codes
           from two adjacent binades E_n, E_n + 1 (biased exponents, E_n cycling over the format's
           range, so the subnormals and the maximum are hit): every weight is m * unit_n with
           |m| <= 14 (e3m2) or 30 (e2m3). The scale is a power of two. Then
           |y| / (unit_n * scale_n) <= 8 * 30 < 256 is an integer, itself a bf16 number, so ONE
           wrong code at a probed k changes the output bits.

The makers assert their conditions on the CPU; the references are written from the header formula
in float64 and call no code under test (the code -> value table and the bit-stream packing are
spelled out here).
"""

import numpy as np
import torch

from exact_inputs import (  # noqa: F401
    BF16,
    _randint,
    add_bias,
    describe_mismatch,
    probe_positions,
)

FORMATS = {"e3m2": (3, 2), "e2m3": (2, 3)}
FAMILIES = ("dense", "probe")
PROBE_G = 32  # chunk size handed to probe_positions (one conversion operand)
DENSE_X = 4

# the smallest shapes at which the GEMV can go wrong: K below one wave slice, one slice plus a
# 64-code tail for a 24-B lane chunk (2048 + 64) and for a 48-B one (4096 + 64), several slices;
# N = 1, N no multiple of any rows-per-workgroup, N = 256
GEMV_K = (64, 2112, 4160, 8256)
GEMV_N = (1, 37, 256)
GEMV_M = tuple(range(1, 9))
# (rows per wave at M == 1, waves along K, row groups, 32-code groups per lane chunk)
GEMV_FORCED = ((2, 1, 1, 1), (8, 2, 4, 1), (4, 8, 1, 1), (2, 2, 2, 2), (8, 1, 8, 2), (4, 3, 2, 2))
MM_M = (9, 48)


def decode_table(ebits, mbits):
    """float64 [64]: the value of every code from the definition: sign, ebits exponent bits
    (bias 2^(ebits - 1) - 1), mbits mantissa bits, subnormals, no inf and no NaN."""
    bias = 2 ** (ebits - 1) - 1
    c = torch.arange(64)
    e = (c >> mbits) & (2 ** ebits - 1)
    m = (c & (2 ** mbits - 1)).double()
    v = torch.where(e == 0, m * 2.0 ** (1 - bias - mbits),
                    (1 + m / 2 ** mbits) * torch.pow(2.0, (e - bias).double()))
    return torch.where(c >= 32, -v, v)


_TABLES = {f: decode_table(*em) for f, em in FORMATS.items()}
assert float(_TABLES["e3m2"].max()) == 28.0 and float(_TABLES["e2m3"].max()) == 7.5
for _t in _TABLES.values():
    assert torch.equal(_t.to(BF16).double(), _t), "an fp6 value is not a bf16 number"


def decode(fmt, codes):
    return _TABLES[fmt][codes.long()]


def pack_native(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes [N, K] -> the op's storage int32 [N, K * 6 / 32]: code k at bits 6 k .. 6 k + 5
    of the row's little-endian bit stream."""
    c = codes.numpy()
    N, K = c.shape
    stream = np.zeros((N, K * 6), dtype=np.uint8)
    for b in range(6):
        stream[:, b::6] = (c >> b) & 1
    return torch.from_numpy(np.packbits(stream, axis=1, bitorder="little").view(np.int32).copy())


def make_fp6_exact(fmt, M, N, K, seed, family="dense", pow2_scale=False):
    """codes uint8 [N, K], scale bf16 [N], bias bf16 [N], x bf16 [M, K]; asserts exactness."""
    assert family in FAMILIES and K % 64 == 0
    ebits, mbits = FORMATS[fmt]
    bias_e = 2 ** (ebits - 1) - 1
    gen = torch.Generator().manual_seed(257 * seed + 11 + FAMILIES.index(family) + 2 * (fmt == "e2m3"))
    if family == "dense":
        codes = _randint(0, 63, (N, K), gen).to(torch.uint8)
        x = _randint(-DENSE_X, DENSE_X, (M, K), gen).to(BF16)
        if pow2_scale:
            scale = torch.pow(2.0, _randint(-9, -3, (N,), gen).double()).to(BF16)
        else:
            scale = (torch.rand(N, generator=gen) * 0.02 + 1e-3).to(BF16)
        unit = 2.0 ** (1 - bias_e - mbits)
        w = decode(fmt, codes)
        assert bool(((w / unit) == (w / unit).round()).all())
        T = K * DENSE_X * float(w.abs().max()) / unit
        assert T < 2 ** 24, f"partial sums can leave the exact fp32 range: T <= {T:.3g}"
    else:
        nE = 2 ** ebits - 1  # rows' lower binade E in [0, 2^ebits - 2]
        E = (torch.arange(N) + seed) % nE
        e = E.view(N, 1) + _randint(0, 1, (N, K), gen)
        m = _randint(0, 2 ** mbits - 1, (N, K), gen)
        codes = ((_randint(0, 1, (N, K), gen) << 5) | (e << mbits) | m).to(torch.uint8)
        for n in range(N):  # the corners on the rows that can hold them
            if int(E[n]) == nE - 1:
                codes[n, 0], codes[n, K - 1] = 0x1F, 0x3F  # +-max
            if int(E[n]) == 0:
                codes[n, 0], codes[n, K - 1] = 0x01, 0x21  # +-smallest subnormal
        x = torch.zeros(M, K)
        for mm in range(M):
            p = torch.tensor(probe_positions(K, PROBE_G, gen))
            x[mm, p] = (_randint(0, 1, (p.numel(),), gen) * 2 - 1).float()
        x = x.to(BF16)
        scale = torch.pow(2.0, ((torch.arange(N) * 3 + seed) % 7 - 3).double()).to(BF16)
        unit = torch.pow(2.0, torch.clamp(E, min=1).double() - bias_e - mbits).view(N, 1)
        mi = decode(fmt, codes) / unit
        assert bool((mi == mi.round()).all()) and float(mi.abs().max()) <= 2 * (2 ** (mbits + 1) - 1)
        assert int((x != 0).sum(1).max()) <= 8
        assert float((x.double().abs() @ mi.abs().t()).max()) < 256
    bias = (torch.randn(N, generator=gen) * 8).to(BF16)
    return codes.contiguous(), scale.contiguous(), bias, x


def exact_fp6(fmt, x, codes):
    """x @ value(codes)^T exactly, float64 [M, N]."""
    return x.double() @ decode(fmt, codes).t()


def ref_fp6(fmt, x, codes, scale, bias=None):
    """tao_fp6_linear_bf16 on exact inputs: bf16(fp32(acc * scale)) (+ bias -> bf16); the sum is
    exact, the product is formed (and rounded) in fp32 as the kernel's epilogue does."""
    acc = exact_fp6(fmt, x, codes)
    acc32 = acc.float()
    assert torch.equal(acc32.double(), acc), "reference sum is not an fp32 number"
    return add_bias((acc32 * scale.float().view(1, -1)).to(BF16), bias)


def dequant64(fmt, codes, scale):
    """float64 of bf16(fp32(value) * fp32(scale)): the dequantizer's formula."""
    return (decode(fmt, codes).float() * scale.float().view(-1, 1)).to(BF16).double()
