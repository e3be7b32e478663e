"""Inputs on which the float8 (e4m3fn) weight-only linear can be checked BIT FOR BIT.

Same idea as tests/exact_inputs.py: every product x * f(w) and every partial sum is an exactly
representable fp32 number, so the order of accumulation (GEMV lanes, MFMA k blocks, split-K
slabs) cannot matter, and what is left is the epilogue of include/torchao_mi355x.h:
o = bf16(fp32(acc * scale)) (+ bias -> bf16), deterministic for any fp32 scale and bf16 bias.

Families:
  "dense"  weights uniform over the 96 e4m3fn values with 0.25 <= |v| < 16 (multiples of 2^-5,
           at most 480 units), integer x in [-4, 4], for K <= 4352: K * 4 * 480 <= 8.4e6 < 2^24.
           Beyond that, the 64 values with 0.5 <= |v| < 8 (multiples of 2^-4, at most 120 units)
           and x in [-2, 2]: 18688 * 2 * 120 = 4.5e6 < 2^24. Scales are arbitrary positive fp32.
  "probe"  each x row is +-1 at 8 positions (exact_inputs.probe_positions). Row n draws its
           codes from two adjacent binades E_n, E_n + 1 (biased exponents; E_n cycles 0..14 over
           the rows, so the subnormals and 448 are hit): every weight is m * unit_n with
           |m| <= 30 and unit_n = 2^(max(E_n, 1) - 10). The scale is a power of two. Then
           |y| / (unit_n * scale_n) <= 8 * 30 < 256 is an integer, itself a bf16 number, so ONE
           wrong code at a probed k changes the output bits.

The makers assert their conditions on the CPU; the references are written from the header
formulas in float64 and call no code under test (the code -> value table is spelled out here and
checked against torch's own float8 cast).
"""

import torch

from exact_inputs import (  # noqa: F401  (shape lists re-exported unchanged)
    BF16,
    FORCED_MNK,
    FORCED_TILES,
    INT8_GEMV_FORCED,
    INT8_GEMV_K,
    INT8_GEMV_M,
    INT8_GEMV_N,
    INT8_MFMA_M,
    MFMA_NK,
    WIDE_MAX_K,
    _randint,
    add_bias,
    describe_mismatch,
    probe_positions,
    round_bf16_once,
    round_up,
)

FP8 = torch.float8_e4m3fn
FAMILIES = ("dense", "probe")
PROBE_G = 32  # chunk size handed to probe_positions (the GEMV's 32-k half slices)


def decode_table():
    """float64 [256]: the value of every e4m3fn code (NaN at 0x7F / 0xFF), from the format's
    definition: sign, 4 exponent bits (bias 7), 3 mantissa bits, subnormals m * 2^-9."""
    c = torch.arange(256)
    sign = torch.where(c >= 128, -1.0, 1.0).double()
    e = (c >> 3) & 15
    m = (c & 7).double()
    v = torch.where(e == 0, m * 2.0 ** -9, (8 + m) * torch.pow(2.0, e.double() - 10))
    v = sign * v
    v[(c & 0x7F) == 0x7F] = float("nan")
    return v


_TABLE = decode_table()


def decode(codes):
    """uint8 codes -> float64 values."""
    return _TABLE[codes.long()]


def _check_table():
    t = torch.arange(256, dtype=torch.uint8).view(FP8).double()
    ok = (t == _TABLE) | (t.isnan() & _TABLE.isnan())
    assert bool(ok.all()), "e4m3fn table disagrees with torch's cast"
    fin = _TABLE[~_TABLE.isnan()]
    assert torch.equal(fin.to(BF16).double(), fin), "a finite e4m3fn value is not a bf16 number"


_check_table()


def _codes(sign, e, m):
    return ((sign << 7) | (e << 3) | m).to(torch.uint8)


def make_fp8wo_exact(M, N, K, seed, family="dense"):
    """codes uint8 [N, K], scale fp32 [N], bias bf16 [N], x bf16 [M, K]; asserts exactness."""
    assert family in FAMILIES
    gen = torch.Generator().manual_seed(131 * seed + 7 + FAMILIES.index(family))
    if family == "dense":
        wide = K <= WIDE_MAX_K
        e_lo, e_hi, xmax = (5, 10, 4) if wide else (6, 9, 2)  # biased exponents
        codes = _codes(_randint(0, 1, (N, K), gen), _randint(e_lo, e_hi, (N, K), gen),
                       _randint(0, 7, (N, K), gen))
        x = _randint(-xmax, xmax, (M, K), gen).to(BF16)
        scale = (torch.rand(N, generator=gen) * 0.02 + 1e-3).float()
        unit = 2.0 ** (e_lo - 10)
        w = decode(codes)
        assert float(w.abs().min()) >= 2.0 ** (e_lo - 7) and float(w.abs().max()) < 2.0 ** (e_hi - 6)
        assert bool(((w / unit) == (w / unit).round()).all())
        T = K * xmax * float(w.abs().max()) / unit
        assert T < 2 ** 24, f"partial sums can leave the exact fp32 range: T <= {T:.3g}"
    else:
        E = (torch.arange(N) + seed) % 15  # row binades E, E + 1
        hi = _randint(0, 1, (N, K), gen)
        m = _randint(0, 7, (N, K), gen)
        e = E.view(N, 1) + hi
        m = torch.where((e == 15) & (m == 7), torch.full_like(m, 6), m)  # 0x7F is NaN: use 448
        codes = _codes(_randint(0, 1, (N, K), gen), e, m)
        # the corners on the first rows that can hold them: +-448, the smallest subnormal
        for n in range(N):
            if int(E[n]) == 14:
                codes[n, 0], codes[n, K - 1] = 0x7E, 0xFE
            if int(E[n]) == 0:
                codes[n, 0], codes[n, K - 1] = 0x01, 0x81
        x = torch.zeros(M, K)
        for mm in range(M):
            p = torch.tensor(probe_positions(K, PROBE_G, gen))
            x[mm, p] = (_randint(0, 1, (p.numel(),), gen) * 2 - 1).float()
        x = x.to(BF16)
        scale = torch.pow(2.0, ((torch.arange(N) * 3 + seed) % 7 - 3).double()).float()
        unit = torch.pow(2.0, torch.clamp(E, min=1).double() - 10).view(N, 1)
        w = decode(codes)
        assert not bool(w.isnan().any())
        mi = w / unit
        assert bool((mi == mi.round()).all()) and float(mi.abs().max()) <= 30
        assert int((x != 0).sum(1).max()) <= 8
        assert float(((x.double().abs() @ mi.abs().t())).max()) < 256
    bias = (torch.randn(N, generator=gen) * 8).to(BF16)
    return codes.contiguous(), scale.contiguous(), bias, x


def exact_fp8wo(x, codes):
    """x @ f(codes)^T exactly, float64 [M, N] (every term a multiple of 2^-9 far below 2^53)."""
    out = torch.empty(x.shape[0], codes.shape[0], dtype=torch.float64)
    xd = x.double()
    step = max(1, (1 << 24) // codes.shape[1])
    for n0 in range(0, codes.shape[0], step):
        out[:, n0:n0 + step] = xd @ decode(codes[n0:n0 + step]).t()
    return out


def ref_fp8wo(x, codes, scale, bias=None):
    """tao_fp8wo_linear_bf16 on exact inputs: bf16(fp32(acc * scale)) (+ bias -> bf16); the sum
    is exact, the product is formed (and rounded) in fp32 as the kernels' epilogue does."""
    acc = exact_fp8wo(x, codes)
    acc32 = acc.float()
    assert torch.equal(acc32.double(), acc), "reference sum is not an fp32 number"
    return add_bias((acc32 * scale.float().view(1, -1)).to(BF16), bias)


def fp8_gpu_shapes():
    """Every (M, N, K) tests/test_gpu_exact_fp8wo.py runs."""
    out = set()
    out.update((M, N, round_up(K, 32)) for M in INT8_GEMV_M for N in INT8_GEMV_N
               for K in INT8_GEMV_K)
    out.update((1, 37, round_up(K, 32)) for K in INT8_GEMV_K)
    out.update((M, N, K) for M in INT8_MFMA_M for N, K in MFMA_NK)
    out.update(FORCED_MNK)
    return sorted(out)


# ---- comparisons shared by tests/test_float8_cpu.py and tests/test_gpu_float8.py ----------------

def same_codes(got, want):
    """uint8 code tensors equal, NaN codes compared without their sign bit (hosts and the GPU
    differ in the sign of a 0 / 0 NaN)."""
    nan = (want & 0x7F) == 0x7F
    return bool(((got == want) | (nan & ((got & 0x7F) == 0x7F))).all())


def same_bf16(got, want):
    """bf16 tensors equal bit for bit, NaN matching any NaN."""
    g, w = got.view(torch.int16), want.view(torch.int16)
    return bool(((g == w) | (got.isnan() & want.isnan())).all())


def rel_l2_finite(y, ref):
    """rel-L2 over the entries where ref is a number; y must be NaN exactly where ref is."""
    y, ref = y.double(), ref.double()
    ok = ~ref.isnan()
    assert torch.equal(~y.isnan(), ok), "NaN columns differ"
    return float(torch.linalg.norm(y[ok] - ref[ok]) / torch.linalg.norm(ref[ok]))
