"""Inputs on which the weight-only linears can be checked BIT FOR BIT, and their references.

The int4 / int8 weight-only kernels accumulate in fp32 in kernel-specific orders (32-k chunks
spread over lanes, MFMA k blocks, split-K slabs), so on ordinary data they can only be held to a
norm. On the inputs made here every product and every partial sum is an exactly representable
fp32 number, so no addition rounds, the order of accumulation cannot matter, and the only
rounding left is the deterministic fp32 -> bf16 (RNE) of the epilogue. Two conditions give that,
and the makers assert both on the CPU:

  1. bf16 representability: x takes small integers, scale = 2^e, zero = zi * 2^e with integer zi
     and |q - 8 + zi| < 256, so scale, zero and the dequantised weight (q - 8) * s + z all
     round-trip through bf16 unchanged (what the MFMA kernels feed the matrix cores), and
     z - 8 s and fma(q, s, z - 8 s) are exact in fp32.
  2. T = max_{m,n} sum_k |x_mk| (|q_nk - 8| s + |z|) / 2^emin < 2^24, with 2^emin the smallest
     scale. Every term is an integer multiple of 2^emin; T bounds the magnitude of every partial
     sum under any ordering, also under the GEMV's split of a chunk into its scale term
     s * sum x (q - 8) and its zero term z * sum x, so every partial sum is an integer below
     2^24 in units of 2^emin: an exact fp32 number.

These are conditions on the inputs, not tolerances: a shape that violates one gets narrower
ranges, the comparison stays torch.equal. The references below are written from the formulas in
include/torchao_mi355x.h in float64 and call no code under test (nor the oracle).

Families: "dense" (every k contributes: accumulation, per-group scales, output rounding) and
"probe" (each x row is +-1 at 8 positions, so |y / s_row| <= 8 * 28 < 256 is itself a bf16 number
and ONE wrong nibble, scale or zero at a probed k changes the output bits; dense outputs reach
~5e4 in units of 1/8, where a bf16 ulp can swallow a single nibble).
"""

import torch

BF16 = torch.bfloat16

# dense-family ranges: x in [-x, x], zi in [-zi, zi], e in [e0, e1]
WIDE = {"x": 4, "zi": 100, "e": (-3, 1)}
NARROW = {"x": 2, "zi": 12, "e": (-1, 0)}
WIDE_MAX_K = 4352  # T reaches ~4.8e6 here with WIDE and would pass 2^24 at K = 18688
PROBE_ZI = 20
PROBE_NNZ = 8
FAMILIES = ("dense", "probe")
GROUPS = (32, 64, 128, 256)


def round_up(k, m):
    return (k + m - 1) // m * m


def ranges_for(K):
    return WIDE if K <= WIDE_MAX_K else NARROW


def _randint(lo, hi, shape, gen, dtype=torch.int64):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=dtype)


def make_q(N, K, seed):
    """Uniform nibbles, int32 [N, K]; a function of (N, K, seed) alone so families can share it."""
    gen = torch.Generator().manual_seed(1_000_003 * seed + 17)
    n = N * K
    # 16 nibbles per random 64-bit word (several times quicker than one draw per nibble)
    raw = torch.randint(-(2 ** 63), 2 ** 63 - 1, ((n + 15) // 16,), generator=gen)
    b = raw.view(torch.uint8)
    return torch.stack([b & 15, b >> 4], -1).flatten()[:n].view(N, K).to(torch.int32)


def probe_positions(K, g, gen):
    """8 distinct k: 0, K - 1, a straddle (b - 1, b) of a boundary of the coarsest kind inside K
    (a multiple of 2048 is also a 256 / 128 / group / 32-k chunk boundary), one of a group
    boundary, one of a chunk / MFMA k-step boundary, the rest random."""
    pos = {0, K - 1}

    def straddle(u):
        n = (K - 1) // u
        if n >= 1:
            b = u * int(_randint(1, n, (1,), gen))
            pos.update((b - 1, b))

    for u in (2048, 256, 128, g, 32):
        if (K - 1) // u >= 1:
            straddle(u)
            break
    straddle(g)
    straddle((32, 128, 256)[int(_randint(0, 2, (1,), gen))])
    while len(pos) < min(PROBE_NNZ, K):
        pos.add(int(_randint(0, K - 1, (1,), gen)))
    return sorted(pos)  # 2 + at most three straddles: never more than 8


def _emin(s):
    return int(torch.log2(s.double().min()).round())


def check_int4_exact(x, q, s, z, g):
    """Assert conditions 1 and 2 of the module docstring; returns the bound on T that was checked
    (computed in float64 with |q - 8| replaced by its maximum 8, so it is >= T)."""
    N, K = q.shape
    G = K // g
    assert s.dtype == BF16 and z.dtype == BF16 and x.dtype == BF16
    assert s.shape == (N, G) and z.shape == (N, G) and x.shape[1] == K
    sd, zd, xd = s.double(), z.double(), x.double()
    mant, _ = torch.frexp(sd)
    assert bool((mant == 0.5).all()), "scales must be powers of two"
    zi = zd / sd
    assert bool((zi == zi.round()).all()), "zero must be an integer multiple of its scale"
    assert float(zi.abs().max()) + 8 < 256, "|q - 8 + zi| must stay below 256"
    assert bool((xd == xd.round()).all()) and int(q.min()) >= 0 and int(q.max()) <= 15
    if N * K <= (1 << 22):  # the dequantised weights themselves, where that is cheap
        w = (q.double() - 8).view(N, G, g) * sd.unsqueeze(-1) + zd.unsqueeze(-1)
        assert torch.equal(w.to(BF16).double(), w), "dequantised weight is not a bf16 number"
    unit = 2.0 ** _emin(s)
    ax = xd.abs().view(-1, G, g).sum(-1)            # [M, G]
    b = (8.0 * sd + zd.abs()) / unit                 # [N, G]
    T = float((ax @ b.t()).max())
    assert T < 2 ** 24, f"partial sums can leave the exact fp32 range: T <= {T:.3g}"
    return T


def make_int4_exact(M, N, K, g, seed, family="dense", q=None):
    """q int32 [N, K], s, z bf16 [N, K/g], x bf16 [M, K]; asserts the two exactness conditions.
    `q`: reuse make_q(N, K, seed) made earlier (it does not depend on the family)."""
    assert family in FAMILIES and K % g == 0
    G = K // g
    if q is None:
        q = make_q(N, K, seed)
    gen = torch.Generator().manual_seed(7919 * seed + FAMILIES.index(family) + 1)
    r = ranges_for(K)
    e0, e1 = r["e"]
    if family == "dense":
        e = _randint(e0, e1, (N, G), gen)
        zi = _randint(-r["zi"], r["zi"], (N, G), gen)
        x = _randint(-r["x"], r["x"], (M, K), gen).to(BF16)
    else:
        # one exponent per row, neighbouring rows always differ
        e = (e0 + (torch.arange(N) + seed) % (e1 - e0 + 1)).view(N, 1).expand(N, G)
        zi = _randint(-PROBE_ZI, PROBE_ZI, (N, G), gen)
        x = torch.zeros(M, K)
        for m in range(M):
            p = torch.tensor(probe_positions(K, g, gen))
            x[m, p] = (_randint(0, 1, (p.numel(),), gen) * 2 - 1).float()
        x = x.to(BF16)
    sd = torch.pow(2.0, e.double())
    s = sd.to(BF16).contiguous()
    z = (zi.double() * sd).to(BF16).contiguous()
    check_int4_exact(x, q, s, z, g)
    return q, s, z, x


def make_bias(N, seed):
    """Arbitrary bf16 bias: the epilogue's bf16(bf16(acc) + bias) is one deterministic rounding."""
    gen = torch.Generator().manual_seed(seed + 99)
    return (torch.randn(N, generator=gen) * 8).to(BF16)


def exact_int4(x, q, s, z, g):
    """y = x @ ((q - 8) * s + z)^T exactly, float64 [M, N]: integer arithmetic in units of the
    smallest scale (every value far below 2^53). Columns where all of x is zero are left out,
    rows of q are taken in chunks."""
    N, K = q.shape
    G = K // g
    unit = 2.0 ** _emin(s)
    si = s.double() / unit
    zi = z.double() / unit
    xd = x.double()
    cols = (xd != 0).any(0).nonzero().flatten()
    if cols.numel() == 0:
        return torch.zeros(x.shape[0], N, dtype=torch.float64)
    sparse = cols.numel() < K
    grp = cols // g if sparse else None
    xs = xd[:, cols] if sparse else xd
    out = torch.empty(x.shape[0], N, dtype=torch.float64)
    step = max(1, (1 << 24) // xs.shape[1])
    for n0 in range(0, N, step):
        n1 = min(N, n0 + step)
        if sparse:
            w = (q[n0:n1][:, cols].double() - 8) * si[n0:n1][:, grp] + zi[n0:n1][:, grp]
        else:
            w = ((q[n0:n1].double() - 8).view(n1 - n0, G, g) * si[n0:n1].unsqueeze(-1)
                 + zi[n0:n1].unsqueeze(-1)).view(n1 - n0, K)
        out[:, n0:n1] = xs @ w.t()
    assert float(out.abs().max()) < 2 ** 24
    return out * unit


def round_bf16_once(y64):
    """float64 values that are exact fp32 numbers -> bf16, one RNE rounding."""
    y32 = y64.float()
    assert torch.equal(y32.double(), y64), "reference value is not an fp32 number"
    return y32.to(BF16)


def add_bias(y, bias):
    """The epilogue's second step: bf16(y + bias), the sum formed in fp32 (None: y)."""
    return y if bias is None else (y.float() + bias.float()).to(BF16)


def ref_int4(x, q, s, z, g, bias=None):
    """tao_int4wo_linear_bf16 on exact inputs: bf16(sum), then bf16(. + bias) in fp32."""
    return add_bias(round_bf16_once(exact_int4(x, q, s, z, g)), bias)


# ---- int8 weight-only -------------------------------------------------------------------------

INT8_X = 4


def make_int8wo_exact(M, N, K, seed):
    """w int8 [N, K] uniform in [-128, 127], arbitrary bf16 scale [N] and bias [N], integer
    x in [-4, 4] bf16 [M, K]. Products are integers and every partial sum stays below
    K * 4 * 128 < 2^24, so the fp32 (or bf16-MFMA) accumulation is exact in any order."""
    assert K * INT8_X * 128 < 2 ** 24, "partial sums can leave the exact fp32 range"
    gen = torch.Generator().manual_seed(31 * seed + 5)
    w = torch.randint(-128, 128, (N, K), generator=gen, dtype=torch.int8)
    x = _randint(-INT8_X, INT8_X, (M, K), gen).to(BF16)
    scale = (torch.rand(N, generator=gen) * 0.02 + 1e-3).to(BF16)
    bias = torch.randn(N, generator=gen).to(BF16)
    assert int(w.min()) >= -128 and int(w.max()) <= 127
    return w, scale, bias, x


def exact_int8wo(x, w):
    """x @ w^T exactly, float64 [M, N]."""
    out = torch.empty(x.shape[0], w.shape[0], dtype=torch.float64)
    xd = x.double()
    step = max(1, (1 << 24) // w.shape[1])
    for n0 in range(0, w.shape[0], step):
        out[:, n0:n0 + step] = xd @ w[n0:n0 + step].double().t()
    return out


def ref_int8wo(x, w, scale, bias=None):
    """tao_int8wo_linear_bf16 on exact inputs: bf16(bf16(sum) * scale) (+ bias -> bf16), each
    product / sum formed in fp32 as the kernels' epilogue does."""
    y = round_bf16_once(exact_int8wo(x, w))
    return add_bias((y.float() * scale.float()).to(BF16), bias)


def describe_mismatch(route, got, want, limit=6):
    """Failure text: the route, how many elements differ, the first few (m, n, got, want)."""
    bad = (got != want).nonzero()
    rows = [f"(m={int(m)}, n={int(n)}, got={float(got[m, n])!r}, want={float(want[m, n])!r})"
            for m, n in bad[:limit]]
    return f"{route}: {bad.shape[0]} of {got.numel()} outputs differ: " + ", ".join(rows)


# ---- the (M, N, K, g) of every GPU case (tests/test_gpu_exact_int4.py), shared with the CPU
# checks of the conditions (tests/test_exact_inputs_cpu.py) ---------------------------------------

# M = 1, built-in routing: K -> slices S of 2048 k (352 -> 1, 2080 -> 2, 4128 -> 3, 8224 -> 5,
# 16416 -> 9, 18464 / 18688 -> 10), N across every branch of m1_shape
M1_ROUTED = (
    [(N, K, 32) for K in (352, 2080) for N in (40, 4100, 6150, 8200, 11010, 16390, 32770)]
    + [(N, K, 32) for K in (4128, 8224)
       for N in (1000, 1540, 2050, 2600, 4100, 6000, 10250, 32770)]
    + [(N, 16416, 32) for N in (24, 1030, 4100)]
    + [(24, 18464, 32), (24, 18688, 256)]
)
M1_GROUPS = [(37, 2080 if g == 32 else 2304, g) for g in GROUPS] + [(24, 18688, g) for g in GROUPS]

GEMV_FORCED_SHAPES = [(rpw, wk, rg, occ)
                      for rpw in (1, 2, 4, 8)
                      for wk, rg in ((1, 1), (1, 8), (2, 4), (8, 1), (3, 2))
                      for occ in ((4, 8) if rpw == 4 else (0,))]
GEMV_FORCED_NK = [(N, K) for N in (1, 37) for K in (32, 2080, 18464)]
XLDS_NK = [(40, 352), (37, 2080), (24, 8224)]

# K rounded up to a multiple of the group size where it is none (352 -> 384, 4128 -> 4224 at 128)
GEMV_MULTI_M = [(M, N, round_up(K, g), g) for M in (2, 3, 4, 5, 8) for N in (9, 200)
                for K in (352, 4128) for g in (32, 128)]

MFMA_NK = [(200, 352), (72, 32), (520, 1056)]
MFMA16_M = (5, 17, 48, 129, 300)
MFMA32_M = (5, 33, 70, 129)
# tests/test_gpu_gemm_tiles.py FORCED: (M tile, k-groups, K slices)
FORCED_TILES = [(16, 1, 1), (16, 4, 1), (16, 2, 3), (32, 4, 4), (32, 1, 2), (64, 2, 2), (64, 1, 1),
                (128, 1, 5), (16, 4, 64), (32, 2, 16)]
FORCED_MNK = [(70, 200, 1056), (70, 72, 3200)]

TILE_MNK = [(70, 200, 1024), (129, 72, 3072), (600, 136, 1024)]
TILE_SPLITS = (0, 1, 2, 16)

# (bn, wm, splits, stages, a_steps); wm 1 = the 32x32x16 kernel (gemm_sf32.hip)
SF_CFGS = [(64, 2, 4, 3, 0), (64, 8, 2, 2, 0), (128, 4, 8, 3, 0), (128, 2, 1, 3, 0),
           (128, 1, 4, 3, 0), (64, 1, 2, 3, 0), (256, 1, 2, 2, 0)]
SF_MNK = [(17, 128, 1024), (100, 200, 3072), (200, 96, 2048), (128, 72, 14336)]
SF_GROUPS_MNK = (96, 320, 3072)

CHAINED_NK = (1000, 2080)


def int4_gpu_shapes():
    """Every (M, N, K, g) the GPU int4 file runs."""
    out = set()
    out.update((1, N, K, g) for N, K, g in M1_ROUTED + M1_GROUPS)
    out.update((1, N, K, 32) for N, K in GEMV_FORCED_NK + XLDS_NK)
    out.update(GEMV_MULTI_M)
    out.update((M, N, K, 32) for M in MFMA16_M for N, K in MFMA_NK)
    out.update((M, N, K, 32) for M, N, K in FORCED_MNK)
    out.update((70, 200, 2048, g) for g in GROUPS)
    out.update((M, N, round_up(K, g), g) for M in MFMA32_M for N, K in MFMA_NK for g in (32, 256))
    out.update((M, N, K, g) for M, N, K in TILE_MNK for g in (32, 64))
    out.update((M, N, K, 32) for M, N, K in SF_MNK)
    out.update((*SF_GROUPS_MNK, g) for g in GROUPS)
    out.add((1, *CHAINED_NK, 32))
    return sorted(out)


# int8 weight-only (tests/test_gpu_exact_int8wo.py). The public entry takes K % 32 == 0 only, so
# each K of the GEMV list that is 16 mod 32 is checked to be REJECTED there (and run through the
# one-token decode entry, which takes K % 16 == 0), and its round-up to 32 runs in its place.
INT8_GEMV_M = (1, 2, 3, 4, 8)
INT8_GEMV_N = (1, 37, 330)
INT8_GEMV_K = (16, 1040, 8208, 16400)
INT8_GEMV_FORCED = [(rpw, wk, rg) for rpw in (2, 4, 8) for wk, rg in ((1, 1), (2, 4), (8, 1))]
INT8_MFMA_M = (5, 48, 129, 300)
INT8_TILE_SPLITS = (0, 2, 16)


def int8_gpu_shapes():
    out = set()
    for K in INT8_GEMV_K:
        out.update((M, N, Kx) for M in INT8_GEMV_M for N in INT8_GEMV_N
                   for Kx in (K, round_up(K, 32)))
    out.update((M, N, K) for M in INT8_MFMA_M for N, K in MFMA_NK)
    out.update(FORCED_MNK)
    out.update(TILE_MNK)
    return sorted(out)
