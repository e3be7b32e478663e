"""Inputs on which the three block-scaled linears can be checked BIT FOR BIT: MXFP8 (mx_scaled_mm,
mx_dyn_linear), MXFP4 weights (mxfp4w_scaled_mm, mxfp4w_dyn_linear) and blockwise float8
(blockfp8_scaled_mm, blockfp8_dyn_linear).

The idea of tests/exact_inputs_fp8dyn.py with per-block scales that are powers of two. Both
operands are codes of small integers, random and unrelated between x and w (x in [-4, 4]; w in
[-7, 7] as e4m3fn, or the 15 nonzero e2m1 values, multiples of 1/2), and block b of row r is scaled
by 2^(r0(r) + d(r, b)) with d in [0, h]: r0 moves the whole row, d differs per (row, block). Then

  * every scaled product of output (m, n) is a multiple of unit(m, n) = ux(m) * uw(n), the lowest
    set bit of the scaled x row times that of the scaled w row;
  * the sum of the magnitudes stays below 2^24 units, so every partial sum, in any order (GEMV
    lanes and slices, MFMAs, steps, k-groups, split-K slices), is an fp32 number;
  * inside one matrix instruction (an aligned run of 128 k) max |scaled product| < 2^12 units
    (MFMA_WINDOW_BITS: v_mfma_scale_f32_16x16x128_f8f6f4 kept a product 2^13 times smaller than the
    largest of its group of 8 k and dropped one 2^14 times smaller; measured with unit scale bytes,
    experiments/probe_mfma_f8_exact.py). The window has not been probed with scale bytes other
    than 127; the bound is put on the SCALED products, i.e. as if the instruction scaled every
    product before adding. With it every case of tests/test_gpu_exact_blockscaled.py is bit-exact
    on the MI355X (MFMA cases: scale bytes 124 .. 133 on both operands, up to 1792 units inside
    one instruction for MXFP8 and 3072 for MXFP4 weights), so the span did not have to be
    narrowed. The blockwise float8 kernel runs the instruction with unit bytes and scales its
    result with fma(P, xs * ws, acc), so there the window is checked on the bare codes and the
    scales only enter the 2^24 bound (a power of two times an exact P is exact).

h is the largest of 3, 2, 1, 0 for which the worst case fits: K * pmax * 4^h < 2^24 and
pmax * 4^h < 2^12, with pmax the largest bare product in units (28, or 48 half units for e2m1). The
bias is a bf16 multiple of the largest unit of its column, small enough that acc + bias is an fp32
number too, so the output is bf16(acc + bias) with ONE rounding.

The references are the float64 formulas of csrc/mx_fp8.hip, mx_fp4.hip and block_fp8.hip (the _y64 of
the three test_gpu_* files); they assert that their sums are fp32 numbers and call no code under
test. The identity tokens are bf16 rows on which the quantizers are the identity on known codes
and scales (checked against to_mx / fp8_blockwise_act_quant in tests/test_exact_blockscaled_cpu.py).
"""

import torch

from exact_inputs_fp8dyn import (  # noqa: F401  (re-exported for the tests)
    BF16,
    FP8,
    MFMA_WINDOW_BITS,
    _lowbit_unit,
    decode,
    describe_mismatch,
)

FORMATS = ("mx", "mxfp4w", "blockfp8")
BLOCK = {"mx": 32, "mxfp4w": 32, "blockfp8": 128}
X_MAX, W_MAX = 4, 7
# e2m1 code -> value (code 8 is -0)
F4_VALUES = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6],
                         dtype=torch.float64)
# the largest bare product in units of the format (mxfp4w: half units)
PMAX = {"mx": X_MAX * W_MAX, "mxfp4w": X_MAX * 12, "blockfp8": X_MAX * W_MAX}


# ---- small helpers ------------------------------------------------------------------------------

def _randint(lo, hi, shape, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen)


def _e4m3(v):
    """float64 values -> e4m3fn codes (uint8), exactly."""
    q = v.to(FP8)
    assert torch.equal(q.double(), v.double()), "not made of e4m3fn values"
    return q.view(torch.uint8).contiguous()


def pack_fp4(codes):
    """uint8 e2m1 codes [N, K] -> [N, K/2], element 2 j in the high nibble (the stored order)."""
    return ((codes[:, ::2] << 4) | codes[:, 1::2]).contiguous()


def unpack_fp4(wq):
    return torch.stack([wq >> 4, wq & 0xF], -1).reshape(wq.shape[0], -1)


def e8m0(byte):
    """E8M0 scale bytes -> float64 (255 is NaN)."""
    v = torch.exp2(byte.double() - 127)
    v[byte == 255] = float("nan")
    return v


def span_half(K, pmax, extra=0):
    """h: each operand's per-block exponent d lies in [0, h]. `extra`: worst-case units a row adds
    beyond K * pmax at h = 0 (the +-448 entries of the blockwise identity token)."""
    for h in (3, 2, 1, 0):
        if (K * pmax + extra) * 4 ** h < 2 ** 24 and pmax * 4 ** h < 2 ** MFMA_WINDOW_BITS:
            return h
    raise AssertionError(f"K = {K} does not fit the exact fp32 range")


def _exponents(rows, nblk, h, gen, lo, hi, mul):
    """[rows, nblk] integer exponents r0(row) + d(row, block), r0 in [lo, hi], d in [0, h]; inside
    a row neighbouring blocks differ, and neighbouring rows differ in r0 (so a scale taken from the
    next block or the next row is another power of two). mul: coprime to hi - lo + 1."""
    r0 = (mul * torch.arange(rows) + int(_randint(0, 6, (1,), gen))) % (hi - lo + 1) + lo
    d = _randint(0, h, (rows, nblk), gen)
    if h > 0:
        for b in range(1, nblk):
            same = d[:, b] == d[:, b - 1]
            d[:, b] = torch.where(same, (d[:, b] + 1) % (h + 1), d[:, b])
    return r0[:, None] + d


def _x_exponents(M, nblk, h, gen):
    return _exponents(M, nblk, h, gen, -2, 2, 3)


def _w_exponents(N, nblk, h, gen):
    return _exponents(N, nblk, h, gen, -3, 3, 5)


def _x_ints(M, K, gen, block=None):
    """Integers in [-4, 4]; with `block`, every block of that many k holds at least one +-4."""
    x = _randint(-X_MAX, X_MAX, (M, K), gen)
    if block:
        nblk = K // block
        pos = _randint(0, block - 1, (M, nblk), gen) + block * torch.arange(nblk)[None, :]
        sign = _randint(0, 1, (M, nblk), gen) * 2 - 1
        x.scatter_(1, pos, sign * X_MAX)
    return x


def _w_fp4_codes(N, K, gen):
    """e2m1 codes over the 15 nonzero values; the code at k differs from the code at k ^ 1."""
    c = _randint(1, 7, (N, K), gen) | (_randint(0, 1, (N, K), gen) << 3)
    even, odd = c[:, ::2], c[:, 1::2]
    c[:, 1::2] = torch.where(odd == even, ((odd & 7) % 7 + 1) | (odd & 8), odd)
    assert bool((c != c[:, torch.arange(K) ^ 1]).all()) and bool(((c & 7) != 0).all())
    return c.to(torch.uint8)


def scaled_values(fmt, q, s, weight=False):
    """float64 [rows, K]: the codes of one operand times their block scales. weight: q is the
    format's weight (packed e2m1 for mxfp4w; for blockfp8 s is the [ceil(N/128), K/128] array)."""
    v = F4_VALUES[unpack_fp4(q).long()] if (fmt == "mxfp4w" and weight) else decode(q)
    rows, K = v.shape
    if fmt == "blockfp8":
        f = s.double().repeat_interleave(128, 0)[:rows] if weight else s.double()
    else:
        f = e8m0(s)
    blk = BLOCK[fmt]
    return (v.reshape(rows, K // blk, blk) * f[..., None]).reshape(rows, K)


def _row_units(v):
    """float64 [rows]: per row, the largest power of two dividing every nonzero entry (all are
    multiples of 2^-18); 2^20 for an all-zero row."""
    i = (v.double() * 2.0 ** 18).round().long().abs()
    low = torch.where(i != 0, i & -i, torch.full_like(i, 1 << 38))
    return low.min(1).values.double() / 2.0 ** 18


def check_mfma_window(xv, wv, ux=None, uw=None):
    """tests/exact_inputs_fp8dyn.py's check for SCALED products: inside every aligned run of 128 k
    (one matrix instruction) max |x| * max |w| < 2^12 units of the output (ux(m) * uw(n))."""
    M, K = xv.shape
    N = wv.shape[0]
    ux = _row_units(xv) if ux is None else ux
    uw = _row_units(wv) if uw is None else uw
    pad = (-K) % 128

    def group_max(v):
        v = torch.nn.functional.pad(v.abs(), (0, pad))
        return v.reshape(v.shape[0], -1, 128).amax(-1)
    worst = (group_max(xv)[:, None, :] * group_max(wv)[None, :, :]).amax(-1)  # [M, N]
    unit = ux[:, None] * uw[None, :]
    assert bool((worst < 2 ** MFMA_WINDOW_BITS * unit).all()), (
        f"products of one MFMA span more than {MFMA_WINDOW_BITS} bits")
    return float((worst / unit).max())


def check_exact(fmt, xq, xs, wq, ws, bias=None):
    """The three conditions of the module docstring on operands as the ops take them. Returns
    (unit [M, N], the largest sum of magnitudes in units)."""
    xv, wv = scaled_values(fmt, xq, xs), scaled_values(fmt, wq, ws, weight=True)
    assert not bool(xv.isnan().any() | wv.isnan().any())
    ux, uw = _row_units(xv), _row_units(wv)
    unit = ux[:, None] * uw[None, :]
    mags = xv.abs() @ wv.abs().t()
    if bias is not None:
        b = bias.double()[None, :]
        assert bool(((b / unit) == (b / unit).round()).all()), "bias is no multiple of the unit"
        mags = mags + b.abs()
    assert bool((mags < 2 ** 24 * unit).all()), "a partial sum can leave the exact fp32 range"
    if fmt == "blockfp8":  # the instruction sees the bare codes (unit scale bytes)
        check_mfma_window(decode(xq), decode(wq))
    else:
        check_mfma_window(xv, wv, ux, uw)
    return unit, float((mags / unit).max())


def _bias(xe, we_rows, gen):
    """bf16 [N]: j * 2^t(n), 1 <= |j| <= 100, with 2^t(n) a multiple of every unit of column n: the x
    rows' units are at most 4 * 2^max(xe) (xe: their exponents [M, nblk]) and we_rows [N] is the
    exponent of each weight row's unit."""
    n = we_rows.shape[0]
    j = (_randint(1, 100, (n,), gen) * (_randint(0, 1, (n,), gen) * 2 - 1)).double()
    return (j * torch.exp2((int(xe.max()) + 2 + we_rows).double())).to(BF16)


# ---- makers ---------------------------------------------------------------------------------------

def make_mx_exact(M, N, K, seed, x_block_max=False):
    """MXFP8: xq uint8 [M, K], xs uint8 [M, K/32], wq uint8 [N, K], ws uint8 [N, K/32], bias bf16
    [N]; asserts the conditions."""
    gen = torch.Generator().manual_seed(7919 * seed + 11)
    nblk, h = K // 32, span_half(K, PMAX["mx"])
    a, c = _x_exponents(M, nblk, h, gen), _w_exponents(N, nblk, h, gen)
    xq = _e4m3(_x_ints(M, K, gen, 32 if x_block_max else None).double())
    wq = _e4m3(_randint(-W_MAX, W_MAX, (N, K), gen).double())
    xs, ws = (a + 127).to(torch.uint8), (c + 127).to(torch.uint8)
    bias = _bias(a, c.min(1).values, gen)
    check_exact("mx", xq, xs, wq, ws, bias)
    return xq, xs.contiguous(), wq, ws.contiguous(), bias


def make_mxfp4w_exact(M, N, K, seed, x_block_max=False):
    """MXFP4 weights: as make_mx_exact with wq uint8 [N, K/2], two e2m1 codes per byte."""
    gen = torch.Generator().manual_seed(7919 * seed + 13)
    nblk, h = K // 32, span_half(K, PMAX["mxfp4w"])
    a, c = _x_exponents(M, nblk, h, gen), _w_exponents(N, nblk, h, gen)
    xq = _e4m3(_x_ints(M, K, gen, 32 if x_block_max else None).double())
    wq = pack_fp4(_w_fp4_codes(N, K, gen))
    xs, ws = (a + 127).to(torch.uint8), (c + 127).to(torch.uint8)
    bias = _bias(a, c.min(1).values - 1, gen)  # e2m1 values are multiples of 1/2
    check_exact("mxfp4w", xq, xs, wq, ws, bias)
    return xq, xs.contiguous(), wq, ws.contiguous(), bias


def make_blockfp8_exact(M, N, K, seed):
    """Blockwise float8: xq uint8 [M, K], xs fp32 [M, K/128] = 2^a(m, b), wq uint8 [N, K], ws fp32
    [ceil(N/128), K/128] = 2^c(n / 128, b), bias bf16 [N]."""
    gen = torch.Generator().manual_seed(7919 * seed + 17)
    nblk, NB, h = K // 128, (N + 127) // 128, span_half(K, PMAX["blockfp8"])
    a, c = _x_exponents(M, nblk, h, gen), _w_exponents(NB, nblk, h, gen)
    xq = _e4m3(_x_ints(M, K, gen).double())
    wq = _e4m3(_randint(-W_MAX, W_MAX, (N, K), gen).double())
    xs, ws = torch.exp2(a.float()).contiguous(), torch.exp2(c.float()).contiguous()
    bias = _bias(a, c.min(1).values.repeat_interleave(128)[:N], gen)
    check_exact("blockfp8", xq, xs, wq, ws, bias)
    return xq, xs, wq, ws, bias


MAKERS = {"mx": make_mx_exact, "mxfp4w": make_mxfp4w_exact, "blockfp8": make_blockfp8_exact}


# ---- references ---------------------------------------------------------------------------------

def _finish(acc, bias, check):
    """bf16(fp32(acc + bias)) of the float64 sum: one rounding when the sums are fp32 numbers."""
    acc32 = acc.float()
    if check:
        ok = (acc32.double() == acc) | acc.isnan()
        assert bool(ok.all()), "reference sum is not an fp32 number"
    if bias is None:
        return acc32.to(BF16)
    y = acc + bias.double()[None, :]
    y32 = acc32 + bias.float()[None, :]
    if check:
        ok = (y32.double() == y) | y.isnan()
        assert bool(ok.all()), "reference sum + bias is not an fp32 number"
    return y32.to(BF16)


def ref_mx(xq, xs, wq, ws, bias=None, check=True):
    """csrc/mx_fp8.hip: y = bf16(sum_b 2^(xs - 127) 2^(ws - 127) sum_k f(xq) f(wq) + bias)."""
    xv, wv = scaled_values("mx", xq, xs), scaled_values("mx", wq, ws, weight=True)
    return _finish(xv @ wv.t(), bias, check)


def ref_mxfp4w(xq, xs, wq, ws, bias=None, check=True):
    """csrc/mx_fp4.hip: ref_mx with e2m1 weight codes, element 2 j in the high nibble."""
    xv, wv = scaled_values("mxfp4w", xq, xs), scaled_values("mxfp4w", wq, ws, weight=True)
    return _finish(xv @ wv.t(), bias, check)


def ref_blockfp8(xq, xs, wq, ws, bias=None, check=True):
    """csrc/block_fp8.hip: y = bf16(sum_b P[m][n][b] * (xs[m][b] * ws[n / 128][b]) + bias), P the
    dot product of block b's 128 code pairs."""
    N, K = wq.shape
    xf = decode(xq).reshape(-1, K // 128, 128)
    wf = decode(wq).reshape(N, K // 128, 128)
    P = torch.einsum("mbk,nbk->mnb", xf, wf)
    f = xs.double().reshape(-1, 1, K // 128) * ws.double().repeat_interleave(128, 0)[:N][None]
    return _finish((P * f).sum(-1), bias, check)


REFS = {"mx": ref_mx, "mxfp4w": ref_mxfp4w, "blockfp8": ref_blockfp8}


# ---- identity tokens ------------------------------------------------------------------------------

def _mx_identity(fmt, N, K, seed):
    xq, xs, wq, ws, bias = MAKERS[fmt](1, N, K, seed, x_block_max=True)
    ints = decode(xq)
    p = xs.long() - 127                                    # [1, K/32]
    token = (ints.reshape(1, -1, 32) * torch.exp2(p.double())[..., None]).reshape(1, K)
    xb = token.to(BF16)
    assert torch.equal(xb.double(), token)
    codes = _e4m3(64.0 * ints)                             # amax 4 * 2^p -> scale 2^(p - 6)
    scale = (p - 6 + 127).to(torch.uint8)
    assert torch.equal(scaled_values("mx", codes, scale), token)
    check_exact(fmt, codes, scale, wq, ws, bias)
    return xb, codes, scale.contiguous(), wq, ws, bias


def make_mx_identity_token(N, K, seed):
    """A bf16 token [1, K] on which the MX quantizer (FLOOR) is the identity: every 32-block is
    integers in [-4, 4] with at least one +-4, times 2^p(block). The block's amax is 2^(p + 2), its
    scale byte p - 6 + 127 and its codes 64 x the integers. Returns the token, the codes, the scale
    bytes and the weight operands (wq, ws, bias) of make_mx_exact."""
    return _mx_identity("mx", N, K, seed)


def make_mxfp4w_identity_token(N, K, seed):
    """make_mx_identity_token with the weight operands of make_mxfp4w_exact."""
    return _mx_identity("mxfp4w", N, K, seed)


def make_blockfp8_identity_token(N, K, seed):
    """tests/exact_inputs_fp8dyn.py's construction per 128-block: integers in [-4, 4] with one
    +-448, times 2^p(block). amax = 448 * 2^p, so the scale is exactly 2^p and the codes are the
    integers. Returns the token, the codes, the scales [1, K/128] and (wq, ws, bias)."""
    gen = torch.Generator().manual_seed(7919 * seed + 19)
    nblk, NB = K // 128, (N + 127) // 128
    h = span_half(K, PMAX["blockfp8"], extra=nblk * (448 * W_MAX - PMAX["blockfp8"]))
    a, c = _x_exponents(1, nblk, h, gen), _w_exponents(NB, nblk, h, gen)
    ints = _x_ints(1, K, gen)
    pos = _randint(0, 127, (1, nblk), gen) + 128 * torch.arange(nblk)[None, :]
    ints.scatter_(1, pos, (_randint(0, 1, (1, nblk), gen) * 2 - 1) * 448)
    token = (ints.double().reshape(1, nblk, 128) * torch.exp2(a.double())[..., None]).reshape(1, K)
    xb = token.to(BF16)
    assert torch.equal(xb.double(), token)
    codes = _e4m3(ints.double())
    wq = _e4m3(_randint(-W_MAX, W_MAX, (N, K), gen).double())
    xs, ws = torch.exp2(a.float()).contiguous(), torch.exp2(c.float()).contiguous()
    bias = _bias(a, c.min(1).values.repeat_interleave(128)[:N], gen)
    check_exact("blockfp8", codes, xs, wq, ws, bias)
    return xb, codes, xs, wq, ws, bias


IDENTITY = {"mx": make_mx_identity_token, "mxfp4w": make_mxfp4w_identity_token,
            "blockfp8": make_blockfp8_identity_token}


# ---- launch rules, restated (csrc/tao_gemv.h gemv_launch_shape, csrc/fp8_dyn_host.h) -------------

def gemv_launch(K, chunk_k, wk, g):
    """(S, Wk, G): S slices of 64 lanes x chunk_k k per row, Wk = min(wk, S) waves along K, G row
    groups halved until Wk * G <= 8. chunk_k: 16 (one-byte codes), 32 (mxfp4w's e2m1 weights)."""
    S = (K // chunk_k + 63) // 64
    Wk = min(wk, S)
    while g > 1 and Wk * g > 8:
        g >>= 1
    return S, Wk, g


def fused_launch(fmt, K):
    """(NPT, S, Wk, threads) of the one-token *_dyn_linear launch, (wk, g) = (4, 2): the token's
    K / 8 16-B pieces spread over the threads, rounded up to the instantiated 1, 2, 4, 8, 16."""
    S, Wk, G = gemv_launch(K, 32 if fmt == "mxfp4w" else 16, 4, 2)
    threads = 64 * Wk * G
    while 64 * Wk * G * 8 * 16 < K and Wk * G * 2 <= 8:
        G *= 2
        threads = 64 * Wk * G
    per = (K // 8 + threads - 1) // threads
    npt = next(n for n in (1, 2, 4, 8, 16) if per <= n)
    return npt, S, Wk, threads


def plain_gemv_launch(fmt, M, K):
    """(S, Wk, G) of the GEMV on ready-made codes: (wk, g) = (8, 1) at M = 1, (8, 8) above."""
    return gemv_launch(K, 32 if fmt == "mxfp4w" else 16, 8, 1 if M <= 1 else 8)


# ---- the shapes of tests/test_gpu_exact_blockscaled.py -----------------------------------------
MFMA_M = (1, 5, 16, 17, 33, 65, 130)
MFMA_N = (16, 37, 80)
MFMA_N_BLOCK = (40, 129, 272)  # one, two and three scale rows of the blockwise weight, ragged N
# 32, 96: tails inside the first MFMA; 128, 256: exactly one MFMA / one step; 288: a tail of one
# block in the second step; 384: the second step's first MFMA full; 256, 512, 2048: the aligned
# policy (K % 256 == 0); 1056: five steps
MX_K = (32, 96, 128, 256, 288, 384, 512, 1056, 2048)
BLOCK_K = (128, 256, 384, 1152, 2048)
# (M tile, k-groups, K slices). BlockFp8 clamps the M tile to 64: the 128 entries run as 64 there
FORCED_TILES = [(16, 1, 1), (16, 2, 1), (16, 1, 2), (32, 2, 3), (64, 1, 3), (64, 2, 2),
                (128, 1, 1), (128, 1, 2)]
# 1056 and 1152 are five steps: splits = 3 gives slices of 2, 2 and 1 steps (uneven, the last one
# shorter than two k-groups, so k-group 1 idles there); 288 / 384 are two steps: splits = 2 or 3
# gives one-step slices, idle under KG = 2 as well, and the second slice starts at step 1 with a
# K tail; 2048 is eight steps (aligned policy), slices 4 + 4 and 3 + 3 + 2
FORCED_MNK = {
    "mx": [(33, 37, 288), (130, 80, 1056), (70, 37, 2048), (17, 16, 384)],
    "mxfp4w": [(33, 37, 288), (130, 80, 1056), (70, 37, 2048), (17, 16, 384)],
    "blockfp8": [(33, 129, 384), (130, 272, 1152), (70, 129, 2048), (17, 272, 256)],
}
GEMV_M = (1, 2, 3, 4, 5, 8)
GEMV_N = (1, 37)
# The fused launch (fused_launch above): one-byte codes (mx, blockfp8) have 1024-k slices, so
# threads = 128 / 256 / 384 / 512 at S = 1 / 2 / 3 / >= 4 and NPT = 1 up to K = 4096; 4128 / 4224
# -> NPT 2, 8224 / 8320 -> 4, 16416 / 16512 -> 8, 32800 / 32896 -> 16, all with S > Wk = 4.
# mxfp4w has 2048-k slices: 1056 runs 128 threads with NPT 2, 4128 384 threads (Wk = 3) NPT 2,
# 8224 -> 4 (S = 5 > Wk), 16416 -> 8, 32800 -> 16.
# The plain GEMV (wk = 8): S > Wk from K > 8192 (mxfp4w: K > 16384), i.e. 8224 (S = 9), 16416
# (S = 17; mxfp4w S = 9) and up; 4128 / 4224 are S = 5 = Wk with the last wave on a short slice.
GEMV_K_MX = (32, 1024, 1056, 4128, 8224, 16416)
GEMV_K_BLOCK = (128, 1152, 4224, 8320, 16512)
GEMV_K_NPT16 = {"mx": 32800, "mxfp4w": 32800, "blockfp8": 32896}  # N = 37 only


def mfma_k(fmt):
    return BLOCK_K if fmt == "blockfp8" else MX_K


def mfma_n(fmt):
    return MFMA_N_BLOCK if fmt == "blockfp8" else MFMA_N


def gemv_k(fmt):
    return GEMV_K_BLOCK if fmt == "blockfp8" else GEMV_K_MX


def seed_of(M, N, K):
    return (M * 31 + N * 7 + K) % 1000
