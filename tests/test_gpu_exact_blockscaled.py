"""Bit-exact GPU tests of every route of the three block-scaled linears: MXFP8 (mx_scaled_mm,
mx_dyn_linear), MXFP4 weights (mxfp4w_scaled_mm, mxfp4w_dyn_linear) and blockwise float8
(blockfp8_scaled_mm, blockfp8_dyn_linear).

On the inputs of tests/exact_inputs_blockscaled.py every scaled product and every partial sum is
an exact fp32 number inside the matrix instruction's exact window, so the output must equal
bf16(sum + bias) of the float64 sum bit for bit, whatever the M tile, the k-groups, the split-K
slices, the columns per wave, the scale-load policy (aligned 8-B words or bytes) or the GEMV's
launch shape. x and w are unrelated random codes and the scales differ per (row, block), so a k
permutation between the operands, a scale from a neighbouring block or row, or a lost 16-B piece
next to a tail changes the bits. No tolerance: a mismatch is a kernel bug. Each case asserts the
kernel family it meant to run through tao_last_kernel; which (BM, KG, splits, NW, AL) and which
token-piece count (NPT) a case reaches follows from the launch rules (choose_shape and launch_gemm in
csrc/gemm_mfma.hip, csrc/fp8_dyn_host.h; restated in exact_inputs_blockscaled.fused_launch).
"""

import functools

import pytest
import torch

import exact_inputs_blockscaled as E

from torchao import _lib
from torchao.kernel import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
T = torch.ops.torchao
MFMA = "gemm_mfma"
GEMV = {"mx": "mx_gemv", "mxfp4w": "mxw4_gemv", "blockfp8": "blockfp8_gemv"}
FORCE_MFMA = {"mx": {"mx_mfma": 1}, "mxfp4w": {"mx_mfma": 1}, "blockfp8": {"blockfp8_mfma": 1}}
FMT = pytest.mark.parametrize("fmt", E.FORMATS)


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _dev(fmt, xq, xs, wq, ws, bias):
    """The operands as the ops take them, on the GPU."""
    w = wq if fmt == "mxfp4w" else wq.view(FP8)
    return (xq.view(FP8).to(DEV), xs.to(DEV), w.to(DEV), ws.to(DEV),
            None if bias is None else bias.to(DEV))


def _mm(fmt, xq, xs, wq, ws, bias):
    op = {"mx": T.mx_scaled_mm, "mxfp4w": T.mxfp4w_scaled_mm, "blockfp8": T.blockfp8_scaled_mm}[fmt]
    return op(xq, xs, wq, ws, bias)


def _dyn(fmt, x, wq, ws, bias):
    op = {"mx": T.mx_dyn_linear, "mxfp4w": T.mxfp4w_dyn_linear, "blockfp8": T.blockfp8_dyn_linear}[fmt]
    return op(x, wq, ws, bias)


def _quant(fmt, x):
    return T.blockfp8_quantize_act(x) if fmt == "blockfp8" else T.mx_quantize_rows(x)


@functools.lru_cache(maxsize=64)
def _inputs(fmt, M, N, K):
    ops = E.MAKERS[fmt](M, N, K, E.seed_of(M, N, K))
    want, want_b = E.REFS[fmt](*ops[:4]), E.REFS[fmt](*ops)
    return ops, _dev(fmt, *ops), want, want_b


def check(route, fmt, M, N, K, kernel):
    _, (xq, xs, wq, ws, bias), want, want_b = _inputs(fmt, M, N, K)
    for b, ref in ((None, want), (bias, want_b)):
        got = _mm(fmt, xq, xs, wq, ws, b).cpu()
        assert kernel in _last_kernel(), (route, _last_kernel())
        where = f"{route} {fmt} M={M} N={N} K={K} bias={'on' if b is not None else 'off'}"
        assert got.shape == ref.shape, where
        assert torch.equal(got, ref), E.describe_mismatch(f"{where} kernel={_last_kernel()}", got, ref)


# ---- the MFMA kernel ------------------------------------------------------------------------------

def _fmt_n_k():
    return [(f, n, k) for f in E.FORMATS for n in E.mfma_n(f) for k in E.mfma_k(f)]


@pytest.mark.parametrize("fmt,N,K", _fmt_n_k())
def test_mfma_every_m(fmt, N, K):
    """Built-in tiles; the MFMA route at every M (below the crossover too)."""
    with tuning(**FORCE_MFMA[fmt]):
        for M in E.MFMA_M:
            check("mfma", fmt, M, N, K, MFMA)


@FMT
def test_mfma_is_the_built_in_route_above_the_crossover(fmt):
    N, K = (129, 384) if fmt == "blockfp8" else (37, 288)
    for M in (5, 16, 33):
        check("mfma built-in", fmt, M, N, K, MFMA)


@FMT
def test_mfma_built_in_shape_picks_two_k_groups(fmt):
    """M >= 4 x 64 rows at a small N: choose_shape stops at the 64-row tile (too few tiles for the
    224 of the short-K rule), does not split (K has fewer steps than two slices need) and so gives
    the preferred one k-group a second one: (BM 64, KG 2, splits 1) with no tile forced."""
    N, K = (129, 1152) if fmt == "blockfp8" else (37, 1056)
    check("mfma built-in kg 2", fmt, 260, N, K, MFMA)


@pytest.mark.parametrize("bm,kg,splits", E.FORCED_TILES)
@FMT
def test_mfma_forced_tiles_and_split_k(fmt, bm, kg, splits):
    with tuning(gemm=(bm, kg, splits), **FORCE_MFMA[fmt]):
        for M, N, K in E.FORCED_MNK[fmt]:
            check(f"mfma bm={bm} kg={kg} splits={splits}", fmt, M, N, K, MFMA)


NW2_TILES = [t for t in E.FORCED_TILES if t[0] <= 64] + [(32, 1, 2)]


@pytest.mark.parametrize("bm,kg,splits", NW2_TILES)
@FMT
def test_mfma_two_column_blocks_per_wave(fmt, bm, kg, splits):
    """gemm_nw = 2: 32 columns per wave, instantiated for every policy at BM <= 64, KG <= 2 (each
    A fragment and each pair of x scale bytes feeds two MFMAs; two weight stages per wave)."""
    with tuning(gemm=(bm, kg, splits), gemm_nw=2, **FORCE_MFMA[fmt]):
        for M, N, K in E.FORCED_MNK[fmt]:
            check(f"mfma nw=2 bm={bm} kg={kg} splits={splits}", fmt, M, N, K, MFMA)


@pytest.mark.parametrize("bm,kg,splits", [(32, 2, 3), (128, 1, 2)])
@FMT
def test_mfma_fenced_split_k(fmt, bm, kg, splits):
    """The split-K hand-off with the agent fences, at uneven slices with an idle k-group and at
    the largest tile."""
    with tuning(gemm=(bm, kg, splits), splitk_fenced=1, **FORCE_MFMA[fmt]):
        for M, N, K in E.FORCED_MNK[fmt]:
            check(f"mfma fenced bm={bm} kg={kg} splits={splits}", fmt, M, N, K, MFMA)


def _odd(t):
    """The same bytes at an odd address (a view one byte into a larger buffer)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


@pytest.mark.parametrize("K", (256, 512, 2048))
@pytest.mark.parametrize("fmt", ("mx", "mxfp4w"))
def test_aligned_and_unaligned_scale_policies_agree(fmt, K):
    """K % 256 == 0 takes the aligned policy (8-B scale words, v_perm regroup). The same operands
    with one more block of zero codes (K + 32) take the byte-load policy and add exactly 0, so
    both must give the same reference; scale views at an odd address are realigned by the op and
    change nothing. Forced at the 16-row and the 128-row tile, one and two k-groups."""
    N = 37
    for M, tile in ((17, (16, 2, 1)), (130, (128, 1, 2)), (70, (64, 2, 3)), (33, (0, 0, 0))):
        (xq, xs, wq, ws, bias), dev, _, want_b = _inputs(fmt, M, N, K)
        pad_q = torch.zeros(M, 32, dtype=torch.uint8)
        pad_w = torch.zeros(N, 32 if fmt == "mx" else 16, dtype=torch.uint8)
        one = torch.full((1,), 127, dtype=torch.uint8)
        longer = (torch.cat([xq, pad_q], 1), torch.cat([xs, one.expand(M, 1)], 1),
                  torch.cat([wq, pad_w], 1), torch.cat([ws, one.expand(N, 1)], 1), bias)
        assert torch.equal(E.REFS[fmt](*longer), want_b)
        with tuning(gemm=tile, **FORCE_MFMA[fmt]):
            where = f"{fmt} M={M} K={K} tile={tile}"
            got = _mm(fmt, *dev).cpu()
            assert MFMA in _last_kernel()
            assert torch.equal(got, want_b), E.describe_mismatch(f"aligned {where}", got, want_b)
            got = _mm(fmt, dev[0], _odd(dev[1]), dev[2], _odd(dev[3]), dev[4]).cpu()
            assert MFMA in _last_kernel()
            assert torch.equal(got, want_b), E.describe_mismatch(f"odd views {where}", got, want_b)
            got = _mm(fmt, *_dev(fmt, *longer)).cpu()
            assert MFMA in _last_kernel()
            assert torch.equal(got, want_b), E.describe_mismatch(f"K + 32 {where}", got, want_b)


# ---- NaN next to a K tail -------------------------------------------------------------------------

def _nan_k():
    return [(f, k) for f in E.FORMATS for k in ((384, 1152) if f == "blockfp8" else (288, 1056, 96))]


@pytest.mark.parametrize("fmt,K", _nan_k())
def test_k_tail_next_to_nan_rows(fmt, K):
    """The last step reads past the row into the next row's codes and clamps its scale index, on
    both operands. With one token and one weight row in the middle and the last of each poisoned
    (NaN codes and NaN scales; e2m1 has no NaN code, so scale bytes only; the blockwise weight's
    last row is alone in its 128-row scale block, which is made NaN / inf), only their own output
    rows / columns may be NaN, and every other element equals the exact reference."""
    M, N = 33, (129 if fmt == "blockfp8" else 37)
    (xq, xs, wq, ws, _), _, want, _ = _inputs(fmt, M, N, K)
    x2, xs2, w2, ws2 = xq.clone(), xs.clone(), wq.clone(), ws.clone()
    pm, pn = (3, M - 1), (5, N - 1)
    x2[3], x2[M - 1] = 0x7F, 0xFF
    if fmt == "blockfp8":
        xs2[3], xs2[M - 1] = float("nan"), float("inf")
        w2[5], w2[N - 1] = 0x7F, 0xFF
        ws2[1, 0::2], ws2[1, 1::2] = float("nan"), float("inf")
    else:
        xs2[3], xs2[M - 1] = 0xFF, 0xFF
        ws2[5], ws2[N - 1] = 0xFF, 0xFF
        if fmt == "mx":
            w2[5], w2[N - 1] = 0x7F, 0xFF
    ref = E.REFS[fmt](x2, xs2, w2, ws2)
    rows = [m for m in range(M) if m not in pm]
    cols = [n for n in range(N) if n not in pn]
    assert torch.equal(ref[rows][:, cols], want[rows][:, cols])  # the test's own algebra
    assert bool(ref[list(pm)].isnan().all()) and bool(ref[:, list(pn)].isnan().all())
    dev = _dev(fmt, x2, xs2, w2, ws2, None)

    def verify(got, m_rows, nan_rows, tag):
        assert bool(got[:, list(pn)].isnan().all()) and bool(got[nan_rows].isnan().all()), tag
        fin = got[m_rows][:, cols]
        assert not bool(fin.isnan().any()), f"{tag}: a NaN past the K tail reached the sum"
        assert torch.equal(fin, want[m_rows][:, cols]), E.describe_mismatch(
            tag, fin, want[m_rows][:, cols])

    for bm in (16, 128):  # BlockFp8 runs 128 as 64
        with tuning(gemm=(bm, 0, 0), **FORCE_MFMA[fmt]):
            got = _mm(fmt, *dev).cpu()
            assert MFMA in _last_kernel()
        verify(got, rows, list(pm), f"{fmt} K={K} mfma bm={bm}")
    with tuning(linear_crossover=8):  # and the GEMV's clamped tail lanes
        got = _mm(fmt, dev[0][:5], dev[1][:5], dev[2], dev[3], None).cpu()
        assert GEMV[fmt] in _last_kernel()
    verify(got, [0, 1, 2, 4], [3], f"{fmt} K={K} gemv")


# ---- the GEMV -----------------------------------------------------------------------------------------

def _fmt_n_gemv_k():
    out = [(f, n, k) for f in E.FORMATS for n in E.GEMV_N for k in E.gemv_k(f)]
    return out + [(f, 37, E.GEMV_K_NPT16[f]) for f in E.FORMATS]


@pytest.mark.parametrize("fmt,N,K", _fmt_n_gemv_k())
def test_gemv(fmt, N, K):
    with tuning(linear_crossover=8):
        for M in E.GEMV_M:
            check("gemv", fmt, M, N, K, GEMV[fmt])


@FMT
def test_crossover_moved_both_ways(fmt):
    """Each M near the built-in crossover (GEMV at M = 1, and up to M = 4 on small weights) runs
    on both kernels and gives the same bits."""
    N, K = (129, 1152) if fmt == "blockfp8" else (37, 1056)
    for M in (1, 2, 3, 4, 5, 8):
        with tuning(linear_crossover=8):
            check("crossover 8", fmt, M, N, K, GEMV[fmt])
        if M > 1:
            with tuning(linear_crossover=1):
                check("crossover 1", fmt, M, N, K, MFMA)
    check("built-in", fmt, 2, N, K, GEMV[fmt])
    check("built-in", fmt, 5, N, K, MFMA)


# ---- the fused one-token launch --------------------------------------------------------------------------

def _fmt_n_fused_k():
    out = [(f, n, k) for f in E.FORMATS for n in (37, 80) for k in E.gemv_k(f)]
    return out + [(f, 37, E.GEMV_K_NPT16[f]) for f in E.FORMATS]


@pytest.mark.parametrize("fmt,N,K", _fmt_n_fused_k())
def test_fused_one_token_equals_quantize_then_scaled_mm(fmt, N, K):
    """The quantizer is the identity on the token's known codes and scales; the one-launch linear
    (every NPT of 1, 2, 4, 8, 16 over the K list, and more slices than waves along K) equals
    quantizer -> scaled mm bit for bit, and both equal the reference."""
    for seed in (1, 2):
        xb, codes, scale, wq, ws, bias = E.IDENTITY[fmt](N, K, seed + K % 5)
        x = xb.to(DEV)
        _, _, w, wsd, b = _dev(fmt, codes, scale, wq, ws, bias)
        q, s = _quant(fmt, x)
        assert torch.equal(q.view(torch.uint8).cpu(), codes), (fmt, K, "codes")
        assert torch.equal(s.cpu().reshape(scale.shape), scale), (fmt, K, "scales")
        for bb in (None, b):
            two = _mm(fmt, q, s, w, wsd, bb)
            assert GEMV[fmt] in _last_kernel()
            one = _dyn(fmt, x, w, wsd, bb)
            assert GEMV[fmt] in _last_kernel()
            ref = E.REFS[fmt](codes, scale, wq, ws, None if bb is None else bias)
            assert torch.equal(one.cpu(), ref), E.describe_mismatch(
                f"fused {fmt} N={N} K={K}", one.cpu(), ref)
            assert torch.equal(two.cpu(), ref), E.describe_mismatch(
                f"quantize + mm {fmt} N={N} K={K}", two.cpu(), ref)
            assert torch.equal(one, two)
