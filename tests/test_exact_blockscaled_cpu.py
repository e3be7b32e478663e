"""CPU checks of tests/exact_inputs_blockscaled.py: the inputs of the bit-exact GPU tests of the
MXFP8, MXFP4-weight and blockwise float8 linears really are order-independent, the identity tokens
really quantise to the stated codes, and the exact comparison really sees the faults a block-scaled
kernel can have.

  * the makers' conditions hold at every shape tests/test_gpu_exact_blockscaled.py runs, and the
    K lists reach the launch instances they are there for (every NPT, S > Wk);
  * order independence: fp32 accumulation in three orders (forward; the GEMV's 16-k chunks over
    64 lanes; 128-k MFMAs over steps, two k-groups and three split-K slices) equals the float64 sum;
  * the identity tokens under to_mx and fp8_blockwise_act_quant;
  * mutations: at every forced shape, each single fault changes at least one output bit.
"""

import pytest
import torch

import exact_inputs_blockscaled as E

from torchao.prototype.blockwise_fp8_inference import fp8_blockwise_act_quant
from torchao.prototype.mx_formats.mx_tensor import to_mx

FMT = pytest.mark.parametrize("fmt", E.FORMATS)
FP8 = torch.float8_e4m3fn


def _make(fmt, M, N, K):
    return E.MAKERS[fmt](M, N, K, E.seed_of(M, N, K))


# ---- conditions at every GPU shape ---------------------------------------------------------------

@FMT
def test_conditions_hold_at_every_gpu_shape(fmt):
    shapes = {(M, N, K) for M in E.MFMA_M for N in E.mfma_n(fmt) for K in E.mfma_k(fmt)}
    shapes |= set(E.FORCED_MNK[fmt])
    shapes |= {(M, N, K) for M in E.GEMV_M for N in E.GEMV_N for K in E.gemv_k(fmt)}
    shapes |= {(M, 37, E.GEMV_K_NPT16[fmt]) for M in E.GEMV_M}
    shapes |= {(260, 129 if fmt == "blockfp8" else 37, 1152 if fmt == "blockfp8" else 1056)}
    worst = 0.0
    for M, N, K in sorted(shapes):
        ops = _make(fmt, M, N, K)  # asserts
        _, mags = E.check_exact(fmt, *ops)
        worst = max(worst, mags)
        y, yb = E.REFS[fmt](*ops[:4]), E.REFS[fmt](*ops)  # assert that their sums are fp32 numbers
        assert y.shape == (M, N) and y.dtype is torch.bfloat16 and not bool(y.isnan().any())
        assert not torch.equal(y, yb)
    assert worst < 2 ** 24
    # the scales are not constant: every row has more than one where it has more than one block
    xq, xs, wq, ws, _ = _make(fmt, 33, 129 if fmt == "blockfp8" else 37, 1152)
    assert bool((xs[:, 1:] != xs[:, :-1]).all()) and bool((ws[:, 1:] != ws[:, :-1]).all())
    assert bool((xs[1:] != xs[:-1]).any()) and bool((ws[1:] != ws[:-1]).any())
    assert len(set(xq.flatten().tolist())) == 9  # all of [-4, 4]
    # the row units are tests/exact_inputs_fp8dyn.py's _lowbit_unit, row by row
    xv = E.scaled_values(fmt, xq, xs)
    assert E._row_units(xv).tolist() == [E._lowbit_unit(xv[m]) for m in range(xv.shape[0])]


def test_mxfp4_weights_use_every_nonzero_code_and_differ_within_a_byte():
    _, _, wq, _, _ = _make("mxfp4w", 5, 37, 1056)
    c = E.unpack_fp4(wq)
    assert set(c.flatten().tolist()) == set(range(1, 8)) | set(range(9, 16))
    assert bool((c[:, ::2] != c[:, 1::2]).all())
    assert torch.equal(E.pack_fp4(c), wq)
    assert int(wq[0, 0]) >> 4 == int(c[0, 0])  # element 2 j in the high nibble


def test_k_lists_reach_every_fused_instance_and_looped_slices():
    for fmt in E.FORMATS:
        ks = E.gemv_k(fmt) + (E.GEMV_K_NPT16[fmt],)
        fused = {K: E.fused_launch(fmt, K) for K in ks}
        assert {v[0] for v in fused.values()} == {1, 2, 4, 8, 16}, fused
        assert all(v[3] <= 512 for v in fused.values())
        assert any(S > Wk for _, S, Wk, _ in fused.values())
        assert fused[E.GEMV_K_NPT16[fmt]][0] == 16
        for M in (1, 2, 8):
            plain = [E.plain_gemv_launch(fmt, M, K) for K in ks]
            assert any(S > Wk for S, Wk, _ in plain) and any(S == 1 for S, _, _ in plain)
            assert all(Wk * G <= 8 for _, Wk, G in plain)
    # the thresholds named in the issue: NPT > 1 starts just above K = 4096 at 512 threads, the
    # plain GEMV loops over slices from K > 8192 (one-byte codes)
    assert E.fused_launch("mx", 4096) == (1, 4, 4, 512) and E.fused_launch("mx", 4128)[0] == 2
    assert E.plain_gemv_launch("mx", 1, 8192) == (8, 8, 1)
    assert E.plain_gemv_launch("mx", 1, 8224) == (9, 8, 1)


def test_forced_shapes_hold_the_uneven_and_the_idle_slices():
    for fmt in E.FORMATS:
        steps = [(K + 255) // 256 for _, _, K in E.FORCED_MNK[fmt]]
        assert 5 in steps  # splits = 3: sps = 2, slices of 2, 2 and 1 steps
        sps = (5 + 3 - 1) // 3
        assert [min(sps, 5 - s) for s in range(0, 5, sps)] == [2, 2, 1]
        assert (32, 2, 3) in E.FORCED_TILES  # ... under two k-groups: the last slice idles one
        assert any(K % 256 == 0 for _, _, K in E.FORCED_MNK[fmt])
        assert any(K % 256 != 0 for _, _, K in E.FORCED_MNK[fmt])


# ---- order independence ---------------------------------------------------------------------------

def _scaled_f32(fmt, xq, xs, wq, ws):
    xv, wv = E.scaled_values(fmt, xq, xs), E.scaled_values(fmt, wq, ws, weight=True)
    x32, w32 = xv.float(), wv.float()
    assert torch.equal(x32.double(), xv) and torch.equal(w32.double(), wv)
    return x32, w32


def _order_forward(x, w):
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k in range(x.shape[1]):
        acc = acc + x[:, k, None] * w[None, :, k]
    return acc


def _order_gemv(x, w):
    """A 16-k chunk c goes to lane c % 64 (slices in ascending order per lane), its 16 products
    added one by one, then into the lane's sum; the lanes are summed pairwise afterwards."""
    M, K = x.shape
    lanes = torch.zeros(M, w.shape[0], 64)
    for c in range(K // 16):
        d = torch.zeros(M, w.shape[0])
        for k in range(16 * c, 16 * c + 16):
            d = d + x[:, k, None] * w[None, :, k]
        lanes[:, :, c % 64] = lanes[:, :, c % 64] + d
    while lanes.shape[-1] > 1:
        lanes = lanes[..., 0::2] + lanes[..., 1::2]
    return lanes[..., 0]


def _order_mfma(x, w, kg=2, splits=3):
    """128-k sums (one matrix instruction each, added in fp32 by torch), two per 256-k step; a
    slice's steps alternate between the k-groups, each with its own accumulator; k-groups are
    summed in order, then the slices in order (csrc/gemm_mfma.hip)."""
    M, K = x.shape
    nsteps = (K + 255) // 256
    sps = (nsteps + splits - 1) // splits
    total = torch.zeros(M, w.shape[0])
    for s0 in range(0, nsteps, sps):
        s1 = min(s0 + sps, nsteps)
        groups = []
        for g in range(kg):
            acc = torch.zeros(M, w.shape[0])
            for st in range(s0 + g, s1, kg):
                for u in range(2):
                    k0 = 256 * st + 128 * u
                    if k0 < K:
                        acc = acc + x[:, k0:k0 + 128] @ w[:, k0:k0 + 128].t()
            groups.append(acc)
        part = groups[0]
        for a in groups[1:]:
            part = part + a
        total = total + part
    return total


@pytest.mark.parametrize("M,N,K", [(3, 9, 1056), (2, 5, 2048), (1, 4, 8320)])
@FMT
def test_accumulation_order_does_not_matter(fmt, M, N, K):
    if fmt == "blockfp8":
        K = (K + 127) // 128 * 128
    xq, xs, wq, ws, bias = _make(fmt, M, N, K)
    x, w = _scaled_f32(fmt, xq, xs, wq, ws)
    want = x.double() @ w.double().t()
    for name, got in (("forward", _order_forward(x, w)), ("gemv chunks", _order_gemv(x, w)),
                      ("mfma steps", _order_mfma(x, w))):
        assert got.dtype is torch.float32 and torch.equal(got.double(), want), name
    assert torch.equal(E.REFS[fmt](xq, xs, wq, ws), want.float().to(torch.bfloat16))
    yb = (want + bias.double()[None, :])
    assert torch.equal(yb.float().double(), yb)
    assert torch.equal(E.REFS[fmt](xq, xs, wq, ws, bias), yb.float().to(torch.bfloat16))


# ---- identity tokens ------------------------------------------------------------------------------

@FMT
def test_identity_tokens_quantise_to_the_stated_codes(fmt):
    for K in E.gemv_k(fmt) + (E.GEMV_K_NPT16[fmt],):
        for seed in (1, 2, 3):
            xb, codes, scale, wq, ws, bias = E.IDENTITY[fmt](37, K, seed + K % 5)
            assert xb.dtype is torch.bfloat16 and xb.shape == (1, K)
            if fmt == "blockfp8":
                q, s = fp8_blockwise_act_quant(xb)
                assert s.dtype is torch.float32 and torch.equal(s, scale)
                assert bool((E.decode(codes).abs().reshape(-1, 128).amax(1) == 448).all())
            else:
                s, q = to_mx(xb, FP8, 32)
                assert torch.equal(s.view(torch.uint8), scale)
                assert bool((E.decode(codes).abs().reshape(-1, 32).amax(1) == 256).all())
            assert torch.equal(q.view(torch.uint8), codes)
            # the codes times the scales are the token itself
            assert torch.equal(E.scaled_values(fmt, codes, scale), xb.double())
            E.REFS[fmt](codes, scale, wq, ws, bias)  # asserts exactness


# ---- mutation check ---------------------------------------------------------------------------------

def _swap_cols(t, i, j):
    out = t.clone()
    out[:, i], out[:, j] = t[:, j], t[:, i]
    return out


def _mutations(fmt, xq, xs, wq, ws):
    """name -> operands carrying one fault of the kind a block-scaled kernel can have. Faults on
    the k axis are applied to every row (what a wrong lane map does)."""
    M, K = xq.shape
    N = wq.shape[0]
    blk = E.BLOCK[fmt]
    nblk = K // blk
    fp4 = fmt == "mxfp4w"
    wc = E.unpack_fp4(wq) if fp4 else wq          # one weight code per k

    def w_of(codes):
        return E.pack_fp4(codes) if fp4 else codes

    out = {}
    # two k swapped inside one block of one operand only (first, a middle and the last block)
    for b in sorted({0, nblk // 2, nblk - 1}):
        k0 = b * blk
        for i, j in ((k0, k0 + 1), (k0 + 3, k0 + blk - 1)):
            out[f"x: k {i} <-> {j}"] = (_swap_cols(xq, i, j), xs, wq, ws)
            out[f"w: k {i} <-> {j}"] = (xq, xs, w_of(_swap_cols(wc, i, j)), ws)
    # the scale of block b taken from block b +- 1, for every row
    for b in sorted({0, nblk // 2, nblk - 1}):
        for d in (-1, 1):
            if 0 <= b + d < nblk:
                s2 = xs.clone()
                s2[:, b] = xs[:, b + d]
                out[f"xs: block {b} from {b + d}"] = (xq, s2, wq, ws)
                s2 = ws.clone()
                s2[:, b] = ws[:, b + d]
                out[f"ws: block {b} from {b + d}"] = (xq, xs, wq, s2)
    # ... from row m +- 1, from row n +- 1 (blockwise: from n-block +- 1)
    for m in sorted({0, M // 2, M - 1}):
        for d in (-1, 1):
            if 0 <= m + d < M:
                s2 = xs.clone()
                s2[m] = xs[m + d]
                out[f"xs: row {m} from {m + d}"] = (xq, s2, wq, ws)
    R = ws.shape[0]
    for n in sorted({0, R // 2, R - 1}):
        for d in (-1, 1):
            if 0 <= n + d < R:
                s2 = ws.clone()
                s2[n] = ws[n + d]
                out[f"ws: row {n} from {n + d}"] = (xq, xs, wq, s2)
    # the last block, or the last 16-B piece (16 one-byte codes; 32 e2m1 codes), dropped
    for what, cut in (("block", blk), ("16-B piece", 16)):
        x2 = xq.clone()
        x2[:, K - cut:] = 0
        out[f"x: last {what} dropped"] = (x2, xs, wq, ws)
        w2 = wc.clone()
        w2[:, K - (32 if fp4 else cut):] = 0
        out[f"w: last {what} dropped"] = (xq, xs, w_of(w2), ws)
        w2 = wc.clone()
        w2[N - 1, K - (32 if fp4 else cut):] = 0
        out[f"w: last {what} of the last row dropped"] = (xq, xs, w_of(w2), ws)
    # the two 16-k runs a lane holds of one matrix instruction exchanged: k 16 g .. + 16 and
    # 64 + 16 g .. + 16 of an aligned 128 (one operand only)
    for base in sorted({0, (K // 128 - 1) * 128}):
        for g in (0, 3):
            lo = torch.arange(base + 16 * g, base + 16 * g + 16)
            idx = torch.arange(K)
            idx[lo], idx[lo + 64] = lo + 64, lo
            out[f"x: halves of lane group {g} at k {base} exchanged"] = (xq[:, idx], xs, wq, ws)
            out[f"w: halves of lane group {g} at k {base} exchanged"] = (xq, xs, w_of(wc[:, idx]), ws)
    if fp4:
        out["w: the nibbles of every byte swapped"] = (xq, xs, (wq >> 4) | ((wq & 0xF) << 4), ws)
        w2 = wq.clone()
        w2[:, 0] = (wq[:, 0] >> 4) | ((wq[:, 0] & 0xF) << 4)
        out["w: the nibbles of one byte per row swapped"] = (xq, xs, w2, ws)
    return out


@FMT
def test_exact_comparison_flags_every_mutation(fmt):
    for M, N, K in E.FORCED_MNK[fmt]:
        xq, xs, wq, ws, bias = _make(fmt, M, N, K)
        good, good_b = E.REFS[fmt](xq, xs, wq, ws), E.REFS[fmt](xq, xs, wq, ws, bias)
        muts = _mutations(fmt, xq, xs, wq, ws)
        assert len(muts) >= 30
        for name, ops in muts.items():
            bad = E.REFS[fmt](*ops, None, check=False)
            assert bad.shape == good.shape and not bool(bad.isnan().any())
            # what the GPU tests assert: elementwise equality of the bf16 bits
            assert not torch.equal(bad, good), f"{fmt} {(M, N, K)} misses: {name}"
            bad_b = E.REFS[fmt](*ops, bias, check=False)
            assert not torch.equal(bad_b, good_b), f"{fmt} {(M, N, K)} with bias misses: {name}"
