"""Inputs on which the float8 x float8 linear (fp8_scaled_mm, fp8_dyn_linear) can be checked BIT
FOR BIT.

The construction of tests/exact_inputs_fp8.py with x drawn from e4m3fn values too: the weight
codes, their scales, the bias and the x VALUES (integers in [-4, 4] for "dense", +-1 at 8 probed
positions for "probe") are that file's; here x is handed over as e4m3fn codes with a per-token
fp32 scale (arbitrary positive for "dense", a power of two for "probe"). Every product
f(xq) * f(wq) and every partial sum is an exact fp32 number, so the order of accumulation (GEMV
lanes, MFMA k blocks, k-groups, split-K slabs) cannot matter, and what is left is the epilogue of
include/torchao_mi355x.h (tao_fp8_scaled_mm_bf16):

    y = bf16( fp32(fp32(acc * xs[m]) * ws[n]) + fp32(bias[n]) )       one rounding to bf16

The reference below is that formula on the float64 sum and calls no code under test.

The matrix instruction's own exact range. v_mfma_scale_f32_16x16x128_f8f6f4 does not add its 128
products in fp32 one by one, so "every partial sum is an fp32 number" is not enough for it. A probe
on the MI355X (one MFMA, +2^16 - 2^16 + 2^e placed at chosen k, each sum exactly representable;
experiments/probe_mfma_f8_exact.py) found:
  * inside an aligned group of 8 consecutive k, a product 2^13 times smaller than the group's
    largest is kept and one 2^14 times smaller is dropped (the result was 0 instead of 2^e);
  * between different groups of 8 of one instruction the first loss was at a ratio of 2^24 - 2^25;
  * between the two MFMAs of a step and between steps (the fp32 accumulator) nothing was lost up
    to the largest ratio two e4m3fn products allow in the probe, 2^32.
So the makers also assert that in every weight row all products are multiples of a unit with
max |product| < 2^12 units, two bits inside the narrowest window found. Both families of
exact_inputs_fp8.py already satisfy it ("dense": at most 4 * 15.5 / 2^-5 = 1984 units; "probe":
at most 30), so neither had to be narrowed.
"""

import torch

import exact_inputs_fp8 as E8
from exact_inputs_fp8 import (  # noqa: F401  (re-exported for the tests)
    BF16,
    FAMILIES,
    FP8,
    decode,
    describe_mismatch,
    same_codes,
)

MFMA_WINDOW_BITS = 12  # max |product| / unit < 2^12 inside one MFMA (see above: 13 measured)


def _lowbit_unit(v):
    """The largest power of two dividing every nonzero entry of v (all multiples of 2^-18)."""
    i = (v.double() * 2.0 ** 18).round().long().abs()
    i = i[i != 0]
    low = (i & -i).min() if i.numel() else torch.tensor(1 << 18)
    return float(low) / 2.0 ** 18


def check_mfma_window(xv, wv):
    """Every row's products stay inside the matrix instruction's exact window."""
    ux = _lowbit_unit(xv)
    xmax = float(xv.abs().max())
    for n in range(wv.shape[0]):
        unit = ux * _lowbit_unit(wv[n])
        assert xmax * float(wv[n].abs().max()) < 2 ** MFMA_WINDOW_BITS * unit, (
            f"row {n}: products span more than {MFMA_WINDOW_BITS} bits")


def make_fp8dyn_exact(M, N, K, seed, family="dense"):
    """xq uint8 [M, K], xs fp32 [M], wq uint8 [N, K], ws fp32 [N], bias bf16 [N]; asserts the
    conditions above."""
    wq, ws, bias, x = E8.make_fp8wo_exact(M, N, K, seed, family)
    xq = x.to(FP8)
    assert torch.equal(xq.double(), x.double()), "x is not made of e4m3fn values"
    gen = torch.Generator().manual_seed(977 * seed + 3 + FAMILIES.index(family))
    if family == "dense":
        xs = (torch.rand(M, generator=gen) * 0.5 + 0.01).float()
    else:
        xs = torch.pow(2.0, ((torch.arange(M) * 5 + seed) % 9 - 4).double()).float()
    xv, wv = x.double(), decode(wq)
    check_mfma_window(xv, wv)
    # every partial sum, in any order, is an fp32 number: all terms are multiples of one unit per
    # row and the sum of magnitudes stays below 2^24 units
    ux = _lowbit_unit(xv)
    mags = xv.abs() @ wv.abs().t()
    for n in range(N):
        assert float(mags[:, n].max()) < 2 ** 24 * ux * _lowbit_unit(wv[n])
    return xq.view(torch.uint8).contiguous(), xs.contiguous(), wq, ws, bias


def exact_acc(xq, wq):
    """f(xq) @ f(wq)^T exactly, float64 [M, N]."""
    return decode(xq) @ decode(wq).t()


def ref_fp8dyn(xq, xs, wq, ws, bias=None):
    """tao_fp8_scaled_mm_bf16 on exact inputs: the exact sum, then the fp32 epilogue
    (acc * xs) * ws (+ bias), each step rounded to fp32, and one rounding to bf16."""
    acc = exact_acc(xq, wq)
    acc32 = acc.float()
    same = (acc32.double() == acc) | acc.isnan()
    assert bool(same.all()), "reference sum is not an fp32 number"
    y = (acc32 * xs.float().view(-1, 1)) * ws.float().view(1, -1)
    if bias is not None:
        y = y + bias.float().view(1, -1)
    return y.to(BF16)


def make_identity_token(N, K, seed):
    """A bf16 token on which the per-row quantisation is the identity on chosen codes: small
    integers, one entry +-448, all times 2^p. Then amax = 448 * 2^p, the scale is exactly 2^p and
    every x / scale is an e4m3fn value. Returns x bf16 [1, K], the codes it must quantise to, the
    scale, and weight codes / scales / bias of the "dense" family."""
    wq, ws, bias, x = E8.make_fp8wo_exact(1, N, K, seed, "dense")
    gen = torch.Generator().manual_seed(seed + 41)
    v = x.double().clone()
    k448 = int(torch.randint(0, K, (1,), generator=gen))
    v[0, k448] = 448.0 if seed % 2 else -448.0
    p = seed % 7 - 3
    xb = (v * 2.0 ** p).to(BF16)
    assert torch.equal(xb.double(), v * 2.0 ** p)
    codes = v.to(FP8)
    assert torch.equal(codes.double(), v)
    wv = decode(wq)
    unit = _lowbit_unit(wv)
    assert float((v.abs() @ wv.abs().t()).max()) < 2 ** 24 * unit
    return xb, codes.view(torch.uint8), torch.tensor([2.0 ** p]), wq, ws, bias


# ---- the shapes of tests/test_gpu_exact_fp8dyn.py ----------------------------------------------
MFMA_M = (1, 5, 16, 17, 33, 128)
MFMA_N = (16, 37, 80)
# a step shorter than one MFMA (16, 112), exactly one (128), one step (256), a tail inside the
# second MFMA of a step (384 = 256 + 128 fills the first; 272 = 256 + 16), 16 past full steps (1040)
MFMA_K = (16, 112, 128, 256, 272, 384, 1040)
# (M tile, k-groups, K slices): k-groups 1 / 2, split-K 1 / 2 / 3 (more slices than steps at small K)
FORCED_TILES = [(16, 1, 1), (16, 2, 1), (16, 1, 2), (32, 2, 3), (64, 1, 3), (128, 1, 2), (64, 2, 2)]
FORCED_MNK = [(33, 37, 272), (70, 80, 1040), (17, 16, 384), (5, 37, 128)]
GEMV_M = (1, 2, 3, 4, 5, 8)
GEMV_N = (1, 37)
GEMV_K = (16, 1024, 1040, 4112)
GEMV_FORCED = [(2, 1, 1), (4, 2, 4), (8, 8, 1), (4, 0, 8), (2, 3, 2)]  # (4, 0, 8): the clamp case
