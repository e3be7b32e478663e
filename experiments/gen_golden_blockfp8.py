"""Generate the blockwise float8 fixtures under tests/golden/ in plain torch on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python3 experiments/gen_golden_blockfp8.py

The arithmetic is the spec of csrc/block_fp8.hip written out block by block (not the package's
vectorised CPU functions, which tests/test_blockfp8_cpu.py checks against these files): per block
amax with NaN ignored, s = amax / 448 in fp32, code = e4m3fn(x / s) by torch's CPU cast
(round-to-nearest-even), the element itself where amax == 0. bf16 tensors are stored as their uint16
bit patterns.

  blockfp8_N128_K128.npz, blockfp8_N272_K384.npz, blockfp8_N384_K1024.npz
      w, bias, x   bf16 bits [N, K], [N], [5, K]; token ZERO_TOKEN is all zero, token
                   OUTLIER_TOKEN has one element of 200, block subnormal_block of token
                   SUBNORMAL_TOKEN holds bf16 subnormals
      wq, ws       uint8 [N, K] codes, float32 [ceil(N/128), K/128] scales
      xq, xs       uint8 [5, K] codes, float32 [5, K/128] scales
      y64          float64 [5, N]   sum_b P_b xs_b ws_b + bias in float64 on those codes
  blockfp8_quant_edges.npz
      x            bf16 bits [6, 256], two blocks per row: NaN in a block, +inf in a block, an
                   all-zero block with a -0, an all-subnormal block, amax exactly 448 and 448 * 2^k,
                   the largest bf16 exponents, a block of NaN and zeros only, -inf beside NaN,
                   subnormals beside a small normal
      q, s         uint8 [6, 256] codes, float32 [6, 2] scales
"""

import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
M = 5
ZERO_TOKEN = 2
OUTLIER_TOKEN = 3
SUBNORMAL_TOKEN = 4
E4 = torch.float8_e4m3fn
B = 128


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(v) -> torch.Tensor:
    return torch.tensor(np.asarray(v, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def quant_block(xb: torch.Tensor):
    """One block (any shape) of fp32 values -> (uint8 codes of that shape, fp32 scale)."""
    a = xb.abs().flatten()
    a = a[~a.isnan()]
    amax = a.max() if a.numel() else torch.tensor(0.0)
    s = (amax / torch.tensor(448.0, dtype=torch.float32)).to(torch.float32)
    v = xb if float(amax) == 0.0 else xb / s
    return v.to(E4).view(torch.uint8), s


def quant_act(x: torch.Tensor):
    xf = x.float()
    R, K = xf.shape
    q = torch.empty(R, K, dtype=torch.uint8)
    s = torch.empty(R, K // B, dtype=torch.float32)
    for r in range(R):
        for b in range(K // B):
            q[r, b * B:(b + 1) * B], s[r, b] = quant_block(xf[r, b * B:(b + 1) * B])
    return q, s


def quant_weight(w: torch.Tensor):
    wf = w.float()
    N, K = wf.shape
    NB = (N + B - 1) // B
    q = torch.empty(N, K, dtype=torch.uint8)
    s = torch.empty(NB, K // B, dtype=torch.float32)
    for i in range(NB):
        for b in range(K // B):
            q[i * B:(i + 1) * B, b * B:(b + 1) * B], s[i, b] = quant_block(
                wf[i * B:(i + 1) * B, b * B:(b + 1) * B])
    return q, s


def y64_of(xq, xs, wq, ws, bias):
    N, K = wq.shape
    xf, wf = xq.view(E4).double(), wq.view(E4).double()
    y = torch.zeros(xq.shape[0], N, dtype=torch.float64)
    for b in range(K // B):
        P = xf[:, b * B:(b + 1) * B] @ wf[:, b * B:(b + 1) * B].t()
        wsr = ws[:, b].double().repeat_interleave(B)[:N]
        y += P * xs[:, b].double()[:, None] * wsr[None, :]
    return y + bias.double()[None, :]


def edge_rows() -> torch.Tensor:
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(6, 256, generator=g) * 0.5).to(torch.bfloat16)
    x[0, 5] = float("nan")                          # a NaN in a block: the scale from the rest
    x[0, B + 9] = float("inf")                      # +inf: s = inf, zeros and one NaN code
    x[1, :B] = 0
    x[1, 17] = -0.0                                 # all zero, one of them negative
    x[1, B:] = from_bits(np.arange(1, B + 1))       # all bf16 subnormals: a subnormal scale
    x[2, :B] = x[2, :B].clamp(-400, 400)
    x[2, 3] = 448.0                                 # amax exactly 448: s = 1
    x[2, B:] = x[2, B:] * 1000
    x[2, B + 3] = -448.0 * 32                       # amax 448 * 2^5
    x[3, :B] = x[3, :B] * 2.0 ** -10
    x[3, 1] = 448.0 * 2.0 ** -10                    # amax 448 * 2^-10
    x[3, B:] = x[3, B:] * 1e38                      # exponent fields 253 / 254
    x[3, B] = 3.0e38
    x[4, :B] = 0
    x[4, 2] = float("nan")                          # NaN and zeros only: amax 0
    x[4, 3] = -0.0
    x[4, B + 4] = float("-inf")
    x[4, B + 5] = float("nan")
    x[5, :B] = from_bits(np.arange(1, B + 1) * 3 % 128)
    x[5, 7] = 2.0 ** -125                           # subnormals beside a small normal amax
    x[5, B:] = x[5, B:] * 2.0 ** -100
    return x


def main():
    os.makedirs(OUT, exist_ok=True)
    for idx, (N, K) in enumerate([(128, 128), (272, 384), (384, 1024)]):
        g = torch.Generator().manual_seed(500 + idx)
        w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
        x = torch.randn(M, K, generator=g).to(torch.bfloat16)
        bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
        sb = min(1, K // B - 1)
        x[ZERO_TOKEN] = 0
        x[OUTLIER_TOKEN, 7] = 200.0
        x[SUBNORMAL_TOKEN, B * sb:B * (sb + 1)] = from_bits(np.arange(1, B + 1))
        wq, ws = quant_weight(w)
        xq, xs = quant_act(x)
        assert int(xq[ZERO_TOKEN].max()) == 0 and float(xs[ZERO_TOKEN].abs().max()) == 0.0
        assert 0.0 < float(xs[SUBNORMAL_TOKEN, sb]) < 2.0 ** -126  # a subnormal scale
        y64 = y64_of(xq, xs, wq, ws, bias)
        assert bool(y64.isfinite().all())
        np.savez_compressed(
            os.path.join(OUT, f"blockfp8_N{N}_K{K}.npz"),
            N=N, K=K, zero_token=ZERO_TOKEN, outlier_token=OUTLIER_TOKEN,
            subnormal_token=SUBNORMAL_TOKEN, subnormal_block=sb,
            w=bf16_bits(w), x=bf16_bits(x), bias=bf16_bits(bias),
            wq=wq.numpy(), ws=ws.numpy(), xq=xq.numpy(), xs=xs.numpy(), y64=y64.numpy(),
        )
        wd = (wq.view(E4).double().reshape(N, K // B, B)
              * ws.double().repeat_interleave(B, 0)[:N][..., None]).reshape(N, K)
        print("blockfp8", N, K, "weight round trip, relative L2:",
              float((wd - w.double()).norm() / w.double().norm()))

    x = edge_rows()
    q, s = quant_act(x)
    np.savez_compressed(os.path.join(OUT, "blockfp8_quant_edges.npz"), x=bf16_bits(x),
                        q=q.numpy(), s=s.numpy())
    print("edges: scales\n", s.numpy())


if __name__ == "__main__":
    main()
