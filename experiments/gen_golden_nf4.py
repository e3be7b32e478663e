"""Generate the NF4 fixtures under tests/golden/ by running the REFERENCE torchao on the CPU.

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_nf4.py

It imports the reference's own ``to_nf4``, ``linear_nf4``, ``quantize_`` and ``nf4_weight_only``
and records inputs and outputs as data; bf16 tensors are stored as their uint16 bit patterns.
Nothing of the reference's source is stored.

  nf4_N{N}_K{K}.npz   N48 K1024, N64 K256, N256 K64, N40 K2048, N32 K1536, N512 K96 (blocks
                      straddle rows: no linear on the HIP route)
      w, x, bias            bf16 bits [N, K], [5, K], [N]
      quantized_data        uint8 [N K / 2]
      quantized_scalers     int8 [N K / 64]
      quantization_factor   bf16 bits [N K / 16384]
      scaler_mean           bf16 bits []
      nf4                   bf16 bits [16]
      w_hat                 bf16 bits [N, K]      get_original_weight()
      y_ref                 bf16 bits [5, N]      the reference's CPU linear_nf4(x, W) + bias
      y64                   float64 [5, N]        x @ w_hat^T + bias in float64
  nf4_quant_edges.npz   two flat tensors of 16384 weights (256 blocks), `fin_*` and `inf_*`, each
                      with w and the five stored tensors as above. Blocks of `fin`: 0 all zero,
                      1 absmax element negative, 2 all values equal, 3 absmax 1.0 with bf16(mid) and
                      its two bf16 neighbours for every midpoint of adjacent levels; the rest
                      random. `inf` is `fin` with an inf in block 5 (its absmax, the mean of the
                      absmaxes and with it every scaler stop being finite, so it is a tensor of
                      its own).
  nf4_refckpt_N32_K512.pt / .npz
      the state_dict of a reference nn.Linear(512, 32) after quantize_(m, nf4_weight_only()) as
      torch.save wrote it, and the same content as numbers (the five tensors, bias, w_hat).

Asserted here and restated by the tests: in every tensor but `inf` the fp32 and float64 means of
the block absmaxes round to the same bf16 (the stored scaler_mean) and lie at least 2^-20
(relative) from a bf16 rounding boundary, so the order of the mean's fp32 sum cannot change a
byte. Seeds are advanced until this holds.
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
SHAPES = ((48, 1024), (64, 256), (256, 64), (40, 2048), (32, 1536), (512, 96))
M = 5
INNER = ("quantized_data", "quantized_scalers", "quantization_factor", "scaler_mean", "nf4")


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def stored(t, prefix=""):
    out = {}
    for name in INNER:
        v = getattr(t, name)
        out[prefix + name] = bits(v) if v.dtype is torch.bfloat16 else v.numpy()
    return out


def mean_is_pinned(w: torch.Tensor) -> bool:
    """The condition of the module docstring on the block absmaxes of a flat bf16 tensor."""
    a = w.flatten().view(-1, 64).abs().max(dim=1).values
    m64 = a.double().mean().item()
    m32 = a.float().mean().item()
    r = torch.tensor(m64, dtype=torch.float64).to(torch.bfloat16)
    if torch.tensor(m32).to(torch.bfloat16) != r or a.mean() != r:
        return False
    rb = r.view(torch.int16).item()
    for nb in (rb - 1, rb + 1):  # the two rounding boundaries around r
        other = torch.tensor(nb, dtype=torch.int16).view(torch.bfloat16).double().item()
        boundary = (r.double().item() + other) / 2
        if abs(m64 - boundary) < abs(m64) * 2.0 ** -20:
            return False
    return True


def pinned_weight(make, seed):
    while True:
        w = make(seed)
        if mean_is_pinned(w):
            return w, seed
        seed += 1


def edge_tensor(seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(256, 64, generator=g) * 0.05).to(torch.bfloat16)
    w[0] = 0
    w[1] = (torch.rand(64, generator=g) * 0.5).to(torch.bfloat16)
    w[1, 17] = -0.75
    w[2] = 0.3125
    levels = torch.tensor([-1.0, -0.6962, -0.5251, -0.3949, -0.2844, -0.1848, -0.0911, 0.0,
                           0.0796, 0.1609, 0.2461, 0.3379, 0.4407, 0.5626, 0.7230, 1.0]
                          ).to(torch.bfloat16)
    mids = ((levels[:-1].float() + levels[1:].float()) / 2).to(torch.bfloat16)
    mb = mids.view(torch.int16)
    trio = torch.stack([mb - 1, mb, mb + 1], -1).flatten().view(torch.bfloat16)
    w[3] = 0.001
    w[3, 0] = 1.0
    w[3, 1:1 + trio.numel()] = trio
    return w.flatten()


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH")
    from torchao.dtypes.nf4tensor import linear_nf4, to_nf4
    from torchao.quantization import quantize_

    try:
        from torchao.dtypes._nf4tensor_api import nf4_weight_only
    except ImportError:
        from torchao.quantization.quant_api import nf4_weight_only

    os.makedirs(OUT, exist_ok=True)
    for i, (N, K) in enumerate(SHAPES):
        def make(seed):
            g = torch.Generator().manual_seed(seed)
            # rows of unequal size, so block absmaxes (and their int8 scalers) spread
            row = 0.02 + 0.1 * torch.rand(N, 1, generator=g)
            return (torch.randn(N, K, generator=g) * row).to(torch.bfloat16)

        w, seed = pinned_weight(make, 1000 * (i + 1))
        g = torch.Generator().manual_seed(seed + 500)
        x = torch.randn(M, K, generator=g).to(torch.bfloat16)
        bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
        t = to_nf4(w)
        w_hat = t.get_original_weight()
        assert w_hat.dtype is torch.bfloat16 and w_hat.shape == w.shape
        y_ref = linear_nf4(x, t) + bias
        y64 = x.double() @ w_hat.double().t() + bias.double()
        np.savez(os.path.join(OUT, f"nf4_N{N}_K{K}.npz"), w=bits(w), x=bits(x), bias=bits(bias),
                 w_hat=bits(w_hat), y_ref=bits(y_ref), y64=y64.numpy(), seed=np.int64(seed),
                 **stored(t))
        print(f"nf4_N{N}_K{K}: seed {seed}, mean {t.scaler_mean.item()}")

    fin, seed = pinned_weight(edge_tensor, 7000)
    inf = fin.clone()
    inf[5 * 64 + 9] = float("inf")
    tf, ti = to_nf4(fin), to_nf4(inf)
    np.savez(os.path.join(OUT, "nf4_quant_edges.npz"), fin_w=bits(fin), inf_w=bits(inf),
             seed=np.int64(seed), **stored(tf, "fin_"), **stored(ti, "inf_"))
    print(f"nf4_quant_edges: seed {seed}")

    N, K = 32, 512

    def make_lin(seed):
        torch.manual_seed(seed)
        return torch.nn.Linear(K, N, dtype=torch.bfloat16).weight.detach().clone()

    w, seed = pinned_weight(make_lin, 9000)
    torch.manual_seed(seed)
    m = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    assert torch.equal(m.weight.detach(), w)
    quantize_(m, nf4_weight_only())
    sd = m.state_dict()
    torch.save(sd, os.path.join(OUT, f"nf4_refckpt_N{N}_K{K}.pt"))
    back = torch.load(os.path.join(OUT, f"nf4_refckpt_N{N}_K{K}.pt"), weights_only=True)
    assert torch.equal(back["weight"].quantized_data, sd["weight"].quantized_data)
    np.savez(os.path.join(OUT, f"nf4_refckpt_N{N}_K{K}.npz"), w=bits(w), bias=bits(sd["bias"]),
             w_hat=bits(sd["weight"].get_original_weight()), seed=np.int64(seed),
             **stored(sd["weight"]))
    print(f"nf4_refckpt_N{N}_K{K}: seed {seed}")


if __name__ == "__main__":
    sys.exit(main())
