"""Generate the uintx fixtures under tests/golden/ by running the REFERENCE torchao on the CPU.

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_uintx.py

It imports the reference's own ``quantize_`` and ``uintx_weight_only`` and records inputs and
outputs as data; bf16 tensors are stored as their uint16 bit patterns. Nothing of the reference's
source is stored.

  uintx_b{bits}_N{N}_K{K}_g{g}.npz   bits 2, 3, 6, 7 at N 32 x K 384, g 64 (K / 8 = 48: segment
                                     boundaries fall inside groups); bits 1, 4, 5 at N 16 x K 128,
                                     g 32
      w, x, bias            bf16 bits [N, K], [5, K], [N]
      int4_shard / int2_shard / int1_shard   uint8, the reference's shards (those the width has)
      codes                 uint8 [N, K]           its get_plain()[0]
      scale                 bf16 bits [N, K / g]
      zero_point            int32 [N, K / g]
      w_hat                 bf16 bits [N, K]       its dequantize()
      y_ref                 bf16 bits [5, N]       its nn.Linear forward on the CPU, with bias
      y64                   float64 [5, N]         sum x (q - zp) s in float64, products unrounded,
                                                   no bias
  uintx_refckpt_b3_N32_K128_g64.pt / .npz
      the state_dict of a reference nn.Linear(128, 32) after
      quantize_(m, uintx_weight_only(torch.uint3, group_size=64)) as torch.save wrote it, and its
      w_hat bits.

Asserted and printed here, so that a failing test cannot be the fixture's fault: the reference's
own rel_l2 against y64 without bias (two bf16 roundings: the weight's and the output's; bound
2 * 2^-9), and that every code fits its width.
"""

import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
CASES = [(b, 32, 384, 64) for b in (2, 3, 6, 7)] + [(b, 16, 128, 32) for b in (1, 4, 5)]
M = 5


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def quantized_linear(bits, N, K, g, seed):
    from torchao.quantization import quantize_, uintx_weight_only

    gen = torch.Generator().manual_seed(seed)
    m = torch.nn.Linear(K, N, bias=True)
    with torch.no_grad():
        m.weight.copy_(torch.randn(N, K, generator=gen) * 0.05)
        m.bias.copy_(torch.randn(N, generator=gen) * 0.1)
    m = m.to(torch.bfloat16)
    w = m.weight.detach().clone()
    quantize_(m, uintx_weight_only(getattr(torch, f"uint{bits}"), group_size=g))
    return m, w, gen


def main():
    os.makedirs(OUT, exist_ok=True)
    for bits, N, K, g in CASES:
        m, w, gen = quantized_linear(bits, N, K, g, 1000 + bits)
        x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
        impl = m.weight.tensor_impl
        codes, scale, zp = impl.get_plain()
        assert codes.dtype == torch.uint8 and int(codes.max()) < 2**bits
        assert zp.dtype == torch.int32 and scale.dtype == torch.bfloat16
        data = impl.int_data
        rec = {name: getattr(data, name).numpy() for name in type(data).bits_to_shard[bits]}
        w_hat = m.weight.dequantize()
        with torch.no_grad():
            y_ref = m(x)
            y_nobias = torch.nn.functional.linear(x, w_hat)
        s_full = scale.double().repeat_interleave(g, dim=1)
        zp_full = zp.double().repeat_interleave(g, dim=1)
        y64 = x.double() @ ((codes.double() - zp_full) * s_full).t()
        err = rel_l2(y_nobias, y64)
        print(f"uint{bits} N{N} K{K} g{g}: reference rel_l2 vs y64 = {err:.3e}")
        assert err <= 2 * 2.0**-9, err
        rec.update(w=bits_of(w), x=bits_of(x), bias=bits_of(m.bias), codes=codes.numpy(),
                   scale=bits_of(scale), zero_point=zp.numpy(), w_hat=bits_of(w_hat),
                   y_ref=bits_of(y_ref), y64=y64.numpy())
        np.savez_compressed(os.path.join(OUT, f"uintx_b{bits}_N{N}_K{K}_g{g}.npz"), **rec)

    m, w, _ = quantized_linear(3, 32, 128, 64, 77)
    stem = os.path.join(OUT, "uintx_refckpt_b3_N32_K128_g64")
    torch.save(m.state_dict(), stem + ".pt")
    np.savez_compressed(stem + ".npz", w=bits_of(w), bias=bits_of(m.bias),
                        w_hat=bits_of(m.weight.dequantize()))


if __name__ == "__main__":
    main()
