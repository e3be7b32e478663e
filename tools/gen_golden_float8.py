"""Generate the float8 weight-only fixtures under tests/golden/ by running the REFERENCE torchao.

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 tools/gen_golden_float8.py

It imports the reference's own float8 primitives, ``quantize_`` and
``Float8WeightOnlyConfig(version=1)`` on the CPU and records inputs and outputs as data; bf16
tensors are stored as their uint16 bit patterns. Nothing of the reference's source is stored.

  float8wo_N64_K256.npz, float8wo_N96_K1024.npz
      w          bf16 bits [N, K]  the weight (row ZERO_ROW of the first file is all zero)
      q          uint8 [N, K]      the reference's e4m3fn codes (_quantize_affine_float8)
      s          float32 [N]       its scales (_choose_scale_float8; 0.0 for the zero row)
      w_dequant  bf16 bits [N, K]  AffineQuantizedTensor.dequantize() of the quantized module
      x, bias    bf16 bits [5, K], [N]
      y_ref      bf16 bits [5, N]  the quantized reference module's CPU output (with bias)
      y64        float64 [5, N]    x @ (f(q) * s)^T in float64, no bias (NaN in a zero row's column)
  float8wo_refckpt_v1_N32_K64.pt / .npz
      the state_dict of a reference-quantized nn.Linear as torch.save wrote it, and the same
      content as numbers (q, s, bias bits, w_dequant bits).
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
ZERO_ROW = 7
M = 5


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH"
    )
    from torchao.quantization import Float8WeightOnlyConfig, quantize_
    from torchao.quantization.quant_primitives import (
        _choose_scale_float8,
        _dequantize_affine_float8,
        _quantize_affine_float8,
    )

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle  # only for the deterministic input generators

    def quantized_linear(w, bias):
        N, K = w.shape
        lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(bias)
        quantize_(lin, Float8WeightOnlyConfig(version=1))
        return lin

    os.makedirs(OUT, exist_ok=True)
    for idx, (N, K, zero_row) in enumerate([(64, 256, True), (96, 1024, False)]):
        w = oracle.make_linear_weight(N, K, seed=40 + idx)
        if zero_row:
            w[ZERO_ROW] = 0
        x = oracle.make_activation(M, K, seed=50 + idx)
        gen = torch.Generator().manual_seed(60 + idx)
        bias = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)

        s = _choose_scale_float8(w, block_size=(1, K), float8_dtype=torch.float8_e4m3fn)
        q = _quantize_affine_float8(w, s, torch.float8_e4m3fn)
        assert s.dtype == torch.float32 and tuple(s.shape) == (N, 1)
        lin = quantized_linear(w, bias)
        impl = lin.weight.tensor_impl
        assert torch.equal(impl.float8_data.view(torch.uint8), q.view(torch.uint8))
        assert torch.equal(impl.scale, s)
        dq = lin.weight.dequantize()
        assert dq.dtype == torch.bfloat16
        same = (dq == _dequantize_affine_float8(q, s, torch.bfloat16)) | dq.isnan()
        assert bool(same.all())
        with torch.no_grad():
            y_ref = lin(x)
        y64 = x.double() @ (q.double() * s.double()).t()
        if zero_row:
            assert float(s[ZERO_ROW]) == 0.0 and bool(q[ZERO_ROW].isnan().all())
            assert bool(y_ref[:, ZERO_ROW].isnan().all()) and bool(y64[:, ZERO_ROW].isnan().all())
        rec = dict(
            N=N, K=K, zero_row=ZERO_ROW if zero_row else -1,
            w=bf16_bits(w), q=q.view(torch.uint8).numpy(), s=s.reshape(-1).numpy(),
            w_dequant=bf16_bits(dq), x=bf16_bits(x), bias=bf16_bits(bias),
            y_ref=bf16_bits(y_ref), y64=y64.numpy(),
        )
        np.savez_compressed(os.path.join(OUT, f"float8wo_N{N}_K{K}.npz"), **rec)
        print("float8wo", N, K, "zero row" if zero_row else "")

    N, K = 32, 64
    w = oracle.make_linear_weight(N, K, seed=70)
    gen = torch.Generator().manual_seed(71)
    bias = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)
    lin = quantized_linear(w, bias)
    torch.save(lin.state_dict(), os.path.join(OUT, f"float8wo_refckpt_v1_N{N}_K{K}.pt"))
    impl = lin.weight.tensor_impl
    np.savez_compressed(
        os.path.join(OUT, f"float8wo_refckpt_v1_N{N}_K{K}.npz"),
        N=N, K=K, q=impl.float8_data.view(torch.uint8).numpy(),
        s=impl.scale.reshape(-1).numpy(), bias=bf16_bits(bias),
        w_dequant=bf16_bits(lin.weight.dequantize()),
    )
    print("float8wo reference checkpoint", N, K)


if __name__ == "__main__":
    main()
