"""Generate the float8 dynamic-activation fixtures under tests/golden/ by running the REFERENCE
torchao.

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 tools/gen_golden_float8_dyn.py

It imports the reference's own ``quantize_``, ``Float8DynamicActivationFloat8WeightConfig(
granularity=PerRow(), version=1)`` and ``_input_activation_quant_func_fp8`` on the CPU and
records inputs and outputs as data; bf16 tensors are stored as their uint16 bit patterns. Nothing
of the reference's source is stored.

There is no reference OUTPUT to record: ``torch._scaled_mm`` on the CPU refuses row-wise scales
("Now _scaled_mm only supports per-tensor"), so calling the reference-quantized module raises
here. ``y64`` is the formula of include/torchao_mi355x.h (tao_fp8_scaled_mm_bf16) evaluated in
float64 on the reference's codes and scales.

  float8dq_N64_K256.npz, float8dq_N96_K1024.npz
      w, x, bias   bf16 bits [N, K], [5, K], [N]   (row ZERO_ROW of the first file's w and token
                                                    ZERO_TOKEN of its x are all zero)
      wq, ws       uint8 [N, K], float32 [N]       the reference's weight codes and scales
      xq, xs       uint8 [5, K], float32 [5]       its activation codes and scales
      y64          float64 [5, N]   ((f(xq) @ f(wq)^T) * xs[m]) * ws[n] + bias[n] in float64
                                    (NaN in the zero token's row and the zero row's column)
  float8dq_refckpt_v1_N32_K64.pt / .npz
      the state_dict of a reference-quantized nn.Linear as torch.save wrote it, and the same
      content as numbers (wq, ws, bias bits).
"""

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
ZERO_ROW = 7
ZERO_TOKEN = 2
M = 5


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH"
    )
    import torchao.quantization.quant_api as ref_api
    from torchao.quantization import Float8DynamicActivationFloat8WeightConfig, PerRow, quantize_
    from torchao.quantization.quant_api import _input_activation_quant_func_fp8

    # the reference asserts a CUDA / MI300 device before it quantizes; the arithmetic recorded
    # here is device-independent torch ops
    ref_api.is_sm_at_least_89 = lambda: True
    ref_api._check_hardware_support = lambda granularity: None

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle  # only for the deterministic input generators

    def quantized_linear(w, bias):
        N, K = w.shape
        lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(bias)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            quantize_(lin, Float8DynamicActivationFloat8WeightConfig(granularity=PerRow(),
                                                                     version=1))
        return lin

    os.makedirs(OUT, exist_ok=True)
    for idx, (N, K, zeros) in enumerate([(64, 256, True), (96, 1024, False)]):
        w = oracle.make_linear_weight(N, K, seed=80 + idx)
        x = oracle.make_activation(M, K, seed=90 + idx)
        if zeros:
            w[ZERO_ROW] = 0
            x[ZERO_TOKEN] = 0
        gen = torch.Generator().manual_seed(100 + idx)
        bias = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)
        lin = quantized_linear(w, bias)
        lw = lin.weight
        wimpl = lw.original_weight_tensor.tensor_impl
        assert lw.input_quant_func is _input_activation_quant_func_fp8
        qx = lw.input_quant_func(x, **lw.quant_kwargs)
        ximpl = qx.tensor_impl
        wq, ws = wimpl.float8_data, wimpl.scale.reshape(-1)
        xq, xs = ximpl.float8_data, ximpl.scale.reshape(-1)
        assert ws.dtype == torch.float32 and xs.dtype == torch.float32
        try:
            with torch.no_grad():
                lin(x)
            raise SystemExit("the reference module ran on the CPU: record its output too")
        except (RuntimeError, NotImplementedError) as e:
            print("reference output not available on the CPU:", str(e).splitlines()[0][:100])
        y64 = (xq.double() @ wq.double().t()) * xs.double()[:, None] * ws.double()[None, :]
        y64 = y64 + bias.double()[None, :]
        if zeros:
            assert float(ws[ZERO_ROW]) == 0.0 and bool(wq[ZERO_ROW].isnan().all())
            assert float(xs[ZERO_TOKEN]) == 0.0 and bool(xq[ZERO_TOKEN].isnan().all())
            nan = y64.isnan()
            assert bool(nan[ZERO_TOKEN].all()) and bool(nan[:, ZERO_ROW].all())
            assert int(nan.sum()) == N + M - 1
        rec = dict(
            N=N, K=K, zero_row=ZERO_ROW if zeros else -1, zero_token=ZERO_TOKEN if zeros else -1,
            w=bf16_bits(w), x=bf16_bits(x), bias=bf16_bits(bias),
            wq=wq.view(torch.uint8).numpy(), ws=ws.numpy(),
            xq=xq.view(torch.uint8).numpy(), xs=xs.numpy(), y64=y64.numpy(),
        )
        np.savez_compressed(os.path.join(OUT, f"float8dq_N{N}_K{K}.npz"), **rec)
        print("float8dq", N, K, "zero row and token" if zeros else "")

    N, K = 32, 64
    w = oracle.make_linear_weight(N, K, seed=110)
    gen = torch.Generator().manual_seed(111)
    bias = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)
    lin = quantized_linear(w, bias)
    print(lin)
    torch.save(lin.state_dict(), os.path.join(OUT, f"float8dq_refckpt_v1_N{N}_K{K}.pt"))
    impl = lin.weight.original_weight_tensor.tensor_impl
    np.savez_compressed(
        os.path.join(OUT, f"float8dq_refckpt_v1_N{N}_K{K}.npz"),
        N=N, K=K, wq=impl.float8_data.view(torch.uint8).numpy(),
        ws=impl.scale.reshape(-1).numpy(), bias=bf16_bits(bias), repr=np.array(repr(lin)),
    )
    print("float8dq reference checkpoint", N, K)


if __name__ == "__main__":
    main()
