"""Generate the MXFP8 fixtures under tests/golden/ by running the REFERENCE torchao on the CPU.

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_mx.py

It calls the reference's own ``MXTensor.to_mx`` (FLOOR, float8_e4m3fn, block 32), its ``to_dtype``,
its emulated ``F.linear`` on MXTensors and its ``quantize_(…, MXFPInferenceConfig())`` and records
inputs and outputs as data; bf16 tensors are stored as their uint16 bit patterns. Nothing of the
reference's source is stored.

  mxfp8_N64_K256.npz, mxfp8_N96_K1024.npz, mxfp8_N40_K352.npz
      w, bias, x   bf16 bits [N, K], [N], [5, K]; token ZERO_TOKEN is all zero, token
                   OUTLIER_TOKEN has one element of 200, block SUBNORMAL_BLOCK of token
                   SUBNORMAL_TOKEN holds bf16 subnormals
      wq, ws       uint8 [N, K], [N, K/32]   the reference's weight codes and E8M0 bytes
      xq, xs       uint8 [5, K], [5, K/32]   its activation codes and bytes
      w_deq        bf16 bits [N, K]          its MXTensor.to_dtype(bfloat16) of the weight (the
                                             two smaller files only, to bound the largest)
      y64          float64 [5, N]   sum_b 2^(xs-127) 2^(ws-127) sum_k f(xq) f(wq) + bias in float64
      y_ref        bf16 bits [5, N] the reference's emulated F.linear(x, MXTensor w, bias)
  mx_quant_edges.npz
      x            bf16 bits [R, 64]: blocks with NaN, +inf, all zero, all subnormal, an amax that
                   is a power of two and the bf16 number just below it, amaxes that round up to /
                   saturate at 448, the largest and smallest normal exponents
      q, s, deq    the reference's codes, E8M0 bytes and to_dtype(bfloat16) bits
  mxfp8_refckpt_N32_K64.pt / .npz
      the state_dict of a reference-quantized nn.Linear as torch.save wrote it, and the same
      content as numbers (wq, ws, bias bits).
"""

import os
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
M = 5
ZERO_TOKEN = 2
OUTLIER_TOKEN = 3
SUBNORMAL_TOKEN = 4
SUBNORMAL_BLOCK = 1
E4 = torch.float8_e4m3fn


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(v) -> torch.Tensor:
    return torch.tensor(np.asarray(v, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def edge_rows() -> torch.Tensor:
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(6, 64, generator=g) * 0.5).to(torch.bfloat16)
    x[0, 5] = float("nan")                      # a NaN block
    x[0, 32 + 9] = float("inf")                 # a +inf block
    x[1, :32] = 0                               # all zero
    x[1, 32:] = from_bits(np.arange(1, 33) * 3)  # all bf16 subnormals
    x[2, :32] = x[2, :32].clamp(-4, 4)
    x[2, 3] = 8.0                               # amax exactly a power of two
    x[2, 32:] = x[2, 32:].clamp(-4, 4)
    x[2, 32 + 3] = -7.96875                     # the bf16 number just below it
    x[3, :32] = x[3, :32] * 100
    x[3, 1] = 440.0                             # 440 / 2^0 rounds up to 448
    x[3, 32:] = x[3, 32:] * 100
    x[3, 32 + 1] = -480.0                       # saturates at -448
    x[3, 32 + 2] = 464.0                        # a tie above 448: clamped
    x[4, :32] = x[4, :32] * 1e38                # exponent field 253 / 254
    x[4, 0] = 3.0e38
    x[4, 32:] = x[4, 32:] * 2.0 ** -120         # small normals: scale byte near 0
    x[5, :32] = from_bits(np.arange(1, 33) * 3)
    x[5, 7] = 2.0 ** -125                       # subnormals beside a small normal amax
    x[5, 32 + 4] = float("-inf")
    x[5, 32 + 5] = float("nan")                 # NaN wins over inf
    return x


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH"
    )
    import torchao.prototype.mx_formats.inference_workflow as ref_wf
    from torchao.prototype.mx_formats.config import MXGemmKernelChoice
    from torchao.prototype.mx_formats.mx_tensor import MXTensor, QuantizeTensorToMXKwargs
    from torchao.quantization import quantize_

    # the reference asserts an sm100 device before it quantizes; the arithmetic recorded here is
    # device-independent torch ops
    ref_wf.is_sm_at_least_100 = lambda: True

    def quantize(t):
        mx = MXTensor.to_mx(t.contiguous(), E4, 32)
        return mx, mx.qdata.view(torch.uint8), mx._scale_e8m0.view(torch.uint8).reshape(
            *t.shape[:-1], t.shape[-1] // 32)

    os.makedirs(OUT, exist_ok=True)
    for idx, (N, K) in enumerate([(64, 256), (96, 1024), (40, 352)]):
        g = torch.Generator().manual_seed(300 + idx)
        w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
        x = torch.randn(M, K, generator=g).to(torch.bfloat16)
        bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
        x[ZERO_TOKEN] = 0
        x[OUTLIER_TOKEN, 7] = 200.0
        x[SUBNORMAL_TOKEN, 32 * SUBNORMAL_BLOCK:32 * (SUBNORMAL_BLOCK + 1)] = from_bits(
            np.arange(1, 33) * 2)
        wmx, wq, ws = quantize(w)
        xmx, xq, xs = quantize(x)
        assert int(xs[ZERO_TOKEN].max()) == 0 and int(xq[ZERO_TOKEN].max()) == 0
        assert int(xs[SUBNORMAL_TOKEN, SUBNORMAL_BLOCK]) == 0

        def deq64(q, s):
            f = q.view(E4).double().reshape(q.shape[0], -1, 32)
            return (f * torch.exp2(s.double() - 127)[..., None]).reshape(q.shape[0], -1)

        y64 = deq64(xq, xs) @ deq64(wq, ws).t() + bias.double()[None, :]
        assert bool(y64.isfinite().all())
        # the reference's emulated linear: the activation is quantised by act_quant_kwargs
        kw = QuantizeTensorToMXKwargs(elem_dtype=E4, block_size=32,
                                      gemm_kernel_choice=MXGemmKernelChoice.EMULATED)
        wlin = MXTensor.to_mx(w, E4, 32, gemm_kernel_choice=MXGemmKernelChoice.EMULATED,
                              act_quant_kwargs=kw)
        with torch.no_grad():
            y_ref = torch.nn.functional.linear(x, wlin, bias)
        assert y_ref.dtype == torch.bfloat16 and y_ref.shape == (M, N)
        extra = {"w_deq": bf16_bits(wmx.to_dtype(torch.bfloat16))} if N * K <= 16384 else {}
        np.savez_compressed(
            os.path.join(OUT, f"mxfp8_N{N}_K{K}.npz"),
            N=N, K=K, zero_token=ZERO_TOKEN, outlier_token=OUTLIER_TOKEN,
            subnormal_token=SUBNORMAL_TOKEN, subnormal_block=SUBNORMAL_BLOCK,
            w=bf16_bits(w), x=bf16_bits(x), bias=bf16_bits(bias),
            wq=wq.numpy(), ws=ws.numpy(), xq=xq.numpy(), xs=xs.numpy(),
            y64=y64.numpy(), y_ref=bf16_bits(y_ref), **extra,
        )
        err = float((y_ref.double() - y64).norm() / y64.norm())
        print("mxfp8", N, K, "reference emulated output vs y64, relative L2:", err)

    x = edge_rows()
    mx, q, s = quantize(x)
    np.savez_compressed(os.path.join(OUT, "mx_quant_edges.npz"), x=bf16_bits(x), q=q.numpy(),
                        s=s.numpy(), deq=bf16_bits(mx.to_dtype(torch.bfloat16)))
    print("edges: scale bytes\n", s.numpy())

    N, K = 32, 64
    g = torch.Generator().manual_seed(310)
    lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_((torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16))
        lin.bias.copy_((torch.randn(N, generator=g) * 0.1).to(torch.bfloat16))
    bias = lin.bias.detach().clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        quantize_(lin, ref_wf.MXFPInferenceConfig())
    print(lin)
    torch.save(lin.state_dict(), os.path.join(OUT, f"mxfp8_refckpt_N{N}_K{K}.pt"))
    wt = lin.weight
    np.savez_compressed(
        os.path.join(OUT, f"mxfp8_refckpt_N{N}_K{K}.npz"), N=N, K=K,
        wq=wt.qdata.view(torch.uint8).numpy(),
        ws=wt._scale_e8m0.view(torch.uint8).reshape(N, K // 32).numpy(), bias=bf16_bits(bias),
        gemm_kernel_choice=np.array(wt._gemm_kernel_choice.value),
    )
    print("mxfp8 reference checkpoint", N, K)


if __name__ == "__main__":
    main()
