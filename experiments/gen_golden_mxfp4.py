"""Generate the MXFP4-weight fixtures under tests/golden/ by running the REFERENCE torchao on the
CPU (e4m3fn activations x e2m1 weights, block 32, FLOOR).

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_mxfp4.py

The reference's ``MXFPInferenceConfig`` asserts equal dtypes, so the mixed recipe is built from its
own ``MXTensor.to_mx`` directly: the weight with ``torch.float4_e2m1fn_x2`` and e4m3fn
``act_quant_kwargs``; its emulated ``F.linear`` then computes the mixed product. Inputs and outputs
are recorded as data; bf16 tensors are stored as their uint16 bit patterns. Nothing of the
reference's source is stored.

  mxfp4w_N64_K256.npz, mxfp4w_N96_K1024.npz, mxfp4w_N40_K352.npz
      w, bias, x   bf16 bits [N, K], [N], [5, K]; tokens as in the mxfp8 fixtures (ZERO_TOKEN all
                   zero, OUTLIER_TOKEN one element of 200, a block of bf16 subnormals)
      wq, ws       uint8 [N, K/2], [N, K/32]  the reference's packed e2m1 codes (element 2j in the
                                              HIGH nibble of byte j) and E8M0 bytes
      xq, xs       uint8 [5, K], [5, K/32]    its e4m3fn activation codes and bytes
      w_deq        bf16 bits [N, K]           its to_dtype(bfloat16) of the weight (two smaller files)
      y64          float64 [5, N]   the formula in float64 on the codes, plus bias
      y_ref        bf16 bits [5, N] the reference's emulated F.linear(x, MXTensor fp4 w, bias)
  mxfp4_quant_edges.npz
      x            bf16 bits [R, 64]: blocks with NaN, +-inf, NaN beside inf, all zero, all
                   subnormal, -0.0 and tiny negatives, every rounding tie of e2m1 in both signs,
                   amaxes of 4, 6, 7 and 7.5 times a power of two, the bf16 number just below a
                   power of two, the largest and smallest normal exponents
      q, s, deq    the reference's packed codes, E8M0 bytes and to_dtype(bfloat16) bits
      nan_elems    [n, 2] (row, k) of the NaN input elements (their nibble's sign is not pinned)
  mxfp4w_refckpt_N32_K64.pt / .npz
      the state_dict of a nn.Linear whose weight is the reference's own fp4 MXTensor with e4m3fn
      act_quant_kwargs, as torch.save wrote it, and the same content as numbers.
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
SUBNORMAL_BLOCK = 1
E4 = torch.float8_e4m3fn
F4 = torch.float4_e2m1fn_x2
F4_VALUES = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6],
                         dtype=torch.float64)


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(v) -> torch.Tensor:
    return torch.tensor(np.asarray(v, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def edge_rows() -> torch.Tensor:
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(10, 64, generator=g) * 0.5).to(torch.bfloat16)
    x[0, 5] = float("nan")                       # a NaN block
    x[0, 32 + 9] = float("inf")                  # a +inf block
    x[1, :32] = 0                                # all zero
    x[1, 32:] = from_bits(np.arange(1, 33) * 3)  # all bf16 subnormals
    x[2, :32] = x[2, :32].clamp(-3, 3)
    x[2, 3] = 8.0                                # amax exactly a power of two
    x[2, 32:] = x[2, 32:].clamp(-3, 3)
    x[2, 32 + 3] = -7.96875                      # the bf16 number just below it
    # every tie, in units of the block scale (amax 4 * 2^-3 -> scale 2^-3), both signs, and -0.0
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, 4.0, 0.0, 0.125, 0.375, 6.0,
                         5.5, 4.5, 0.2490234375])
    x[3, :16] = (ties * 0.125).to(torch.bfloat16)
    x[3, 16:32] = (-ties * 0.125).to(torch.bfloat16)
    x[3, 32:] = x[3, 32:].clamp(-1, 1) * 2.0 ** -20
    x[3, 32 + 2] = -0.0
    x[3, 32 + 3] = -(2.0 ** -30)                 # tiny negatives beside a larger amax
    x[3, 32 + 4] = from_bits([0x8001])[0]
    # saturation: amaxes 4, 6, 7 and 7.5 times a power of two
    x[4, :32] = x[4, :32].clamp(-1, 1)
    x[4, 0] = 4.0
    x[4, 32:] = x[4, 32:].clamp(-1, 1) * 16
    x[4, 32 + 1] = -96.0                         # 6 * 2^4
    x[5, :32] = x[5, :32].clamp(-1, 1) * 0.25
    x[5, 2] = 1.75                               # 7 * 2^-2: saturates at 6
    x[5, 3] = -1.75
    x[5, 32:] = x[5, 32:].clamp(-1, 1) * 2.0 ** 10
    x[5, 32 + 6] = -7.5 * 2.0 ** 10
    x[5, 32 + 7] = 7.5 * 2.0 ** 10
    x[6, :32] = x[6, :32] * 1e38                 # exponent field 253 / 254
    x[6, 0] = 3.0e38
    x[6, 32:] = x[6, 32:] * 2.0 ** -124          # small normals: scale byte 0 / 1
    x[7, :32] = from_bits(np.arange(1, 33) * 3)
    x[7, 7] = 2.0 ** -125                        # subnormals beside a small normal amax
    x[7, 32 + 4] = float("-inf")
    x[7, 32 + 5] = float("nan")                  # NaN beside inf: NaN wins
    x[8, 1] = float("-inf")                      # -inf alone
    x[8, 32 + 31] = -float("nan")                # a negative NaN, last element of its block
    x[9, :32] = x[9, :32].clamp(-1, 1) * 2.0 ** -126   # byte 0 with normal and subnormal members
    x[9, 0] = 2.0 ** -126
    x[9, 1] = 3.0 * 2.0 ** -126
    x[9, 32:] = x[9, 32:].clamp(-1, 1)
    x[9, 32] = 3.984375                          # just below 4: scale from exponent 1
    return x


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH"
    )
    from torchao.prototype.mx_formats.config import MXGemmKernelChoice
    from torchao.prototype.mx_formats.mx_tensor import MXTensor, QuantizeTensorToMXKwargs

    def quantize(t, dtype):
        mx = MXTensor.to_mx(t.contiguous(), dtype, 32)
        return mx, mx.qdata.view(torch.uint8), mx._scale_e8m0.view(torch.uint8).reshape(
            *t.shape[:-1], t.shape[-1] // 32)

    def f4_values(q):  # [R, K/2] bytes -> float64 [R, K], element 2j from the high nibble
        u = torch.stack([q >> 4, q & 0xF], -1).reshape(q.shape[0], -1).long()
        return F4_VALUES[u]

    def scaled(f, s):
        return (f.reshape(f.shape[0], -1, 32) * torch.exp2(s.double() - 127)[..., None]).reshape(
            f.shape[0], -1)

    kw = QuantizeTensorToMXKwargs(elem_dtype=E4, block_size=32,
                                  gemm_kernel_choice=MXGemmKernelChoice.EMULATED)
    os.makedirs(OUT, exist_ok=True)
    for idx, (N, K) in enumerate([(64, 256), (96, 1024), (40, 352)]):
        g = torch.Generator().manual_seed(400 + idx)
        w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
        x = torch.randn(M, K, generator=g).to(torch.bfloat16)
        bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
        x[ZERO_TOKEN] = 0
        x[OUTLIER_TOKEN, 7] = 200.0
        x[SUBNORMAL_TOKEN, 32 * SUBNORMAL_BLOCK:32 * (SUBNORMAL_BLOCK + 1)] = from_bits(
            np.arange(1, 33) * 2)
        wmx, wq, ws = quantize(w, F4)
        xmx, xq, xs = quantize(x, E4)
        assert wq.shape == (N, K // 2) and tuple(wmx.shape) == (N, K)
        assert int(xs[ZERO_TOKEN].max()) == 0 and int(xq[ZERO_TOKEN].max()) == 0
        y64 = scaled(xq.view(E4).double(), xs) @ scaled(f4_values(wq), ws).t() + bias.double()
        assert bool(y64.isfinite().all())
        wlin = MXTensor.to_mx(w, F4, 32, gemm_kernel_choice=MXGemmKernelChoice.EMULATED,
                              act_quant_kwargs=kw)
        with torch.no_grad():
            y_ref = torch.nn.functional.linear(x, wlin, bias)
        assert y_ref.dtype == torch.bfloat16 and y_ref.shape == (M, N)
        extra = {"w_deq": bf16_bits(wmx.to_dtype(torch.bfloat16))} if N * K <= 16384 else {}
        np.savez_compressed(
            os.path.join(OUT, f"mxfp4w_N{N}_K{K}.npz"),
            N=N, K=K, zero_token=ZERO_TOKEN, outlier_token=OUTLIER_TOKEN,
            subnormal_token=SUBNORMAL_TOKEN, subnormal_block=SUBNORMAL_BLOCK,
            w=bf16_bits(w), x=bf16_bits(x), bias=bf16_bits(bias),
            wq=wq.numpy(), ws=ws.numpy(), xq=xq.numpy(), xs=xs.numpy(),
            y64=y64.numpy(), y_ref=bf16_bits(y_ref), **extra,
        )
        err = float((y_ref.double() - y64).norm() / y64.norm())
        full = float((y64 - (x.double() @ w.double().t() + bias.double())).norm() / y64.norm())
        print("mxfp4w", N, K, "reference emulated vs y64:", err, " y64 vs unquantised:", full)

    x = edge_rows()
    mx, q, s = quantize(x, F4)
    nan_elems = torch.nonzero(torch.isnan(x.float())).numpy()
    np.savez_compressed(os.path.join(OUT, "mxfp4_quant_edges.npz"), x=bf16_bits(x), q=q.numpy(),
                        s=s.numpy(), deq=bf16_bits(mx.to_dtype(torch.bfloat16)),
                        nan_elems=nan_elems)
    print("edges: scale bytes\n", s.numpy(), "\nNaN elements", nan_elems.tolist())
    print("ties row", [hex(v) for v in q[3, :16].tolist()])

    N, K = 32, 64
    g = torch.Generator().manual_seed(410)
    lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_((torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16))
        lin.bias.copy_((torch.randn(N, generator=g) * 0.1).to(torch.bfloat16))
    bias = lin.bias.detach().clone()
    kw = QuantizeTensorToMXKwargs(elem_dtype=E4, block_size=32,
                                  gemm_kernel_choice=MXGemmKernelChoice.CUBLAS)
    wt = MXTensor.to_mx(lin.weight.detach(), F4, 32, gemm_kernel_choice=MXGemmKernelChoice.CUBLAS,
                        act_quant_kwargs=kw)
    lin.weight = torch.nn.Parameter(wt, requires_grad=False)
    torch.save(lin.state_dict(), os.path.join(OUT, f"mxfp4w_refckpt_N{N}_K{K}.pt"))
    wt = lin.weight
    np.savez_compressed(
        os.path.join(OUT, f"mxfp4w_refckpt_N{N}_K{K}.npz"), N=N, K=K,
        wq=wt.qdata.view(torch.uint8).numpy(),
        ws=wt._scale_e8m0.view(torch.uint8).reshape(N, K // 32).numpy(), bias=bf16_bits(bias),
        gemm_kernel_choice=np.array(wt._gemm_kernel_choice.value),
    )
    print("mxfp4w reference checkpoint", N, K)


if __name__ == "__main__":
    main()
