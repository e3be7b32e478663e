"""Generate the W4A8 fixtures under tests/golden/ by running the REFERENCE torchao on the CPU
(Int8DynamicActivationInt4WeightConfig(layout=CutlassInt4PackedLayout(), act_mapping_type=
SYMMETRIC): quantize_, the two quantizers, a saved state dict).

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 experiments/gen_golden_w4a8.py

Only data is written; bf16 tensors are stored as their uint16 bit patterns.

  w4a8_N64_K256.npz (bias), w4a8_N96_K1024.npz (no bias), w4a8_N40_K288.npz (bias; N is not a
  multiple of 16, K % 256 = 32)
      w, bias, x       bf16 bits [N, K], [N] (absent without bias), [6, K]
      wq_packed, ws    int8 [N, K/2], float32 [N]: int_data and scale of the reference's
                       Int4PackedTensorImpl after quantize_
      xq, xs           int8 [6, K], float32 [6]: the reference's _int8_symm_cutlass_quant(x)
      y_ref            bf16 bits [6, N]: the formula of the reference's own op test
                       (test/test_ops_rowwise_scaled_linear_cutlass.py) with the accumulation exact:
                       bf16(fp32(Xq.int32 @ Wq.int32.T) * xs[m] * ws[n] + fp32(bias[n])); the
                       reference's linear raises on the CPU, so there is no forward to record
      y64              float64 [6, N]: the unquantized product x @ w^T + bias
  w4a8_refckpt_N32_K64.pt
      the state dict of Sequential(Linear(64, 32, bias=True)) the reference saved after quantize_
  w4a8_refckpt_N32_K64_io.npz
      w, bias, x, y_ref for that checkpoint (as above)

Conditions asserted on the inputs (not a tolerance of any test): token 1 is all zeros; token 2 has
its largest-magnitude element negative and the code -128 occurs in it; weight row 1 is all zeros;
weight row 2 has a negative maximum and holds the code -8; every code value from -8 to 7 occurs in
both nibble positions.

Recorded relative L2 error of y_ref against y64 (CPU run of the reference's quantizers; a record,
not a threshold): N64_K256 0.1151, N96_K1024 0.1319, N40_K288 0.1112. Tokens are Gaussian with one
outlier channel boosted 20 times, except the two special tokens.
"""

import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
CASES = [(64, 256, True, 1200), (96, 1024, False, 1201), (40, 288, True, 1202)]
M = 6


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def rel_l2(y, ref):
    return float((y.double() - ref).norm() / ref.norm())


def unpack(p):
    return torch.stack(((p << 4) >> 4, p >> 4), dim=-1).view(p.shape[0], -1)


def make_inputs(N, K, has_bias, seed, quant_x, quant_w):
    gen = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=gen) * 0.05).to(torch.bfloat16)
    w[1] = 0
    bias = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16) if has_bias else None
    x = torch.randn(M, K, generator=gen)
    x[:, int(torch.randint(K, (1,), generator=gen))] *= 20.0  # one outlier channel
    x = x.to(torch.bfloat16)
    x[1] = 0
    # Token 2: a negative extreme that takes the code -128. With a bf16 amax = (k / 128) 2^e the
    # quotient amax / 127.5 has the mantissa k * 1.0039..., whose fraction lies above one half for
    # every k but 255, so its bf16 rounding goes up and |x| / s stays below 127.5: the code -128
    # needs k = 255 (amax / 127.5 is then the power of two 2^(e - 6), and -127.5 rounds to even).
    j = int(x[2].float().abs().argmax())
    e = int(np.ceil(np.log2(float(x[2].float().abs().max()))))
    x[2, j] = -(255.0 / 128.0) * 2.0 ** e
    q = quant_x(x[2:3])
    assert int(q.min()) == -128 and int(q[0, j]) == -128
    assert int(x[2].float().abs().argmax()) == j
    # Weight row 2: a negative maximum that takes the code -8; here the rounding of amax / 7.5
    # goes either way, so step the magnitude until |w| / s >= 7.5
    j = int(w[2].float().abs().argmax())
    base = float(w[2].float().abs().max())
    for step in range(64):
        w[2, j] = -(base * (1.0 + step / 64.0) + 1e-3)
        q = quant_w(w[2:3])
        if int(q.min()) == -8 and int(q[0, j]) == -8:
            break
    else:
        raise AssertionError("no magnitude gave the code -8")
    assert int(w[2].float().abs().argmax()) == j and float(w[2, j]) < 0
    return w, bias, x


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH"
    )
    from torchao.dtypes import CutlassInt4PackedLayout
    from torchao.dtypes.uintx.cutlass_int4_packed_layout import Int4PackedTensorImpl
    from torchao.quantization import Int8DynamicActivationInt4WeightConfig, quantize_
    from torchao.quantization.quant_api import _int4_symm_cutlass_quant, _int8_symm_cutlass_quant
    from torchao.quantization.quant_primitives import MappingType

    config = Int8DynamicActivationInt4WeightConfig(
        layout=CutlassInt4PackedLayout(), act_mapping_type=MappingType.SYMMETRIC)

    def quant_x(t):
        return _int8_symm_cutlass_quant(t).tensor_impl.int_data

    def quant_w(t):
        return _int4_symm_cutlass_quant(t).tensor_impl.get_plain()[0]

    def record(N, K, has_bias, seed, all_codes=True):
        w, bias, x = make_inputs(N, K, has_bias, seed, quant_x, quant_w)
        lin = torch.nn.Linear(K, N, bias=has_bias, dtype=torch.bfloat16)
        with torch.no_grad():
            lin.weight.copy_(w)
            if has_bias:
                lin.bias.copy_(bias)
        model = torch.nn.Sequential(lin)
        quantize_(model, config)
        wt = model[0].weight
        assert wt.input_quant_func is _int8_symm_cutlass_quant
        impl = wt.original_weight_tensor.tensor_impl
        assert isinstance(impl, Int4PackedTensorImpl)
        wq_packed, ws = impl.int_data, impl.scale
        assert wq_packed.dtype == torch.int8 and tuple(wq_packed.shape) == (N, K // 2)
        assert ws.dtype == torch.float32 and tuple(ws.shape) == (N,)
        xa = _int8_symm_cutlass_quant(x)
        xq, xs = xa.tensor_impl.int_data, xa.tensor_impl.scale
        assert xq.dtype == torch.int8 and tuple(xq.shape) == (M, K)
        assert xs.dtype == torch.float32 and tuple(xs.shape) == (M,)
        assert xa.tensor_impl.zero_point is None

        wq = unpack(wq_packed)
        assert torch.equal(wq, impl.get_plain()[0])
        assert not x[1].any() and not xq[1].any()
        assert int(xq[2].min()) == -128 and float(x[2].float().min()) == -float(x[2].float().abs().max())
        assert not w[1].any() and not wq_packed[1].any()
        assert int(wq[2].min()) == -8 and float(w[2].float().min()) == -float(w[2].float().abs().max())
        for half in (wq[:, 0::2], wq[:, 1::2]):
            assert not all_codes or sorted(set(half.flatten().tolist())) == list(range(-8, 8))

        acc = (xq.to(torch.int32) @ wq.to(torch.int32).t()).to(torch.float32)
        y = acc * xs.reshape(-1, 1) * ws.reshape(1, -1)
        y64 = x.double() @ w.double().t()
        if has_bias:
            y = y + bias.float()
            y64 = y64 + bias.double()
        y_ref = y.to(torch.bfloat16)
        rec = dict(N=N, K=K, w=bf16_bits(w), x=bf16_bits(x), wq_packed=wq_packed.numpy(),
                   ws=ws.numpy(), xq=xq.numpy(), xs=xs.numpy(), y_ref=bf16_bits(y_ref),
                   y64=y64.numpy())
        if has_bias:
            rec["bias"] = bf16_bits(bias)
        return rec, model, rel_l2(y_ref, y64)

    os.makedirs(OUT, exist_ok=True)
    with torch.no_grad():
        for N, K, has_bias, seed in CASES:
            rec, _, err = record(N, K, has_bias, seed)
            print(N, K, "rel-L2 of y_ref against y64:", round(err, 4))
            np.savez_compressed(os.path.join(OUT, f"w4a8_N{N}_K{K}.npz"), **rec)
        rec, model, _ = record(32, 64, True, 1203, all_codes=False)
        torch.save(model.state_dict(), os.path.join(OUT, "w4a8_refckpt_N32_K64.pt"))
        np.savez_compressed(os.path.join(OUT, "w4a8_refckpt_N32_K64_io.npz"),
                            **{k: rec[k] for k in ("N", "K", "w", "bias", "x", "y_ref")})


if __name__ == "__main__":
    main()
