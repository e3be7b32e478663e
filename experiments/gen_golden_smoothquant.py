"""Generate the SmoothQuant fixtures under tests/golden/ by running the REFERENCE torchao on the
CPU (torchao.prototype.smoothquant: observer, SmoothQuantConfig convert, recipe save, forward).

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 experiments/gen_golden_smoothquant.py

Only data is written; bf16 tensors are stored as their uint16 bit patterns.

  smoothquant_N64_K256.npz (bias), smoothquant_N96_K1024.npz (no bias), smoothquant_N48_K512.npz
      w, bias, calib   bf16 bits [N, K], [N] (absent without bias), [T, K]: K/32 outlier channels
                       boosted 20 to 50 times
      outliers         the boosted channels
      x                bf16 bits [5, K] test tokens: 0 and 4 drawn like calib; 1 all zeros; 2 small
                       enough that the dynamic quantizer's 2^-7 scale clamp binds for every alpha;
                       3 five times the calibrated magnitude, so the static codes saturate
      y64              float64 [5, N]: the unquantized product x @ w^T + bias
      per alpha in (None, 0.5, 0.75) and mode in (dynamic, static), keys <name>_<tag> with tag
      aNone_dynamic, a0.5_static, ...:
        smoothing_factor   bf16 bits [K]      the observer's calculate_qparams()
        act_scales         bf16 bits []       (static only)
        wei_scales         bf16 bits [N]
        wq, ws             int8 [N, K], bf16 bits [N]: the converted weight's codes and scale
        xq, xs             int8 [5, K], bf16 bits [5] (dynamic) or [] (static): what the
                           reference's _ActQuantizer gives for x / smoothing_factor
        y_ref              bf16 bits [5, N] the reference's CPU forward of the converted module
  smoothquant_recipe_N*_K*_<mode>.pt
      the recipe file save_smooth_quant_recipe wrote for the alpha = 0.5 observed model
      (Sequential(linear): keys 0.smoothing_factor, 0.act_scales, 0.wei_scales)

Condition asserted on the inputs (not a tolerance of any test): at alpha 0.5 the reference's plain
Int8DynamicActivationInt8WeightConfig linear has at least 1.5 times the relative L2 error of the
SmoothQuant linear, dynamic and static, against the float64 product on the calibration tokens.
Also asserted: token 2's dynamic scale is 2^-7 and token 3 saturates static codes, for every alpha.
"""

import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
CASES = [(64, 256, True, 900), (96, 1024, False, 901), (48, 512, True, 902)]
ALPHAS = (None, 0.5, 0.75)
MODES = ("dynamic", "static")
T = 64  # calibration tokens
M = 5


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def rel_l2(y, ref):
    return float((y.double() - ref).norm() / ref.norm())


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH"
    )
    from torchao.prototype.smoothquant import (
        SmoothQuantConfig,
        SmoothQuantObservedLinear,
        insert_smooth_quant_observer_,
        save_smooth_quant_recipe,
    )
    from torchao.prototype.smoothquant.api import _ActQuantizer
    from torchao.quantization import Int8DynamicActivationInt8WeightConfig, quantize_
    from torchao.quantization.linear_activation_quantized_tensor import (
        LinearActivationQuantizedTensor,
    )
    from torchao.quantization.linear_activation_scale import (
        WeightTensorWithLinearActivationScaleMetadata,
    )
    from torchao.quantization.weight_tensor_linear_activation_quantization import (
        WeightTensorWithLinearActivationQuantizationMetadata,
    )

    def is_observed(m, fqn):
        return isinstance(m, SmoothQuantObservedLinear)

    os.makedirs(OUT, exist_ok=True)
    for N, K, has_bias, seed in CASES:
        gen = torch.Generator().manual_seed(seed)
        w = (torch.randn(N, K, generator=gen) * 0.05).to(torch.bfloat16)
        bias = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16) if has_bias else None
        outliers = torch.randperm(K, generator=gen)[: K // 32].sort().values
        boost = 20 + 30 * torch.rand(K // 32, generator=gen)

        def draw(rows, mul=1.0):
            t = torch.randn(rows, K, generator=gen) * mul
            t[:, outliers] *= boost
            return t.to(torch.bfloat16)

        calib = draw(T)
        x = draw(M)
        x[1] = 0
        x[2] = (0.15 * torch.randn(K, generator=gen)).to(torch.bfloat16)
        x[3] = draw(1, 5.0)[0]

        def linear():
            lin = torch.nn.Linear(K, N, bias=has_bias, dtype=torch.bfloat16)
            with torch.no_grad():
                lin.weight.copy_(w)
                if has_bias:
                    lin.bias.copy_(bias)
            return torch.nn.Sequential(lin)

        def f64(t):
            y = t.double() @ w.double().t()
            return y + bias.double() if has_bias else y

        rec = {}
        err = {}
        with torch.no_grad():
            plain = linear()
            quantize_(plain, Int8DynamicActivationInt8WeightConfig())
            err["plain"] = rel_l2(plain(calib), f64(calib))
            for alpha in ALPHAS:
                for mode in MODES:
                    tag = f"a{alpha}_{mode}"
                    model = linear()
                    insert_smooth_quant_observer_(model, alpha, mode)
                    model(calib)
                    factor, act_scales, wei_scales = model[0].obs.calculate_qparams()
                    assert factor.dtype == torch.bfloat16 and tuple(factor.shape) == (K,)
                    assert wei_scales.dtype == torch.bfloat16 and tuple(wei_scales.shape) == (N,)
                    if alpha == 0.5:
                        save_smooth_quant_recipe(
                            model, os.path.join(OUT, f"smoothquant_recipe_N{N}_K{K}_{mode}.pt"))
                    quantize_(model, SmoothQuantConfig(), is_observed)
                    wt = model[0].weight
                    assert isinstance(wt, WeightTensorWithLinearActivationScaleMetadata)
                    assert wt.scale.dtype == torch.bfloat16 and torch.equal(wt.scale, factor)
                    inner = wt.original_weight_tensor
                    t = x / wt.scale
                    if mode == "dynamic":
                        assert act_scales is None
                        assert isinstance(inner, LinearActivationQuantizedTensor)
                        assert inner.input_quant_func.__func__ is _ActQuantizer.dynamic_quantize
                        xa = inner.input_quant_func(t)
                        xs = xa.tensor_impl.scale.reshape(-1)
                        assert tuple(xs.shape) == (M,)
                        assert float(xs[1]) == 2.0 ** -7 and float(xs[2]) == 2.0 ** -7, xs
                    else:
                        assert act_scales.dtype == torch.bfloat16 and act_scales.dim() == 0
                        assert isinstance(
                            inner, WeightTensorWithLinearActivationQuantizationMetadata)
                        assert (inner.input_quant_func_static.__func__
                                is _ActQuantizer.static_quantize)
                        assert torch.equal(inner.scale, act_scales)
                        assert inner.zero_point.dtype == torch.int64 and not inner.zero_point.any()
                        xa = inner.input_quant_func_static(
                            t, scale=inner.scale, zero_point=inner.zero_point)
                        xs = xa.tensor_impl.scale
                        assert torch.equal(xs, act_scales)
                        big = (t[3].float().abs() / act_scales.float()) > 128
                        assert int(big.sum()) >= 1
                        assert bool((xa.tensor_impl.int_data[3][big].abs() == 127).all())
                        rec[f"act_scales_{tag}"] = bf16_bits(act_scales)
                    aqt = inner.original_weight_tensor
                    wq, ws, _ = aqt.tensor_impl.get_plain()
                    assert wq.dtype == torch.int8 and tuple(wq.shape) == (N, K)
                    assert torch.equal(ws.reshape(-1), wei_scales)
                    xq = xa.tensor_impl.int_data
                    assert xq.dtype == torch.int8 and tuple(xq.shape) == (M, K)
                    y_ref = model(x)
                    assert y_ref.dtype == torch.bfloat16 and tuple(y_ref.shape) == (M, N)
                    err[tag] = rel_l2(model(calib), f64(calib))
                    rec[f"smoothing_factor_{tag}"] = bf16_bits(factor)
                    rec[f"wei_scales_{tag}"] = bf16_bits(wei_scales)
                    rec[f"wq_{tag}"] = wq.numpy()
                    rec[f"ws_{tag}"] = bf16_bits(ws.reshape(-1))
                    rec[f"xq_{tag}"] = xq.numpy()
                    rec[f"xs_{tag}"] = bf16_bits(xs)
                    rec[f"y_ref_{tag}"] = bf16_bits(y_ref)
        print(N, K, {k: round(v, 5) for k, v in err.items()})
        for mode in MODES:
            assert err["plain"] >= 1.5 * err[f"a0.5_{mode}"], (N, K, mode, err)
        extra = {"bias": bf16_bits(bias)} if has_bias else {}
        np.savez_compressed(
            os.path.join(OUT, f"smoothquant_N{N}_K{K}.npz"), N=N, K=K, w=bf16_bits(w),
            calib=bf16_bits(calib), outliers=outliers.numpy(), x=bf16_bits(x),
            y64=f64(x).numpy(), **extra, **rec)


if __name__ == "__main__":
    main()
