"""Generate the AWQ fixtures under tests/golden/ by running the REFERENCE torchao on the CPU
(torchao.prototype.awq over Int4WeightOnlyConfig(layout=Int4CPULayout(), version=1)).

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_awq.py

Only data is written; bf16 tensors are stored as their uint16 bit patterns. ``get_plain()`` of the
reference's tensor impl returns layout-independent int32 codes [N, K] and bf16 scales / zeros
[N, K/g], so the CPU layout's results pin the GPU layout's.

  awq_N64_K256_g32.npz, awq_N96_K1024_g64.npz, awq_N48_K512_g128.npz
      w, bias, calib   bf16 bits [N, K], [N], [T, K]: K/32 outlier channels boosted 20 to 50 times
      outliers         the boosted channels
      per search size n in (3, 5, 20):
        scale_n, index_n, losses_n   the reference observer's chosen scale (bf16 bits [K]), its
                                     candidate index, and the loss of every candidate. The table is
                                     recorded by restating the loop over the reference's own
                                     handler; the observer's result is asserted equal to that
                                     loop's first strict minimum.
      for the size-5 scale:
        q, s, z          the reference's int32 codes [N, K] (values 0..15, stored as uint8), bf16
                         scales and zeros [N, K/g] of weight * scale (get_plain())
        x                bf16 bits [5, K] test tokens
        y_ref            bf16 bits [5, N] the reference's CPU forward of the converted module
        y64              float64 [5, N] bf16(x / scale) @ ((q - 8) * s + z)^T + bias in float64
  awq_refckpt_N48_K352_g32.pt / .npz
      the reference TensorCoreTiledLayout AQT of ref_ckpt_rocm_N48_K352_g32_ikt8.pt, loaded with the
      reference's classes, wrapped by its to_weight_tensor_with_linear_activation_scale_metadata
      with a recorded scale, as torch.save wrote the state_dict of an nn.Linear holding it; and the
      same content as numbers (q_u8, s, z of the source fixture, scale bits, fmt).

Conditions asserted on the inputs (they make the argmin well separated; not tolerances):
  size 3: second-best / best loss >= 2;  size 5: second-best / best >= 1.3 and the loss at ratio 0
  (plain int4) >= 3 times the best.
"""

import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
SIZES = (3, 5, 20)
CASES = [(64, 256, 32, 700), (96, 1024, 64, 701), (48, 512, 128, 703)]
T = 96  # calibration tokens
M = 5


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(v) -> torch.Tensor:
    return torch.tensor(np.asarray(v, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH"
    )
    from torchao.dtypes import Int4CPULayout
    from torchao.prototype.awq import AWQConfig
    from torchao.prototype.awq.core import AWQObserver
    from torchao.quantization import Int4WeightOnlyConfig, quantize_
    from torchao.quantization.linear_activation_scale import (
        WeightTensorWithLinearActivationScaleMetadata,
        to_weight_tensor_with_linear_activation_scale_metadata,
    )
    from torchao.quantization.transform_module import _QUANTIZE_CONFIG_HANDLER
    from torchao.utils import DummyModule

    os.makedirs(OUT, exist_ok=True)
    for N, K, g, seed in CASES:
        gen = torch.Generator().manual_seed(seed)
        w = (torch.randn(N, K, generator=gen) * 0.05).to(torch.bfloat16)
        bias = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)
        outliers = torch.randperm(K, generator=gen)[: K // 32].sort().values
        boost = 20 + 30 * torch.rand(K // 32, generator=gen)
        calib = torch.randn(T, K, generator=gen)
        calib[:, outliers] *= boost
        calib = calib.to(torch.bfloat16)
        x = torch.randn(M, K, generator=gen)
        x[:, outliers] *= boost
        x = x.to(torch.bfloat16)
        base = Int4WeightOnlyConfig(group_size=g, layout=Int4CPULayout(), version=1)
        handler = _QUANTIZE_CONFIG_HANDLER[type(base)]
        rec = {}
        with torch.no_grad():
            mean = calib.abs().view(-1, K).mean(0)
            orig = F.linear(calib, w, bias)
            for n in SIZES:
                losses, cands = [], []
                for i in range(n):
                    s = mean.pow(i / n).to(w.dtype).clamp(min=1e-4).view(-1)
                    s = s / (s.max() * s.min()).sqrt()
                    qw = handler(DummyModule(w * s), base).weight
                    losses.append((orig - F.linear(calib / s, qw, bias)).pow(2).mean().item())
                    cands.append(s)
                best = min(range(n), key=lambda i: (losses[i], i))  # the first strict minimum
                obs = AWQObserver(w, bias, base, n)
                obs(calib, None)
                chosen = obs.calculate_qparams()
                assert chosen.dtype == torch.bfloat16 and chosen.shape == (K,)
                assert torch.equal(chosen, cands[best]), (N, K, n, best, losses)
                srt = sorted(losses)
                if n == 3:
                    assert srt[1] / srt[0] >= 2, (N, K, losses)
                if n == 5:
                    assert srt[1] / srt[0] >= 1.3, (N, K, losses)
                    assert losses[0] >= 3 * srt[0], (N, K, losses)
                rec[f"scale_{n}"] = bf16_bits(chosen)
                rec[f"index_{n}"] = best
                rec[f"losses_{n}"] = np.asarray(losses, dtype=np.float64)
                print(N, K, g, "n", n, "best", best, "second/best", srt[1] / srt[0],
                      "ratio0/best", losses[0] / srt[0])
            # the whole flow through the reference's quantize_, at 5 candidates
            lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
            lin.weight.copy_(w)
            lin.bias.copy_(bias)
            model = torch.nn.Sequential(lin)
            quantize_(model, AWQConfig(base, step="prepare", scale_search_space_size=5))
            model(calib)
            quantize_(model, AWQConfig(base, step="convert", scale_search_space_size=5))
            wt = model[0].weight
            assert isinstance(wt, WeightTensorWithLinearActivationScaleMetadata)
            scale = wt.scale
            assert torch.equal(scale, from_bits(rec["scale_5"]))
            q, s, z = wt.original_weight_tensor.tensor_impl.get_plain()
            assert q.dtype == torch.int32 and tuple(q.shape) == (N, K)
            s, z = s.reshape(N, K // g), z.reshape(N, K // g)
            y_ref = model(x)
            model.state_dict()  # the reference's flow ends here; must not raise
            deq = ((q.double() - 8).reshape(N, K // g, g) * s.double()[..., None]
                   + z.double()[..., None]).reshape(N, K)
            y64 = (x / scale).double() @ deq.t() + bias.double()
        np.savez_compressed(
            os.path.join(OUT, f"awq_N{N}_K{K}_g{g}.npz"), N=N, K=K, g=g,
            w=bf16_bits(w), bias=bf16_bits(bias), calib=bf16_bits(calib),
            outliers=outliers.numpy(), q=q.numpy().astype(np.uint8), s=bf16_bits(s),
            z=bf16_bits(z), x=bf16_bits(x), y_ref=bf16_bits(y_ref), y64=y64.numpy(), **rec)
        print("  y_ref vs y64:", float((y_ref.double() - y64).norm() / y64.norm()))

    # a reference AWQ checkpoint over the reference's own TensorCoreTiledLayout tensor
    src = "ref_ckpt_rocm_N48_K352_g32_ikt8"
    sd = torch.load(os.path.join(OUT, src + ".pt"), weights_only=True)
    aqt = sd["weight"]
    N, K = aqt.shape
    gen = torch.Generator().manual_seed(710)
    scale = (0.25 + 3 * torch.rand(K, generator=gen)).to(torch.bfloat16)
    lin = torch.nn.Linear(K, N, bias="bias" in sd, dtype=torch.bfloat16)
    lin.weight = torch.nn.Parameter(
        to_weight_tensor_with_linear_activation_scale_metadata(aqt, scale), requires_grad=False)
    if "bias" in sd:
        lin.bias = torch.nn.Parameter(sd["bias"], requires_grad=False)
    torch.save(lin.state_dict(), os.path.join(OUT, "awq_refckpt_N48_K352_g32.pt"))
    num = np.load(os.path.join(OUT, src + ".npz"))
    np.savez_compressed(os.path.join(OUT, "awq_refckpt_N48_K352_g32.npz"),
                        scale=bf16_bits(scale), **{k: num[k] for k in num.files})
    print("awq reference checkpoint", N, K, sorted(num.files))


if __name__ == "__main__":
    main()
