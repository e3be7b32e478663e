"""Generate the MoE fixtures under tests/golden/ by running the REFERENCE torchao on the CPU.

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_moe.py

It imports the reference's own ``MOEFeedForwardAOQuantizable``, ``MoEQuantConfig``,
``UseFakeExtraDimTensor``, ``cond_ffn_filter``, ``quantize_`` and ``Int8WeightOnlyConfig``, runs
the module on the CPU in bf16 and records inputs and outputs as data; bf16 tensors are stored as
their uint16 bit patterns. Nothing of the reference's source is stored.

  moe_E4_D64_I128_k{A}.npz   A in (1, 2, 3): one module (E = 4, hidden 64, expert 128, top-A)
      router, w1, w2, w3    bf16 bits [4, 64], [4, 128, 64], [4, 64, 128], [4, 128, 64]
      x_T{T}                bf16 bits [T, 1, 64], T in (1, 2, 7): T = 1 takes the module's one-token
                            branch, the others its many-token branch
      idx_T{T}              int64 [T, A]          the experts' own input expert_indices
      scores_T{T}           bf16 bits [T, A]      the normalised top-A scores (return_scores)
      y_T{T}                bf16 bits [T, 1, 64]  the plain module's output
      yq8_T{T}              bf16 bits [T, 1, 64]  its output after
                            quantize_(m, MoEQuantConfig(Int8WeightOnlyConfig(),
                            UseFakeExtraDimTensor.FALSE), cond_ffn_filter)

Asserted here, so that a failing test cannot be the fixture's fault: the indices seen by the
experts are those of the recorded scores' top-k, every T > 1 case routes to at least two experts,
and the int8-quantized output stays within 5e-2 rel-L2 of the plain one.
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
E, D, I = 4, 64, 128
TOKENS = (1, 2, 7)
TOP_KS = (1, 2, 3)


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH")
    from torchao.prototype.moe_quant.quantizable_moe_modules import MOEFeedForwardAOQuantizable
    from torchao.prototype.moe_quant.utils import (MoEQuantConfig, UseFakeExtraDimTensor,
                                                   cond_ffn_filter)
    from torchao.quantization import Int8WeightOnlyConfig, quantize_

    os.makedirs(OUT, exist_ok=True)
    for A in TOP_KS:
        seed = 4100 + A
        g = torch.Generator().manual_seed(seed)
        m = MOEFeedForwardAOQuantizable(D, I, E, A, return_scores=True, empty_init=False)
        m = m.to(torch.bfloat16)
        with torch.no_grad():
            m.router.weight.copy_(torch.randn(E, D, generator=g) * 0.5)
            m.experts.w1.copy_(torch.randn(E, I, D, generator=g) / D ** 0.5)
            m.experts.w2.copy_(torch.randn(E, D, I, generator=g) / I ** 0.5)
            m.experts.w3.copy_(torch.randn(E, I, D, generator=g) / D ** 0.5)
        rec = {"router": bits(m.router.weight), "w1": bits(m.experts.w1),
               "w2": bits(m.experts.w2), "w3": bits(m.experts.w3), "seed": np.int64(seed)}
        seen = {}
        hook = m.experts.register_forward_pre_hook(
            lambda mod, args: seen.__setitem__("idx", args[1].detach().clone()))
        xs = {}
        with torch.no_grad():
            for T in TOKENS:
                x = torch.randn(T, 1, D, generator=g).to(torch.bfloat16)
                y, scores = m(x)
                idx = seen["idx"]
                assert idx.shape == (T, A) and scores.shape == (T, A)
                assert T == 1 or idx.unique().numel() >= 2, f"T={T} top-{A}: one expert only"
                xs[T] = x
                rec.update({f"x_T{T}": bits(x), f"idx_T{T}": idx.numpy().astype(np.int64),
                            f"scores_T{T}": bits(scores), f"y_T{T}": bits(y)})
            quantize_(m, MoEQuantConfig(Int8WeightOnlyConfig(), UseFakeExtraDimTensor.FALSE),
                      cond_ffn_filter)
            for T in TOKENS:
                yq, _ = m(xs[T])
                assert torch.equal(seen["idx"], torch.from_numpy(rec[f"idx_T{T}"]))
                err = rel_l2(yq, torch.from_numpy(rec[f"y_T{T}"].view(np.int16)).view(torch.bfloat16))
                assert err <= 5e-2, f"top-{A} T={T}: int8 output off by {err}"
                rec[f"yq8_T{T}"] = bits(yq)
                print(f"moe top-{A} T={T}: rel_l2(int8wo, plain) {err:.3e}")
        hook.remove()
        np.savez_compressed(os.path.join(OUT, f"moe_E{E}_D{D}_I{I}_k{A}.npz"), **rec)


if __name__ == "__main__":
    sys.exit(main())
