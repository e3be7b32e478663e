"""Generate the FP6 fixtures under tests/golden/ by running the REFERENCE torchao on the CPU.

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_fp6.py

It imports the reference's own ``to_affine_quantized_fpx``, ``FloatxTensorCoreLayout``,
``quantize_`` and ``fpx_weight_only`` and records inputs and outputs as data; bf16 tensors are
stored as their uint16 bit patterns. Nothing of the reference's source is stored.

  fp6_{fmt}_N{N}_K{K}.npz   fmt in (e3m2, e2m3); N256 K64, N256 K320, N512 K192
      w, x, bias            bf16 bits [N, K], [5, K], [N]
      packed                uint8 [N, K * 6 / 8]   the reference's packed_floatx_data
      codes                 uint8 [N, K]           its get_plain()[0], 00SEEEMM
      scale                 bf16 bits [N]
      w_hat                 bf16 bits [N, K]       its dequantize()
      y_ref                 bf16 bits [5, N]       F.linear(x, w_hat, bias) on the CPU
      y64                   float64 [5, N]         (x . value(codes)) * scale + bias in float64
  fp6_quant_edges.npz   per format {fmt}_w, {fmt}_packed, {fmt}_codes, {fmt}_scale, {fmt}_w_hat of
                      a 64 x 256 weight whose rows hit: 0 all zero; 1 / 2 a scale of exactly
                      2^-3 with every midpoint of adjacent codes and its two bf16 neighbours,
                      positive / negative (ties); 3 the same scale with magnitudes around and
                      below half the smallest subnormal; 4 .. 11 row maxima whose bf16-rounded
                      scale is below amax / max_normal, so w / s exceeds max_normal (saturation;
                      at least one such row is asserted); 12 negative zeros and a negative row
                      maximum; 13 a row below the 1e-12 clamp; the rest random, rows of unequal
                      size. No inf, no NaN.
  fp6_refckpt_e3m2_N256_K64.pt / .npz
      the state_dict of a reference nn.Linear(64, 256) after quantize_(m, fpx_weight_only(3, 2))
      as torch.save wrote it, and the same content as numbers (w, bias, packed, codes, scale,
      w_hat).

Asserted here, so that a failing test cannot be the fixture's fault: the code -> value table of
the reference equals the formats' definition for all 64 codes, and rel_l2(y_ref, y64) <= 4e-3.
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
SHAPES = ((256, 64), (256, 320), (512, 192))
FORMATS = (("e3m2", 3, 2), ("e2m3", 2, 3))
M = 5


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def values(ebits, mbits):
    """The 64 values from the definition (bias 2^(ebits - 1) - 1, subnormals, no inf / NaN)."""
    bias = 2 ** (ebits - 1) - 1
    out = []
    for c in range(64):
        e, m = (c >> mbits) & (2**ebits - 1), c & (2**mbits - 1)
        mag = m * 2.0 ** (1 - bias - mbits) if e == 0 else (1 + m / 2**mbits) * 2.0 ** (e - bias)
        out.append(-mag if c >> 5 else mag)
    return torch.tensor(out, dtype=torch.float64)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def edge_weight(ebits, mbits, seed):
    g = torch.Generator().manual_seed(seed)
    N, K = 64, 256
    v = values(ebits, mbits)
    mx = v.max().item()
    pos = v[:32]
    row = 0.02 + 0.1 * torch.rand(N, 1, generator=g)
    w = (torch.randn(N, K, generator=g) * row).to(torch.bfloat16)
    w[0] = 0
    # rows 1, 2: amax = max * 2^-3, so the scale is exactly 2^-3 and w / s = 8 w exactly
    mids = ((pos[:-1] + pos[1:]) / 2 / 8).to(torch.bfloat16)
    assert torch.equal(mids.double() * 8, (pos[:-1] + pos[1:]) / 2), "midpoints must be bf16 numbers"
    mb = mids.view(torch.int16)
    trio = torch.stack([mb - 1, mb, mb + 1], -1).flatten().view(torch.bfloat16)
    for r, sgn in ((1, 1.0), (2, -1.0)):
        w[r] = 0
        w[r, 0] = sgn * mx / 8
        w[r, 1:1 + trio.numel()] = sgn * trio
    # row 3: around and below half the smallest subnormal (in units of the scale 2^-3)
    sub = v[1].item() / 8
    tiny = torch.tensor([0.49, 0.5, 0.51, 0.25, 1e-3, 1e-6, 0.75, 1.0, 1.49, 1.5, 1.51]) * sub
    tiny = tiny.to(torch.bfloat16)
    w[3] = 0
    w[3, 0] = mx / 8
    w[3, 1:1 + tiny.numel()] = tiny
    w[3, 32:32 + tiny.numel()] = -tiny
    # rows 4 .. 11: maxima whose bf16-rounded scale falls below amax / max
    found, cand = 0, 1.0
    while found < 8:
        a = torch.tensor(cand, dtype=torch.float32).to(torch.bfloat16)
        s = (a.float() / mx).to(torch.bfloat16)
        if (a.float() / s.float()).item() > mx:
            w[4 + found, 0] = a
            w[4 + found, 1] = -a
            w[4 + found, 2:] = (w[4 + found, 2:].float().clamp(-1, 1) * a.float()).to(torch.bfloat16)
            found += 1
        cand += 0.0390625
    w[12, :16] = -0.0
    w[12, 16] = -1.25
    w[12, 17:] = (w[12, 17:].float().clamp(-1, 1)).to(torch.bfloat16)
    w[13] = (torch.randn(K, generator=g) * 1e-13).to(torch.bfloat16)
    assert torch.isfinite(w.float()).all()
    return w


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH")
    from torchao.dtypes import to_affine_quantized_fpx
    from torchao.dtypes.floatx import FloatxTensorCoreLayout
    from torchao.prototype.custom_fp_utils import _floatx_unpacked_to_f32
    from torchao.quantization import fpx_weight_only, quantize_

    os.makedirs(OUT, exist_ok=True)

    def quantized(w, ebits, mbits):
        t = to_affine_quantized_fpx(w, FloatxTensorCoreLayout(ebits, mbits))
        impl = t.tensor_impl
        codes, scale = impl.get_plain()
        w_hat = t.dequantize()
        assert impl.packed_floatx_data.dtype is torch.uint8 and codes.dtype is torch.uint8
        assert scale.dtype is torch.bfloat16 and w_hat.dtype is torch.bfloat16
        return impl.packed_floatx_data, codes, scale, w_hat

    edges = {}
    for fi, (fmt, ebits, mbits) in enumerate(FORMATS):
        v = values(ebits, mbits)
        ref_v = _floatx_unpacked_to_f32(torch.arange(64, dtype=torch.uint8), ebits, mbits)
        assert torch.equal(ref_v.double(), v), f"{fmt}: the reference's table is not the definition"
        for si, (N, K) in enumerate(SHAPES):
            seed = 1000 * (fi + 1) + 100 * si
            g = torch.Generator().manual_seed(seed)
            row = 0.02 + 0.1 * torch.rand(N, 1, generator=g)  # rows of unequal size
            w = (torch.randn(N, K, generator=g) * row).to(torch.bfloat16)
            x = torch.randn(M, K, generator=g).to(torch.bfloat16)
            bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
            packed, codes, scale, w_hat = quantized(w, ebits, mbits)
            y_ref = torch.nn.functional.linear(x, w_hat, bias)
            y64 = (x.double() @ v[codes.long()].t()) * scale.double() + bias.double()
            err = rel_l2(y_ref, y64)
            assert err <= 4e-3, f"{fmt} N{N} K{K}: rel_l2(y_ref, y64) = {err}"
            np.savez_compressed(os.path.join(OUT, f"fp6_{fmt}_N{N}_K{K}.npz"), w=bits(w), x=bits(x),
                     bias=bits(bias), packed=packed.numpy(), codes=codes.numpy(),
                     scale=bits(scale), w_hat=bits(w_hat), y_ref=bits(y_ref), y64=y64.numpy(),
                     seed=np.int64(seed))
            print(f"fp6_{fmt}_N{N}_K{K}: seed {seed}, rel_l2(y_ref, y64) {err:.2e}")

        w = edge_weight(ebits, mbits, 7000 + fi)
        packed, codes, scale, w_hat = quantized(w, ebits, mbits)
        sat = (w.float() / scale.float().view(-1, 1)).abs().amax(1) > v.max().item()
        assert sat[4:12].all(), f"{fmt}: saturation rows do not exceed max_normal: {sat[4:12]}"
        assert (codes[0] == 0).all() and (codes[12, :16] == 0x20).all()
        edges.update({f"{fmt}_w": bits(w), f"{fmt}_packed": packed.numpy(),
                      f"{fmt}_codes": codes.numpy(), f"{fmt}_scale": bits(scale),
                      f"{fmt}_w_hat": bits(w_hat)})
        print(f"fp6_quant_edges {fmt}: {int(sat.sum())} saturating rows")
    np.savez_compressed(os.path.join(OUT, "fp6_quant_edges.npz"), **edges)

    N, K, seed = 256, 64, 9000
    torch.manual_seed(seed)
    m = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    w = m.weight.detach().clone()
    quantize_(m, fpx_weight_only(3, 2))
    sd = m.state_dict()
    path = os.path.join(OUT, f"fp6_refckpt_e3m2_N{N}_K{K}.pt")
    torch.save(sd, path)
    back = torch.load(path, weights_only=True)
    impl = sd["weight"].tensor_impl
    assert torch.equal(back["weight"].tensor_impl.packed_floatx_data, impl.packed_floatx_data)
    codes, scale = impl.get_plain()
    np.savez_compressed(os.path.join(OUT, f"fp6_refckpt_e3m2_N{N}_K{K}.npz"), w=bits(w), bias=bits(sd["bias"]),
             packed=impl.packed_floatx_data.numpy(), codes=codes.numpy(), scale=bits(scale),
             w_hat=bits(sd["weight"].dequantize()), seed=np.int64(seed))
    print(f"fp6_refckpt_e3m2_N{N}_K{K}: seed {seed}")


if __name__ == "__main__":
    sys.exit(main())
