"""Generate the NVFP4 fixtures under tests/golden/ by running the REFERENCE torchao on the CPU.

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_nvfp4.py

It imports the reference's own ``NVFP4Tensor``, ``per_tensor_amax_to_scale``, ``to_blocked``,
``quantize_`` and ``NVFP4InferenceConfig`` and records inputs and outputs as data; bf16 tensors are
stored as their uint16 bit patterns, e4m3 scales as bytes. Nothing of the reference's source is
stored.

  nvfp4_N{N}_K{K}.npz, nvfp4_N{N}_K{K}_pts.npz     N48 K64, N144 K320, N256 K1024; _pts: with a
                         per-tensor scale on the weight and on the activation
      w, x, bias         bf16 bits [N, K], [5, K], [N]; N(0, 1), a few blocks of w times 1e-3 / 1e3
      per_tensor_scale, act_per_tensor_scale      fp32 0-dim (_pts only):
                         per_tensor_amax_to_scale(amax|w|), (amax|x|)
      qdata              uint8 [N, K / 2]        to_nvfp4(w).qdata
      scales_rowmajor    uint8 [N, K / 16]       its _scale_e4m3 bytes
      scales_swizzled    uint8 flat              the same with is_swizzled_scales=True
      w_hat              bf16 bits [N, K]        its to_dtype(bfloat16)
      xq_codes, x_scales uint8 [5, K / 2], [5, K / 16]   to_nvfp4(x, per_tensor_scale=act scale)
      x_dq               bf16 bits [5, K]        value(code) * e4m3(scale) of x, asserted exact
      y_ref              bf16 bits [5, N]        F.linear(x, weight-only NVFP4Tensor, bias)
      y64_wo, y64_dyn    float64 [5, N]          alpha * (xq . (value(code) * e4m3(scale))) + bias
                         in float64; xq = x / x_dq, alpha = per_tensor_scale (* act_per_tensor_scale)
  nvfp4_quant_edges.npz  x bf16 bits [16, 128] and, without / with (_pts) a per-tensor scale,
                         qdata, scales_rowmajor, scales_swizzled, x_dq. Rows: 0 all zero; 1 / 2
                         blocks led by +-6 (scale exactly 1) holding every midpoint of adjacent e2m1
                         codes and its two bf16 neighbours; 3 block maxima at and below 6 * 2^-6 (the
                         scale's lower clamp); 4 maxima at and above 6 * 448 (its upper clamp); 5 / 6
                         maxima whose amax / 6 is a tie of two e4m3 numbers; 7 negative zeros under
                         a negative maximum; the rest N(0, 1). No inf, no NaN.
  nvfp4_refckpt_N32_K64.pt / .npz
      the state_dict of a reference nn.Linear(64, 32) after quantize_(m, NVFP4InferenceConfig(
      WEIGHT_ONLY, use_triton_kernel=False)) as torch.save wrote it, and the same content as numbers.

Asserted here, so that a failing test cannot be the fixture's fault: value(code) * e4m3(scale) is a
bf16 number for every element of every w and x, and rel_l2(y_ref, y64_wo) <= 4e-3.
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
SHAPES = ((48, 64), (144, 320), (256, 1024))
M = 5
# Seed offsets of the _pts fixtures. The reference rounds the per-tensor scale to bf16 (up to 2^-8
# relative, the same sign on every weight), so its own distance from float64 depends on the
# weight's maximum: at N48 K64 offset 0 gives 4.7e-3, above the bar asserted below; offset 1 1.8e-3.
PTS_SEED = (1, 0, 0)
E2M1 = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6],
                    dtype=torch.float64)


def bits(t):
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def u8(t):
    return t.detach().contiguous().view(torch.uint8).numpy()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def grid_values(qdata, scales):
    """float64 value(code) * e4m3(scale), asserted exactly representable in bf16."""
    codes = torch.stack([qdata >> 4, qdata & 0xF], -1).reshape(qdata.shape[0], -1).long()
    v = E2M1[codes].view(qdata.shape[0], -1, 16) * scales.double().unsqueeze(-1)
    v = v.view(qdata.shape[0], -1)
    assert torch.equal(v.to(torch.bfloat16).double(), v), "code * scale is not a bf16 number"
    return v


def edge_input(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(16, 128, generator=g).to(torch.bfloat16)
    x[0] = 0
    pos = E2M1[:8]
    mids = ((pos[:-1] + pos[1:]) / 2).to(torch.bfloat16)
    mb = mids.view(torch.int16)
    trio = torch.stack([mb - 1, mb, mb + 1], -1).flatten().view(torch.bfloat16)  # 21 values
    for r, sgn in ((1, 1.0), (2, -1.0)):
        x[r] = 0
        for b in range(2):
            part = trio[15 * b:15 * (b + 1)]
            x[r, 16 * b] = sgn * 6.0
            x[r, 16 * b + 1:16 * b + 1 + part.numel()] = sgn * part
    lows = [6 * 2.0 ** -6, 0.09, 0.05, 0.01, 1e-4, 6 * 2.0 ** -7, 0.0935, 1e-30]
    highs = [6 * 448.0, 2704.0, 3000.0, 1e4, 2680.0, 2672.0, 5e3, 2.5e3]
    ties = [6 * (a + b) / 2 * 2.0 ** e for e in (-4, 0, 3, 6)
            for a, b in ((1.0, 1.125), (1.125, 1.25), (1.75, 1.875), (1.875, 2.0))]
    for r, maxima in ((3, lows), (4, highs), (5, ties[:8]), (6, ties[8:])):
        for b, a in enumerate(maxima):
            a = torch.tensor(a, dtype=torch.float32).to(torch.bfloat16)
            blk = x[r, 16 * b:16 * (b + 1)].float().clamp(-1, 1) * a.float()
            x[r, 16 * b:16 * (b + 1)] = blk.to(torch.bfloat16)
            x[r, 16 * b + (b % 16)] = a if b % 2 == 0 else -a
    x[7, :16] = -0.0
    x[7, 16] = -1.25
    x[7, 17:32] = x[7, 17:32].float().clamp(-1, 1).to(torch.bfloat16)
    assert torch.isfinite(x.float()).all()
    return x


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH")
    from torchao.prototype.mx_formats.inference_workflow import NVFP4InferenceConfig
    from torchao.prototype.mx_formats.nvfp4_tensor import (NVFP4MMConfig, NVFP4Tensor,
                                                            per_tensor_amax_to_scale)
    from torchao.quantization import quantize_

    os.makedirs(OUT, exist_ok=True)

    def quantized(t, pts):
        plain = NVFP4Tensor.to_nvfp4(t, per_tensor_scale=pts)
        swz = NVFP4Tensor.to_nvfp4(t, per_tensor_scale=pts, is_swizzled_scales=True)
        assert torch.equal(plain.qdata, swz.qdata)
        assert torch.equal(swz.to_dtype(torch.bfloat16), plain.to_dtype(torch.bfloat16))
        return plain, swz

    for si, (N, K) in enumerate(SHAPES):
        for with_pts in (False, True):
            seed = 3000 + 100 * si + (PTS_SEED[si] if with_pts else 0)
            g = torch.Generator().manual_seed(seed)
            w = torch.randn(N, K, generator=g)
            blocks = w.view(N, K // 16, 16)
            for i, f in enumerate((1e-3, 1e3, 1e-3, 1e3)):
                blocks[(7 * i + 3) % N, (5 * i + 1) % (K // 16)] *= f
            w = w.to(torch.bfloat16)
            x = torch.randn(M, K, generator=g).to(torch.bfloat16)
            bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
            pts = per_tensor_amax_to_scale(w.abs().max()) if with_pts else None
            apts = per_tensor_amax_to_scale(x.abs().max()) if with_pts else None
            plain, swz = quantized(w, pts)
            xt = NVFP4Tensor.to_nvfp4(x, per_tensor_scale=apts)
            wv = grid_values(plain.qdata, plain._scale_e4m3)
            xv = grid_values(xt.qdata, xt._scale_e4m3)
            y_ref = torch.nn.functional.linear(x, swz, bias)
            assert y_ref.dtype is torch.bfloat16
            alpha = pts.double() if with_pts else 1.0
            y64_wo = alpha * (x.double() @ wv.t()) + bias.double()
            y64_dyn = alpha * (apts.double() if with_pts else 1.0) * (xv @ wv.t()) + bias.double()
            err = rel_l2(y_ref, y64_wo)
            assert err <= 4e-3, f"N{N} K{K} pts={with_pts}: rel_l2(y_ref, y64_wo) = {err}"
            rec = dict(w=bits(w), x=bits(x), bias=bits(bias), qdata=plain.qdata.numpy(),
                       scales_rowmajor=u8(plain._scale_e4m3).reshape(N, K // 16),
                       scales_swizzled=u8(swz._scale_e4m3).reshape(-1),
                       w_hat=bits(plain.to_dtype(torch.bfloat16)), xq_codes=xt.qdata.numpy(),
                       x_scales=u8(xt._scale_e4m3).reshape(M, K // 16), x_dq=bits(xv),
                       y_ref=bits(y_ref), y64_wo=y64_wo.numpy(), y64_dyn=y64_dyn.numpy(),
                       seed=np.int64(seed))
            if with_pts:
                rec.update(per_tensor_scale=pts.numpy(), act_per_tensor_scale=apts.numpy())
            name = f"nvfp4_N{N}_K{K}" + ("_pts" if with_pts else "")
            np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
            print(f"{name}: seed {seed}, rel_l2(y_ref, y64_wo) {err:.2e}, "
                  f"rel_l2(y64_dyn, y64_wo) {rel_l2(y64_dyn, y64_wo):.2e}")

    x = edge_input(7100)
    edges = {"x": bits(x)}
    for tag, pts in (("", None), ("_pts", per_tensor_amax_to_scale(x.abs().max()))):
        plain, swz = quantized(x, pts)
        edges.update({f"qdata{tag}": plain.qdata.numpy(),
                      f"scales_rowmajor{tag}": u8(plain._scale_e4m3).reshape(16, 8),
                      f"scales_swizzled{tag}": u8(swz._scale_e4m3).reshape(-1),
                      f"x_dq{tag}": bits(grid_values(plain.qdata, plain._scale_e4m3)),
                      f"w_hat{tag}": bits(plain.to_dtype(torch.bfloat16))})
        if pts is not None:
            edges["per_tensor_scale"] = pts.numpy()
        s = u8(plain._scale_e4m3).reshape(16, 8)
        assert (plain.qdata[0] == 0).all() and (plain.qdata[7, :8] == 0x88).all()
        print(f"nvfp4_quant_edges{tag}: scale bytes min {s.min()} max {s.max()}")
    np.savez_compressed(os.path.join(OUT, "nvfp4_quant_edges.npz"), **edges)

    N, K, seed = 32, 64, 9100
    torch.manual_seed(seed)
    m = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    w = m.weight.detach().clone()
    quantize_(m, NVFP4InferenceConfig(mm_config=NVFP4MMConfig.WEIGHT_ONLY, use_triton_kernel=False))
    sd = m.state_dict()
    path = os.path.join(OUT, f"nvfp4_refckpt_N{N}_K{K}.pt")
    torch.save(sd, path)
    back = torch.load(path, weights_only=True)
    t = sd["weight"]
    assert torch.equal(back["weight"].qdata, t.qdata) and t._is_swizzled_scales
    np.savez_compressed(os.path.join(OUT, f"nvfp4_refckpt_N{N}_K{K}.npz"), w=bits(w),
                        bias=bits(sd["bias"]), qdata=t.qdata.numpy(),
                        scales_swizzled=u8(t._scale_e4m3).reshape(-1),
                        w_hat=bits(t.to_dtype(torch.bfloat16)), seed=np.int64(seed))
    print(f"nvfp4_refckpt_N{N}_K{K}: seed {seed}")


if __name__ == "__main__":
    sys.exit(main())
