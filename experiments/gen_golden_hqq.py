"""Generate the HQQ fixtures under tests/golden/ by running the REFERENCE torchao on the CPU
(Int4WeightOnlyConfig(group_size=g, layout=Int4CPULayout(), use_hqq=True, version=1): fp32
arithmetic, the path this package serves on every device).

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_hqq.py

Only data is written; bf16 tensors are stored as their uint16 bit patterns.

  hqq_N64_K256_g32.npz, hqq_N96_K1024_g64.npz, hqq_N48_K512_g128.npz, hqq_N40_K2048_g256.npz
      w                bf16 bits [N, K]: Gaussian * 0.03 with 1 % of the entries six times larger
      q, s, z          the reference's codes [N, K] (uint8) and bf16 bits [N, K/g] of the scales
                       and zeros of quantize_(use_hqq=True) (get_plain()): w ~= (q - 8) s + z
                       (N = 40 is no multiple of the CPU layout's 16 rows: there the handler's
                       to_affine_quantized_intx call is made with PlainLayout)
      errors, iters    the error e_i of every iteration the reference ran (its own verbose
                       output, parsed back: repr round-trips a double) and their count
      q_plain, s_plain, z_plain   the same of quantize_(use_hqq=False), the tinygemm quantizer
      mean_err_hqq, mean_err_plain   mean |W - W^| of both, in float64 on the stored values
      moved_model      the largest share of groups whose codes or bf16 zero differ from the
                       reference's, over 8 seeded runs of the same iteration in which every new
                       zero is moved by one fp32 ulp (random sign): how far an implementation
                       with its own pow and summation order may drift. moved_codes_model /
                       moved_runs are the largest share of changed codes and every run's share.
  hqq_N40_K352_g32.npz
      the same record for a shape of 1760 eight-weight pieces, no multiple of a 256-thread
      workgroup, under the same conditions (the weight of int4_N40_K352_g32.npz reaches a fixed
      point, e_12 == e_11 exactly, so it cannot pin the stop index; seed 7 is the first of the
      recipe whose comparisons all keep the margin).
  hqq_quant_edges.npz
      w [5, 64] bf16 bits, g = 32: the first group of each row is a constant group (max == min:
      the 2e4 clamp), an all-zero group, a group with a range under 15 / 2e4, one huge outlier
      among tiny values, and weights that put w * scale + zero exactly on .5 in the first
      iteration; the second group is Gaussian. q, s, z, errors, iters of the reference's
      _choose_qparams_and_quantize_affine_hqq(device="cpu", compute_dtype=bfloat16).

Conditions asserted on the inputs (they pin the stop index; not tolerances):
  every comparison the stop rule makes, up to and including the stopping one, differs by at least
  3e-5 relative (fp32 summation noise is about 1e-6); HQQ's mean |W - W^| is below plain's.
"""

import contextlib
import io
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
CASES = [(64, 256, 32, 9), (96, 1024, 64, 196), (48, 512, 128, 1), (40, 2048, 256, 0)]
EXPECT_ITERS = {32: 11, 64: 16, 128: 20, 256: 20}  # the first two stop at i = 10 and i = 15
TAIL = (40, 352, 32, 7)
MARGIN = 3e-5
RUNS = 8


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def make_weight(N, K, seed):
    gen = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=gen)
    m = torch.rand(N, K, generator=gen) < 0.01
    return (torch.where(m, 6 * W, W) * 0.03).bfloat16()


def check_margin(errors, tag):
    """Every comparison e_i < best the loop made is at least MARGIN away from equality."""
    best = 1e4
    for i, e in enumerate(errors):
        rel = abs(e - best) / max(e, best)
        assert rel >= MARGIN, (tag, i, e, best, rel)
        if e < best:
            best = e
        else:
            assert i == len(errors) - 1, (tag, i)


def traced_hqq(qp, w, g):
    """The reference's function with verbose=True; its printed errors parsed back."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        q, s, z, _ = qp._choose_qparams_and_quantize_affine_hqq(
            w, nbits=4, group_size=g, axis=1, compute_dtype=torch.bfloat16, device="cpu",
            verbose=True)
    errors = [float(line.split("Error:")[1]) for line in buf.getvalue().splitlines()
              if "Error:" in line]
    return q, s, z, errors


def perturbed_run(qp, w, g, seed):
    """The reference's arithmetic restated over its own _shrink_lp_op, every new zero moved by
    one fp32 ulp with a random sign (seed < 0: not moved, which must give the reference's bits)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    W = w.float().reshape(-1, g)
    mn, mx = W.min(1, keepdim=True)[0], W.max(1, keepdim=True)[0]
    scale = (15 / (mx - mn)).clamp(max=2e4)
    zero = torch.round(-mn * scale)
    beta, best = 1e1, 1e4
    for _ in range(20):
        Wq = torch.round(W * scale + zero).clamp(0, 15)
        Wr = (Wq - zero) / scale
        We = qp._shrink_lp_op(W - Wr, beta, 0.7)
        zero = torch.mean(Wq - (W - We) * scale, axis=1, keepdim=True)
        if seed >= 0:
            up = torch.rand(zero.shape, generator=gen) < 0.5
            inf = torch.full_like(zero, float("inf"))
            zero = torch.nextafter(zero, torch.where(up, inf, -inf))
        beta *= 1.01
        e = float(torch.abs(W - Wr).mean())
        if e < best:
            best = e
        else:
            break
    q = torch.round(W * scale + zero).clamp(0, 15).to(torch.uint8).reshape(w.shape)
    inv = 1.0 / scale
    return q, inv.bfloat16(), ((8 - zero) * inv).bfloat16()


def mean_err(w, q, s, z, g):
    N, K = w.shape
    deq = (q.double().reshape(N, K // g, g) - 8) * s.double().reshape(N, K // g, 1) \
        + z.double().reshape(N, K // g, 1)
    return float((w.double() - deq.reshape(N, K)).abs().mean())


def edge_rows():
    gen = torch.Generator().manual_seed(77)
    w = torch.randn(5, 64, generator=gen) * 0.03
    w[0, :32] = 0.0625                                    # constant: max == min
    w[1, :32] = 0.0                                       # all zero
    base = torch.tensor(0.01).bfloat16().float()          # range of 3 bf16 ulps < 15 / 2e4
    w[2, :32] = base + torch.randint(0, 4, (32,), generator=gen) * 2.0 ** -14
    w[3, :32] = torch.randn(32, generator=gen) * 1e-4     # one huge outlier among tiny values
    w[3, 5] = 8.0
    half = torch.arange(15) + 0.5                         # min 0, max 15: scale 1, zero 0
    w[4, :32] = torch.cat([torch.tensor([0.0, 15.0]), half, torch.arange(1, 16).float()])
    wb = w.bfloat16()
    assert torch.equal(wb[4, :32].float(), w[4, :32]) and torch.equal(wb[2].float()[:32], w[2, :32])
    return wb


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH"
    )
    from torchao.dtypes import Int4CPULayout, PlainLayout, to_affine_quantized_intx
    from torchao.quantization.quant_primitives import MappingType, ZeroPointDomain
    from torchao.quantization import Int4WeightOnlyConfig, quantize_
    from torchao.quantization import quant_primitives as qp

    os.makedirs(OUT, exist_ok=True)
    for N, K, g, seed in CASES + [TAIL]:
        w = make_weight(N, K, seed)
        plain = {}
        for hqq in (True, False):
            lin = torch.nn.Linear(K, N, bias=False, dtype=torch.bfloat16)
            with torch.no_grad():
                lin.weight.copy_(w)
            if N % 16 == 0:
                quantize_(lin, Int4WeightOnlyConfig(group_size=g, layout=Int4CPULayout(),
                                                    use_hqq=hqq, version=1))
                q, s, z = lin.weight.tensor_impl.get_plain()
            else:
                # the CPU layout packs 16 rows at a time: the same call its handler makes, with
                # the plain layout (quant_api.py:1126-1139)
                q, s, z = to_affine_quantized_intx(
                    w, MappingType.ASYMMETRIC, (1, g), torch.int32, 0, 15, 1e-6,
                    zero_point_dtype=torch.bfloat16, preserve_zero=False,
                    zero_point_domain=ZeroPointDomain.FLOAT, _layout=PlainLayout(),
                    use_hqq=hqq).tensor_impl.get_plain()
            assert tuple(q.shape) == (N, K) and s.dtype == torch.bfloat16
            plain[hqq] = (q.to(torch.uint8), s.reshape(N, K // g), z.reshape(N, K // g))
        q, s, z = plain[True]
        # the function itself gives quantize_'s result, and the error trajectory
        q2, s2, z2, errors = traced_hqq(qp, w, g)
        assert torch.equal(q2, q) and torch.equal(s2.reshape(s.shape), s)
        assert torch.equal(z2.reshape(z.shape), z)
        check_margin(errors, (N, K, g))
        assert (N, K, g, seed) == TAIL or len(errors) == EXPECT_ITERS[g], (g, len(errors))
        q0, s0, z0 = perturbed_run(qp, w, g, -1)
        assert torch.equal(q0, q) and torch.equal(s0.reshape(s.shape), s)
        assert torch.equal(z0.reshape(z.shape), z), "the restated loop must give the reference's bits"
        e_hqq, e_plain = mean_err(w, q, s, z, g), mean_err(w, *plain[False], g)
        assert e_hqq < e_plain, (e_hqq, e_plain)
        moved, moved_codes = [], []
        for r in range(RUNS):
            qr, sr, zr = perturbed_run(qp, w, g, r)
            assert torch.equal(sr.reshape(s.shape), s)
            dq = (qr != q).reshape(N, K // g, g)
            dz = bf16_bits(zr.reshape(z.shape)) != bf16_bits(z)
            assert int((qr.int() - q.int()).abs().max()) <= 1
            moved.append(float((dq.any(-1).numpy() | dz).mean()))
            moved_codes.append(float(dq.float().mean()))
        np.savez_compressed(
            os.path.join(OUT, f"hqq_N{N}_K{K}_g{g}.npz"), N=N, K=K, g=g, seed=seed,
            w=bf16_bits(w), q=q.numpy(), s=bf16_bits(s), z=bf16_bits(z),
            errors=np.asarray(errors, dtype=np.float64), iters=len(errors),
            q_plain=plain[False][0].numpy(), s_plain=bf16_bits(plain[False][1]),
            z_plain=bf16_bits(plain[False][2]), mean_err_hqq=e_hqq, mean_err_plain=e_plain,
            moved_model=max(moved), moved_codes_model=max(moved_codes),
            moved_runs=np.asarray(moved, dtype=np.float64))
        print(N, K, g, "iters", len(errors), "mean err hqq/plain", e_hqq, e_plain,
              "moved_model", max(moved), "codes", max(moved_codes))

    w = edge_rows()
    q, s, z, errors = traced_hqq(qp, w, 32)
    check_margin(errors, "edges")
    assert bool(torch.isfinite(s.float()).all()) and bool(torch.isfinite(z.float()).all())
    np.savez_compressed(
        os.path.join(OUT, "hqq_quant_edges.npz"), g=32, w=bf16_bits(w), q=q.numpy(),
        s=bf16_bits(s.reshape(5, 2)), z=bf16_bits(z.reshape(5, 2)),
        errors=np.asarray(errors, dtype=np.float64), iters=len(errors))
    print("edges iters", len(errors), "scales", s.reshape(5, 2)[:, 0].tolist())


if __name__ == "__main__":
    main()
