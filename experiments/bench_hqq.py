"""Time and quality of the fused HQQ int4 quantizer (csrc/hqq.hip) on one GPU, at g = 32:

  hqq_op        torch.ops.torchao.int4_hqq_quantize_pack (three launches, no host copy)
  hqq_torch     _choose_qparams_and_quantize_affine_hqq on the GPU in plain torch ops (fp32) +
                torchao::int4_pack: what a user has without the op (a device-to-host copy in
                every iteration)
  plain_op      torch.ops.torchao.int4_quantize_pack, the tinygemm quantizer (one launch)

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 on Gaussian * 0.02 bf16 weights. Each line
also reports, for the op's HQQ result and the plain quantizer's: the mean |W - W^| and the rel-L2
of x @ W^^T against x @ W^T (x Gaussian [64, K], products in fp32), the iterations the op ran, and
the share of groups whose codes or zero differ between the op and the plain-torch function.

Method: wall clock around `reps` back-to-back calls ending in a device synchronise, the three paths
in alternation for `rounds` rounds; per path the median over rounds and the spread
(max - min) / median. Nothing here is a threshold.

One JSON line per shape to --out (default profiles/hqq_bench.jsonl).
python experiments/bench_hqq.py [--out FILE] [--rounds N] [--shapes I,J]
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "torchao-fork_amd")]
import torch  # noqa: E402

import torchao  # noqa: E402,F401
from torchao.quantization.quant_primitives import (  # noqa: E402
    _choose_qparams_and_quantize_affine_hqq,
)

T = torch.ops.torchao
SHAPES = [(4096, 4096), (6144, 4096), (14336, 4096), (4096, 14336)]
G = 32


def dequant(packed, sz):
    N, K = packed.shape[0], packed.shape[1] * 8
    q = T.int4_unpack(packed).float().reshape(N, K // G, G)
    s, z = sz[..., 0].float()[..., None], sz[..., 1].float()[..., None]
    return ((q - 8) * s + z).reshape(N, K)


def quality(w, x, packed, sz):
    wf, d = w.float(), dequant(packed, sz)
    ref = x @ wf.t()
    return {"mean_abs_err": float((wf - d).abs().mean()),
            "product_rel_l2": float((x @ d.t() - ref).norm() / ref.norm())}


def bench_shape(N, K, rounds, emit):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
    x = torch.randn(64, K, generator=gen, device=dev)

    def hqq_op():
        return T.int4_hqq_quantize_pack(w, G)

    def hqq_torch():
        q, s, z, _ = _choose_qparams_and_quantize_affine_hqq(
            w, nbits=4, group_size=G, axis=1, compute_dtype=torch.bfloat16, device=dev)
        return T.int4_pack(q.to(torch.int32)), torch.stack(
            [s.reshape(N, K // G), z.reshape(N, K // G)], -1)

    def plain_op():
        return T.int4_quantize_pack(w, G, 1e-6)

    paths = {"hqq_op": (hqq_op, 10), "hqq_torch": (hqq_torch, 1), "plain_op": (plain_op, 20)}
    res = {name: fn() for name, (fn, _) in paths.items()}
    ms = {name: [] for name in paths}
    for _ in range(rounds):
        for name, (fn, reps) in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    med = {n: statistics.median(v) for n, v in ms.items()}
    po, so, it = res["hqq_op"]
    pt, st = res["hqq_torch"]
    moved = ((po != pt).reshape(N, K // G, G // 8).any(-1)
             | (so.view(torch.int16) != st.view(torch.int16)).any(-1))
    emit({"N": N, "K": K, "g": G, "rounds": rounds,
          "ms": {n: round(v, 4) for n, v in med.items()},
          "spread": {n: round((max(v) - min(v)) / med[n], 4) for n, v in ms.items()},
          "hqq_torch_over_hqq_op": round(med["hqq_torch"] / med["hqq_op"], 2),
          "hqq_op_over_plain_op": round(med["hqq_op"] / med["plain_op"], 2),
          "iters": int(it.item()),
          "hqq": quality(w, x, po, so), "hqq_torch_quality": quality(w, x, pt, st),
          "plain": quality(w, x, *res["plain_op"]),
          "groups_differing_op_vs_torch": float(moved.float().mean()),
          "device": torch.cuda.get_device_name(0)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hqq_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hqq.py measures on the GPU; no device found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for i in (int(v) for v in args.shapes.split(",") if v != ""):
            bench_shape(*SHAPES[i], args.rounds, emit)


if __name__ == "__main__":
    main()
