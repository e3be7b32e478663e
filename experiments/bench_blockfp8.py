"""Per-launch time of the blockwise float8 linear (1 x 128 / 128 x 128 fp32 scales) against the
per-row float8 dynamic linear and the MXFP8 linear (the same tile structure and GEMV decomposition),
and against the formulation a user has without it, in one process on one GPU:

  blk_dyn       torch.ops.torchao.blockfp8_dyn_linear  the whole linear from a bf16 activation
                                                       (M = 1: one launch; else quantizer + scaled mm)
  blk_mm        torch.ops.torchao.blockfp8_scaled_mm   the product alone, on ready-made codes
  blk_mm_mfma   the same with the MFMA route forced (gemm_mfma_kernel<BlockFp8>)
  blk_quant     torch.ops.torchao.blockfp8_quantize_act
  fp8_dyn, fp8_mm, fp8_mm_mfma      the per-row float8 ops on same-shape operands
  mx_dyn, mx_mm, mx_mm_mfma         the MXFP8 ops on same-shape operands
  deq_linear    blockfp8_dequantize_weight to bf16 once per call, then a bf16 F.linear

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 16, 128, 512.

Method (as experiments/bench_mx.py): each path's launches over weight copies rotated past the
Infinity Cache are captured in one HIP graph (back to back, no host gaps) and timed by the wall
clock around `reps` replays ending in a device synchronise. The graphs are timed in alternation
for `rounds` rounds, so drift of a shared machine lands on all of them; per path the median over
rounds and the spread (max - min) / median are reported.

One JSON line per (shape, M) to --out (default profiles/blockfp8_bench.jsonl; --append adds to it,
so that each shape can be its own process under its own time limit).
python experiments/bench_blockfp8.py [--out FILE] [--append] [--rounds N] [--shapes I,J] [--ms 1,128]
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchao-fork_amd"))
import torch  # noqa: E402

import torchao  # noqa: E402,F401
from torchao import _lib  # noqa: E402
from torchao.kernel.tuning import tuning  # noqa: E402

SHAPES = [(4096, 4096), (6144, 4096), (14336, 4096), (4096, 14336)]
MS = [1, 16, 128, 512]
ROTATE_BYTES = 1 << 30  # weight bytes per rotation: four times the 256 MiB Infinity Cache
T = torch.ops.torchao


def make_graph(fn, knobs):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), tuning(**knobs):  # launch shapes are fixed at capture
        fn()
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    return g


def time_graph(g, launches, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps / launches * 1e6


def bench_shape(N, K, ms, rounds, emit):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    copies = max(3, -(-ROTATE_BYTES // (N * K)))
    bq, bs, mq, msc, fq, fs = [], [], [], [], [], []
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        q, s = T.blockfp8_quantize_weight(w)
        bq.append(q)
        bs.append(s)
        q, s = T.mx_quantize_rows(w)
        mq.append(q)
        msc.append(s)
        q, s = T.fp8_quantize_rows(w)
        fq.append(q)
        fs.append(s.reshape(-1).contiguous())
        del w
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        xqb, xsb = T.blockfp8_quantize_act(x)
        xqm, xsm = T.mx_quantize_rows(x)
        xq8, xs8 = T.fp8_quantize_rows(x)
        xs8 = xs8.reshape(-1).contiguous()

        def deq_linear(i):
            return torch.nn.functional.linear(x, T.blockfp8_dequantize_weight(bq[i], bs[i], True))

        paths = {
            "blk_dyn": (lambda i: T.blockfp8_dyn_linear(x, bq[i], bs[i], None), {}),
            "blk_mm": (lambda i: T.blockfp8_scaled_mm(xqb, xsb, bq[i], bs[i], None), {}),
            "blk_mm_mfma": (lambda i: T.blockfp8_scaled_mm(xqb, xsb, bq[i], bs[i], None),
                            {"blockfp8_mfma": 1}),
            "blk_quant": (lambda i: T.blockfp8_quantize_act(x), {}),
            "fp8_dyn": (lambda i: T.fp8_dyn_linear(x, fq[i], fs[i], None), {}),
            "fp8_mm": (lambda i: T.fp8_scaled_mm(xq8, xs8, fq[i], fs[i], None), {}),
            "fp8_mm_mfma": (lambda i: T.fp8_scaled_mm(xq8, xs8, fq[i], fs[i], None),
                            {"fp8dyn_mfma": 1}),
            "mx_dyn": (lambda i: T.mx_dyn_linear(x, mq[i], msc[i], None), {}),
            "mx_mm": (lambda i: T.mx_scaled_mm(xqm, xsm, mq[i], msc[i], None), {}),
            "mx_mm_mfma": (lambda i: T.mx_scaled_mm(xqm, xsm, mq[i], msc[i], None), {"mx_mfma": 1}),
            "deq_linear": (deq_linear, {}),
        }
        # bf16 x against the dequantised blockwise weight: the activation quantisation's error
        ref = x.double() @ T.blockfp8_dequantize_weight(bq[0], bs[0], False).double().t()
        err, kernel = {}, {}
        for name, (fn, knobs) in paths.items():
            with tuning(**knobs):
                y = fn(0)
                kernel[name] = _lib.lib().tao_last_kernel().decode()
            if name.startswith("blk") and "quant" not in name or name == "deq_linear":
                err[name] = float(f"{float((y.double() - ref).norm() / ref.norm()):.3e}")
        del ref
        launches = copies * max(1, 48 // copies)
        graphs = {name: make_graph(lambda fn=fn: [fn(i % copies) for i in range(launches)], knobs)
                  for name, (fn, knobs) in paths.items()}
        reps = {name: max(3, int(0.08 / (time_graph(g, launches, 3) * launches * 1e-6)))
                for name, g in graphs.items()}
        us = {name: [] for name in paths}
        for _ in range(rounds):
            for name, g in graphs.items():
                us[name].append(time_graph(g, launches, reps[name]))
        med = {n: statistics.median(v) for n, v in us.items()}
        emit({
            "M": M, "N": N, "K": K, "copies": copies, "launches_per_graph": launches,
            "rounds": rounds, "kernel": kernel,
            "us": {n: round(v, 3) for n, v in med.items()},
            "us_min": {n: round(min(v), 3) for n, v in us.items()},
            "spread": {n: round((max(v) - min(v)) / med[n], 4) for n, v in us.items()},
            "blk_mm_over_fp8_mm": round(med["blk_mm"] / med["fp8_mm"], 4),
            "blk_mm_over_mx_mm": round(med["blk_mm"] / med["mx_mm"], 4),
            "blk_mfma_over_fp8_mfma": round(med["blk_mm_mfma"] / med["fp8_mm_mfma"], 4),
            "blk_mfma_over_mx_mfma": round(med["blk_mm_mfma"] / med["mx_mm_mfma"], 4),
            "blk_dyn_over_fp8_dyn": round(med["blk_dyn"] / med["fp8_dyn"], 4),
            "deq_linear_over_blk_dyn": round(med["deq_linear"] / med["blk_dyn"], 4),
            "rel_l2_vs_bf16_x": err, "device": torch.cuda.get_device_name(0),
        })
        del graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blockfp8_bench.jsonl"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_blockfp8.py measures on the GPU; no device found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ms = [int(m) for m in args.ms.split(",")]
    with open(args.out, "a" if args.append else "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for i in (int(s) for s in args.shapes.split(",")):
            bench_shape(*SHAPES[i], ms, args.rounds, emit)


if __name__ == "__main__":
    main()
