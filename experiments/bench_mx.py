"""Per-launch time of the MXFP8 linear against the per-row float8 dynamic linear (the same tile
structure with unit block scales), in one process on one GPU:

  mx_dyn       torch.ops.torchao.mx_dyn_linear     the whole linear from a bf16 activation
                                                   (M = 1: one launch; else quantizer + scaled mm)
  mx_mm        torch.ops.torchao.mx_scaled_mm      the product alone, on ready-made codes
  mx_mm_mfma   the same with the MFMA route forced (gemm_mfma_kernel<MxFp8>)
  mx_quant     torch.ops.torchao.mx_quantize_rows  the block quantizer alone (no row-wide reduction)
  fp8_dyn, fp8_mm, fp8_mm_mfma, fp8_quant           the float8 ops on same-shape operands

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 16, 128, 512.

Method (as experiments/bench_fp8wo.py): each path's launches over weight copies rotated past the
Infinity Cache are captured in one HIP graph (back to back, no host gaps) and timed by the wall
clock around `reps` replays ending in a device synchronise. The graphs are timed in alternation
for `rounds` rounds, so drift of a shared machine lands on all of them; per path the median over
rounds and the spread (max - min) / median are reported.

One JSON line per (shape, M) to --out (default profiles/mx_bench.jsonl).
python experiments/bench_mx.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,128]
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
    mq, msc, fq, fs = [], [], [], []
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        q, s = T.mx_quantize_rows(w)
        mq.append(q)
        msc.append(s)
        q, s = T.fp8_quantize_rows(w)
        fq.append(q)
        fs.append(s.reshape(-1).contiguous())
        del w
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        xq, xs = T.mx_quantize_rows(x)
        xq8, xs8 = T.fp8_quantize_rows(x)
        xs8 = xs8.reshape(-1).contiguous()
        paths = {
            "mx_dyn": (lambda i: T.mx_dyn_linear(x, mq[i], msc[i], None), {}),
            "mx_mm": (lambda i: T.mx_scaled_mm(xq, xs, mq[i], msc[i], None), {}),
            "mx_mm_mfma": (lambda i: T.mx_scaled_mm(xq, xs, mq[i], msc[i], None), {"mx_mfma": 1}),
            "mx_quant": (lambda i: T.mx_quantize_rows(x), {}),
            "fp8_dyn": (lambda i: T.fp8_dyn_linear(x, fq[i], fs[i], None), {}),
            "fp8_mm": (lambda i: T.fp8_scaled_mm(xq8, xs8, fq[i], fs[i], None), {}),
            "fp8_mm_mfma": (lambda i: T.fp8_scaled_mm(xq8, xs8, fq[i], fs[i], None),
                            {"fp8dyn_mfma": 1}),
            "fp8_quant": (lambda i: T.fp8_quantize_rows(x), {}),
        }
        ref = x.double() @ (mq[0].double().reshape(N, -1, 32) * torch.exp2(
            msc[0].double() - 127)[..., None]).reshape(N, K).t()  # bf16 x, dequantised MX weight
        err, kernel = {}, {}
        for name, (fn, knobs) in paths.items():
            with tuning(**knobs):
                y = fn(0)
                kernel[name] = _lib.lib().tao_last_kernel().decode()
            if "quant" not in name:  # against the unquantised activation: the whole recipe's error
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
            "mx_mm_over_fp8_mm": round(med["mx_mm"] / med["fp8_mm"], 4),
            "mx_mfma_over_fp8_mfma": round(med["mx_mm_mfma"] / med["fp8_mm_mfma"], 4),
            "mx_dyn_over_fp8_dyn": round(med["mx_dyn"] / med["fp8_dyn"], 4),
            "mx_quant_over_fp8_quant": round(med["mx_quant"] / med["fp8_quant"], 4),
            "rel_l2_vs_bf16_x": err, "device": torch.cuda.get_device_name(0),
        })
        del graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx.py measures on the GPU; no device found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ms = [int(m) for m in args.ms.split(",")]
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for i in (int(s) for s in args.shapes.split(",")):
            bench_shape(*SHAPES[i], ms, args.rounds, emit)


if __name__ == "__main__":
    main()
