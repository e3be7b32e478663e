"""Per-launch time of the MXFP4-weight linear (e4m3fn activations x e2m1 weights) against the MXFP8
linear and the int4 g32 weight-only linear on same-shape operands, in one process on one GPU:

  fp4_dyn      torch.ops.torchao.mxfp4w_dyn_linear  the whole linear from a bf16 activation
                                                    (M = 1: one launch; else quantizer + scaled mm)
  fp4_mm       torch.ops.torchao.mxfp4w_scaled_mm   the product alone, on ready-made codes
  fp4_mm_mfma  the same with the MFMA route forced (gemm_mfma_kernel<MxFp8Fp4>)
  mx_dyn, mx_mm, mx_mm_mfma                         the MXFP8 ops
  int4         torch.ops.torchao.int4_weight_only_linear, group size 32 (bf16 activation)

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 16, 128, 512.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 1 GiB of the smallest format's bytes per rotation) are captured in one HIP
graph and timed by the wall clock around `reps` replays ending in a device synchronise. The graphs
are timed in alternation for `rounds` rounds; per path the median over rounds and the spread
(max - min) / median are reported.

Required (`gate_m1`): at M = 1 the fp4 scaled mm's median is no larger than the MXFP8 one's plus
that run's measured spread (the larger of the two paths' spreads, times the MXFP8 median).

Accuracy on Gaussian data: relative L2 of each path against bf16 x times the path's own dequantised
weight (the activation's quantisation alone) and against bf16 x times the unquantised weight (the
whole recipe).

One JSON line per (shape, M) to --out (default profiles/mxfp4_bench.jsonl).
python experiments/bench_mxfp4.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,128]
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "torchao-fork_amd"), os.path.join(ROOT, "experiments")]
import torch  # noqa: E402

import torchao  # noqa: E402,F401
from bench_mx import MS, ROTATE_BYTES, SHAPES, make_graph, time_graph  # noqa: E402
from torchao import _lib  # noqa: E402
from torchao.kernel.tuning import tuning  # noqa: E402
from torchao.prototype.mx_formats.mx_tensor import to_dtype  # noqa: E402

T = torch.ops.torchao
E8 = torch.float8_e8m0fnu
F4 = torch.float4_e2m1fn_x2


def bench_shape(N, K, ms, rounds, emit):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    copies = max(3, -(-ROTATE_BYTES // (N * K // 2)))
    q4, s4, q8, s8, qi, zi = [], [], [], [], [], []
    w0 = None
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        q, s = T.mxfp4_quantize_rows(w)
        q4.append(q)
        s4.append(s)
        q, s = T.mx_quantize_rows(w)
        q8.append(q)
        s8.append(s)
        p, sz = T.int4_quantize_pack(w, 32, 1e-6)
        qi.append(p)
        zi.append(sz)
        if w0 is None:
            w0 = w.double()
        del w
    deq = {"fp4": to_dtype(q4[0], s4[0].view(E8), F4, 32, torch.float32).double(),
           "mx": to_dtype(q8[0], s8[0].view(E8), torch.float8_e4m3fn, 32, torch.float32).double()}
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        xq, xs = T.mx_quantize_rows(x)
        paths = {
            "fp4_dyn": (lambda i: T.mxfp4w_dyn_linear(x, q4[i], s4[i], None), {}),
            "fp4_mm": (lambda i: T.mxfp4w_scaled_mm(xq, xs, q4[i], s4[i], None), {}),
            "fp4_mm_mfma": (lambda i: T.mxfp4w_scaled_mm(xq, xs, q4[i], s4[i], None),
                            {"mx_mfma": 1}),
            "mx_dyn": (lambda i: T.mx_dyn_linear(x, q8[i], s8[i], None), {}),
            "mx_mm": (lambda i: T.mx_scaled_mm(xq, xs, q8[i], s8[i], None), {}),
            "mx_mm_mfma": (lambda i: T.mx_scaled_mm(xq, xs, q8[i], s8[i], None), {"mx_mfma": 1}),
            "int4": (lambda i: T.int4_weight_only_linear(x, qi[i], zi[i], 32, None), {}),
        }
        full = x.double() @ w0.t()
        err_act, err_full, kernel = {}, {}, {}
        for name, (fn, knobs) in paths.items():
            with tuning(**knobs):
                y = fn(0).double()
                kernel[name] = _lib.lib().tao_last_kernel().decode()
            err_full[name] = float(f"{float((y - full).norm() / full.norm()):.3e}")
            if name != "int4":
                ref = x.double() @ deq[name.split("_")[0]].t()
                err_act[name] = float(f"{float((y - ref).norm() / ref.norm()):.3e}")
        del full
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
        spread = {n: (max(v) - min(v)) / med[n] for n, v in us.items()}
        rec = {
            "M": M, "N": N, "K": K, "copies": copies, "launches_per_graph": launches,
            "rounds": rounds, "kernel": kernel,
            "us": {n: round(v, 3) for n, v in med.items()},
            "us_min": {n: round(min(v), 3) for n, v in us.items()},
            "spread": {n: round(v, 4) for n, v in spread.items()},
            "fp4_mm_over_mx_mm": round(med["fp4_mm"] / med["mx_mm"], 4),
            "fp4_mfma_over_mx_mfma": round(med["fp4_mm_mfma"] / med["mx_mm_mfma"], 4),
            "fp4_dyn_over_mx_dyn": round(med["fp4_dyn"] / med["mx_dyn"], 4),
            "fp4_mm_over_int4": round(med["fp4_mm"] / med["int4"], 4),
            "rel_l2_vs_bf16_x_own_weight": err_act, "rel_l2_vs_unquantised": err_full,
            "device": torch.cuda.get_device_name(0),
        }
        if M == 1:
            rec["gate_m1"] = bool(med["fp4_mm"] <= med["mx_mm"] * (
                1 + max(spread["fp4_mm"], spread["mx_mm"])))
        emit(rec)
        del graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mxfp4.py measures on the GPU; no device found")
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
