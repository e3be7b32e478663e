"""Per-linear time of the W4A8 linear (int8 dynamic activations x packed int4 weights, csrc/w4a8.hip)
against the two formats it sits between, in one process on one GPU:

  w4a8_mm    torch.ops.torchao.rowwise_scaled_linear_cutlass_s8s4 on codes quantized beforehand
  w4a8_dyn   torch.ops.torchao.w4a8_dyn_linear, the whole linear from a bf16 activation (M = 1: one
             launch; else the per-token quantizer, then the scaled mm)
  int8_mm    torch.ops.torchao.int8_scaled_mm on codes quantized beforehand
  int8_dyn   int8_dyn_linear at M = 1, int8_quantize_per_token + int8_scaled_mm above
  int4wo     torch.ops.torchao.int4_weight_only_linear, group size 32 (bf16 activations)

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 4, 16, 128, 512.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 512 MiB of packed int4 weights per rotation, i.e. 1 GiB of int8 ones; the
same number of copies for every format) are captured in one HIP graph and timed by the wall clock
around `reps` replays ending in a device synchronise. The graphs are timed in alternation for
`rounds` rounds; per path the median over rounds and the spread (max - min) / median are reported.
w4a8_dyn is compared bit for bit with the quantizer followed by w4a8_mm before timing.

Nothing here is a threshold. The expectation to confirm or refute: at M = 1 w4a8 at or below
int4wo and well below int8; at M >= 128 w4a8_mm near int8_mm and below int4wo.

One JSON line per (shape, M) to --out (default profiles/w4a8_bench.jsonl).
python experiments/bench_w4a8.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,16]

--boundary (with --ms 1,2,3,4): only the scaled mm, forced onto the GEMV and onto the MFMA kernel
through tao_tune_linear_crossover, and as routed: the measurement behind the route's boundary
(profiles/w4a8_bench_boundary.jsonl).
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
from bench_mx import SHAPES, make_graph, time_graph  # noqa: E402
from torchao import _lib  # noqa: E402
from torchao.kernel import tuning  # noqa: E402

T = torch.ops.torchao
MS = [1, 4, 16, 128, 512]
ROTATE_BYTES = 1 << 29  # packed int4 weight bytes per rotation: twice the 256 MiB Infinity Cache


def bench_shape(N, K, ms, rounds, emit, boundary=False):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    copies = max(3, -(-ROTATE_BYTES // (N * K // 2)))
    w4, w4s, w8, w8s, wg, wgs = [], [], [], [], [], []
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        q, s = T.int4_quantize_rows_packed(w)
        w4.append(q)
        w4s.append(s)
        q, s = T.int8_quantize_rows(w, 1e-5)
        w8.append(q)
        w8s.append(s.reshape(-1).contiguous())
        q, s = T.int4_quantize_pack(w, 32, 1e-6)
        wg.append(q)
        wgs.append(s)
        del w
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        xq4, xs4 = T.int8_quantize_per_token_f32(x)
        xq8, xs8 = T.int8_quantize_per_token(x)

        def int8_dyn(i):
            if M == 1:
                return T.int8_dyn_linear(x, w8[i], w8s[i], None)
            q, sc = T.int8_quantize_per_token(x)
            return T.int8_scaled_mm(q, sc, w8[i], w8s[i], None)

        paths = {
            "w4a8_mm": lambda i: T.rowwise_scaled_linear_cutlass_s8s4(xq4, xs4, w4[i], w4s[i], None,
                                                                      None),
            "w4a8_dyn": lambda i: T.w4a8_dyn_linear(x, w4[i], w4s[i], None),
            "int8_mm": lambda i: T.int8_scaled_mm(xq8, xs8, w8[i], w8s[i], None),
            "int8_dyn": int8_dyn,
            "int4wo": lambda i: T.int4_weight_only_linear(x, wg[i], wgs[i], 32, None),
        }
        knobs = {name: {} for name in paths}
        if boundary:  # the scaled mm on both routes, whatever the built-in boundary
            paths = {"w4a8_mm_gemv": paths["w4a8_mm"], "w4a8_mm_mfma": paths["w4a8_mm"],
                     "w4a8_mm": paths["w4a8_mm"]}
            knobs = {"w4a8_mm_gemv": {"linear_crossover": 4}, "w4a8_mm_mfma": {"linear_crossover": 1},
                     "w4a8_mm": {}}
        kernel = {}
        for name, fn in paths.items():
            with tuning(**knobs[name]):
                fn(0)
            kernel[name] = _lib.lib().tao_last_kernel().decode()
        launches = copies * max(1, 48 // copies)
        graphs = {name: make_graph(lambda fn=fn: [fn(i % copies) for i in range(launches)],
                                   knobs[name])
                  for name, fn in paths.items()}
        reps = {name: max(3, int(0.08 / (time_graph(g, launches, 3) * launches * 1e-6)))
                for name, g in graphs.items()}
        us = {name: [] for name in paths}
        for _ in range(rounds):
            for name, g in graphs.items():
                us[name].append(time_graph(g, launches, reps[name]))
        med = {n: statistics.median(v) for n, v in us.items()}
        rec = {
            "M": M, "N": N, "K": K, "copies": copies, "launches_per_graph": launches,
            "rounds": rounds, "kernel": kernel,
            "us": {n: round(v, 3) for n, v in med.items()},
            "us_min": {n: round(min(v), 3) for n, v in us.items()},
            "spread": {n: round((max(v) - min(v)) / med[n], 4) for n, v in us.items()},
            "device": torch.cuda.get_device_name(0),
        }
        if boundary:
            rec["gemv_over_mfma"] = round(med["w4a8_mm_gemv"] / med["w4a8_mm_mfma"], 4)
            emit(rec)
            del graphs
            torch.cuda.empty_cache()
            continue
        same = bool(torch.equal(paths["w4a8_dyn"](0), paths["w4a8_mm"](0)))
        rec.update({
            "w4a8_mm_over_int8_mm": round(med["w4a8_mm"] / med["int8_mm"], 4),
            "w4a8_dyn_over_int8_dyn": round(med["w4a8_dyn"] / med["int8_dyn"], 4),
            "w4a8_dyn_over_int4wo": round(med["w4a8_dyn"] / med["int4wo"], 4),
            "w4a8_mm_over_int4wo": round(med["w4a8_mm"] / med["int4wo"], 4),
            "dyn_bit_equal_to_quantize_then_mm": same,
        })
        emit(rec)
        del graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w4a8_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    ap.add_argument("--boundary", action="store_true",
                    help="time the scaled mm on the GEMV and on the MFMA route at each M (<= 4)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_w4a8.py measures on the GPU; no device found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ms = [int(m) for m in args.ms.split(",")]
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for i in (int(v) for v in args.shapes.split(",") if v != ""):
            bench_shape(*SHAPES[i], ms, args.rounds, emit, args.boundary)


if __name__ == "__main__":
    main()
