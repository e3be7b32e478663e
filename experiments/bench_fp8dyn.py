"""Per-launch time of the float8 dynamic-activation x float8-weight linear and its comparators, in
one process on one GPU:

  dyn       torch.ops.torchao.fp8_dyn_linear       the whole linear from a bf16 activation
                                                   (M = 1: one launch; else quantizer + scaled mm)
  mm        torch.ops.torchao.fp8_scaled_mm        the product alone, on ready-made codes
  mm_gemv   the same with the crossover forced up  (M <= 8: fp8dyn_gemv_kernel)
  mm_mfma   the same with the MFMA route forced    (gemm_mfma_kernel<Fp8Dyn>)
  quant     torch.ops.torchao.fp8_quantize_rows    the activation quantizer alone
  fp8wo     torch.ops.torchao.fp8_weight_only_linear on the same weight codes (multiplies in bf16)
  int8dyn   int8_dyn_linear (M = 1) / int8_quantize_per_token + int8_scaled_mm on the same shape
  vendor    torch._scaled_mm with row-wise scales, where this build runs it

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 2, 4, 8, 16, 128, 512.

Method (as experiments/bench_fp8wo.py): each path's launches over weight copies rotated past the
Infinity Cache are captured in one HIP graph (back to back, no host gaps) and timed by the wall
clock around `reps` replays ending in a device synchronise. The graphs are timed in alternation
for `rounds` rounds, so drift of a shared machine lands on all of them; per path the median over
rounds and the spread (max - min) / median are reported.

One JSON line per (shape, M) to --out (default profiles/fp8dyn_bench.jsonl).
python experiments/bench_fp8dyn.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,128]
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

FP8 = torch.float8_e4m3fn
SHAPES = [(4096, 4096), (6144, 4096), (14336, 4096), (4096, 14336)]
MS = [1, 2, 4, 8, 16, 128, 512]
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
    wq, ws, w8, s8 = [], [], [], []
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        q, s = T.fp8_quantize_rows(w)
        wq.append(q)
        ws.append(s.reshape(-1).contiguous())
        qi, si = T.int8_quantize_rows(w, 1e-5)
        w8.append(qi)
        s8.append(si)
        del w
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        xq, xs = T.fp8_quantize_rows(x)
        xs = xs.reshape(-1).contiguous()

        def int8dyn(i):
            if M == 1:
                return T.int8_dyn_linear(x, w8[i], s8[i], None)
            q8, sc8 = T.int8_quantize_per_token(x)
            return T.int8_scaled_mm(q8, sc8, w8[i], s8[i], None)

        paths = {
            "dyn": (lambda i: T.fp8_dyn_linear(x, wq[i], ws[i], None), {}),
            "mm": (lambda i: T.fp8_scaled_mm(xq, xs, wq[i], ws[i], None), {}),
            "quant": (lambda i: T.fp8_quantize_rows(x), {}),
            "fp8wo": (lambda i: T.fp8_weight_only_linear(x, wq[i], ws[i], None), {}),
            "int8dyn": (int8dyn, {}),
            "mm_mfma": (lambda i: T.fp8_scaled_mm(xq, xs, wq[i], ws[i], None), {"fp8dyn_mfma": 1}),
        }
        if M <= 8:
            paths["mm_gemv"] = (lambda i: T.fp8_scaled_mm(xq, xs, wq[i], ws[i], None),
                                {"linear_crossover": 8})
        vendor_error = None
        try:
            torch._scaled_mm(xq, wq[0].t(), scale_a=xs.view(-1, 1), scale_b=ws[0].view(1, -1),
                             out_dtype=torch.bfloat16, use_fast_accum=True)
            torch.cuda.synchronize()
            paths["vendor"] = (lambda i: torch._scaled_mm(
                xq, wq[i].t(), scale_a=xs.view(-1, 1), scale_b=ws[i].view(1, -1),
                out_dtype=torch.bfloat16, use_fast_accum=True), {})
        except (RuntimeError, NotImplementedError, ValueError) as e:
            vendor_error = str(e).splitlines()[0][:160]
        ref = (xq.double() @ wq[0].double().t()) * xs.double().view(-1, 1) * ws[0].double().view(1, -1)
        err, kernel = {}, {}
        for name, (fn, knobs) in paths.items():
            with tuning(**knobs):
                y = fn(0)
                kernel[name] = _lib.lib().tao_last_kernel().decode()
            if name in ("dyn", "mm", "mm_mfma", "mm_gemv", "vendor"):
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
            "mm_over_fp8wo": round(med["mm"] / med["fp8wo"], 4),
            "dyn_over_fp8wo": round(med["dyn"] / med["fp8wo"], 4),
            "dyn_over_int8dyn": round(med["dyn"] / med["int8dyn"], 4),
            "rel_l2_vs_float64": err, "vendor_error": vendor_error,
            "device": torch.cuda.get_device_name(0),
        })
        del graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8dyn_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp8dyn.py measures on the GPU; no device found")
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
