"""Per-launch time of the float8 (e4m3fn) weight-only linear against its two comparators, in one
process on one GPU:

  fp8      torch.ops.torchao.fp8_weight_only_linear          (fp8wo_gemv_kernel / gemm_mfma_kernel)
  int8     torch.ops.torchao.int8_weight_only_linear         same bytes per weight, same decomposition
  dequant  torch.ops.torchao.fp8_dequantize + bf16 F.linear  the reference formulation
           (floatx/float8_layout.py:391-396: F.linear(x, weight.dequantize(), bias))

at M = 1 for 4096^2, 6144x4096, 14336x4096, 4096x14336 and at M = 128 for 4096^2.

Method: each path's launches over weight copies rotated past the Infinity Cache are captured in
one HIP graph (R launches back to back, no host gaps) and timed by the wall clock around `reps`
replays ending in a device synchronise. The three graphs are timed in alternation for `rounds`
rounds, so drift of the shared machine lands on all of them; per path the median over rounds and
the spread (max - min) / median are reported. The fp8 / int8 ratio is to be read against the
spread int8 itself shows. Outputs of the three paths are compared first (rel-L2 against the
float64 result of the first copy).

One JSON line per shape to --out (default profiles/fp8wo_bench.jsonl).
python experiments/bench_fp8wo.py [--out FILE] [--rounds N]
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

FP8 = torch.float8_e4m3fn
CASES = [(1, 4096, 4096), (1, 6144, 4096), (1, 14336, 4096), (1, 4096, 14336), (128, 4096, 4096)]
ROTATE_BYTES = 1 << 30  # weight bytes per rotation: four times the 256 MiB Infinity Cache


def make_graph(fn):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
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


def rel_l2(y, ref):
    return float((y.double() - ref).norm() / ref.norm())


def bench(M, N, K, rounds):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K + M)
    copies = max(3, -(-ROTATE_BYTES // (N * K)))
    x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
    wq, ws, w8, s8 = [], [], [], []
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        q, s = torch.ops.torchao.fp8_quantize_rows(w)
        wq.append(q)
        ws.append(s.reshape(-1).contiguous())
        qi, si = torch.ops.torchao.int8_quantize_rows(w, 1e-5)
        w8.append(qi)
        s8.append(si)
        del w
    paths = {
        "fp8": lambda i: torch.ops.torchao.fp8_weight_only_linear(x, wq[i], ws[i], None),
        "int8": lambda i: torch.ops.torchao.int8_weight_only_linear(x, w8[i], s8[i], None),
        "dequant": lambda i: torch.nn.functional.linear(
            x, torch.ops.torchao.fp8_dequantize(wq[i], ws[i])),
    }
    ref = x.double() @ (wq[0].float().double() * ws[0].double().view(-1, 1)).t()
    ref8 = x.double() @ (w8[0].double() * s8[0].double().view(-1, 1)).t()
    err, kernel = {}, {}
    for name, fn in paths.items():
        y = fn(0)
        kernel[name] = _lib.lib().tao_last_kernel().decode()
        err[name] = rel_l2(y, ref8 if name == "int8" else ref)
    del ref, ref8
    launches = copies * max(1, 48 // copies)
    graphs = {name: make_graph(lambda fn=fn: [fn(i % copies) for i in range(launches)])
              for name, fn in paths.items()}
    # enough work per timing: about 0.1 s of replays, sized from a first pass
    reps = {name: max(3, int(0.1 / (time_graph(g, launches, 3) * launches * 1e-6)))
            for name, g in graphs.items()}
    us = {name: [] for name in paths}
    for _ in range(rounds):
        for name, g in graphs.items():
            us[name].append(time_graph(g, launches, reps[name]))
    med = {n: statistics.median(v) for n, v in us.items()}
    spread = {n: (max(v) - min(v)) / med[n] for n, v in us.items()}
    nbytes = N * K + 4 * N + 2 * M * K + 2 * M * N  # fp8 algorithmic bytes
    return {
        "M": M, "N": N, "K": K, "copies": copies, "launches_per_graph": launches,
        "rounds": rounds, "reps": reps, "kernel": kernel,
        "us": {n: round(v, 3) for n, v in med.items()},
        "us_min": {n: round(min(v), 3) for n, v in us.items()},
        "spread": {n: round(v, 4) for n, v in spread.items()},
        "fp8_over_int8": round(med["fp8"] / med["int8"], 4),
        "dequant_over_fp8": round(med["dequant"] / med["fp8"], 3),
        "fp8_bytes": nbytes, "fp8_GBps": round(nbytes / med["fp8"] / 1e3, 1),
        "rel_l2_vs_float64": {n: float(f"{v:.3e}") for n, v in err.items()},
        "device": torch.cuda.get_device_name(0),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8wo_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp8wo.py measures on the GPU; no device found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for M, N, K in CASES:
            rec = bench(M, N, K, args.rounds)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
