"""Per-linear time of the 2:4 sparse int8 linear (csrc/sparse24.hip) against the dense int8 dynamic
linear on the same pruned weight, in one process on one GPU:

  sp24_mm    torch.ops.torchao.int8_sp24_scaled_mm on codes quantized beforehand
  sp24_dyn   torch.ops.torchao.int8_sp24_dyn_linear, the whole linear from a bf16 activation
  int8_mm    torch.ops.torchao.int8_scaled_mm on the decompressed weight
  int8_dyn   int8_dyn_linear at M = 1, int8_quantize_per_token + int8_scaled_mm above

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 16, 128, 512. The baseline is
always the dense int8 op of the same process.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 1 GiB of dense int8 weights per rotation, the same number of copies for
both formats) are captured in one HIP graph and timed by the wall clock around `reps` replays ending
in a device synchronise. The graphs are timed in alternation for `rounds` rounds; per path the median
over rounds and the spread (max - min) / median are reported. A GEMV line also gives the achieved
bytes/s over values + meta. Outputs are compared bit for bit before timing.

Nothing here is a threshold. One JSON line per (shape, M) to --out (default
profiles/sp24_bench.jsonl).
python experiments/bench_sp24.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,16]

--boundary (default --ms 2,4,8,16, --out profiles/sp24_bench_boundary.jsonl): only the sparse scaled
mm, forced onto the GEMV and onto the GEMM through tao_tune_sp24: the measurement behind
kSp24GemvDefaultMaxM (csrc/sparse24_host.h).
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
from torchao.dtypes import SemiSparseLayout  # noqa: E402
from torchao.kernel import tuning  # noqa: E402

T = torch.ops.torchao
MS = [1, 16, 128, 512]
ROTATE_BYTES = 1 << 30  # dense int8 weight bytes per rotation: four times the Infinity Cache


def bench_shape(N, K, ms, rounds, emit, boundary=False):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    copies = max(3, -(-ROTATE_BYTES // (N * K)))
    w8, ws, sv, sm = [], [], [], []
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        q, s = T.int8_quantize_rows(SemiSparseLayout().pre_process(w), 1e-5)
        values, meta, err = T.int8_sp24_compress(q)
        assert int(err) == 0
        ws.append(s.reshape(-1).contiguous())
        sv.append(values)
        sm.append(meta)
        if not boundary:
            w8.append(q)
        del w, q
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        xq, xs = T.int8_quantize_per_token(x)

        def int8_dyn(i):
            if M == 1:
                return T.int8_dyn_linear(x, w8[i], ws[i], None)
            q, sc = T.int8_quantize_per_token(x)
            return T.int8_scaled_mm(q, sc, w8[i], ws[i], None)

        sp24_mm = lambda i: T.int8_sp24_scaled_mm(xq, xs, sv[i], sm[i], ws[i], None)  # noqa: E731
        if boundary:  # the sparse scaled mm on both routes, whatever the built-in boundary
            paths = {"sp24_mm_gemv": sp24_mm, "sp24_mm_gemm": sp24_mm}
            knobs = {"sp24_mm_gemv": {"sp24": (1, 0, 0, 0, 0)},
                     "sp24_mm_gemm": {"sp24": (2, 0, 0, 0, 0)}}
        else:
            paths = {
                "sp24_mm": sp24_mm,
                "sp24_dyn": lambda i: T.int8_sp24_dyn_linear(x, sv[i], sm[i], ws[i], None),
                "int8_mm": lambda i: T.int8_scaled_mm(xq, xs, w8[i], ws[i], None),
                "int8_dyn": int8_dyn,
            }
            knobs = {name: {} for name in paths}
        kernel, out = {}, {}
        for name, fn in list(paths.items()):
            try:
                with tuning(**knobs[name]):
                    out[name] = fn(0)
            except RuntimeError as e:  # a forced GEMV whose tokens do not fit LDS is refused
                if "tokens in LDS" not in str(e):
                    raise
                del paths[name]
                continue
            kernel[name] = _lib.lib().tao_last_kernel().decode()
        first = next(iter(out.values()))
        same = all(bool(torch.equal(first, o)) for o in out.values())
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
            "all_paths_bit_equal": same,
            "device": torch.cuda.get_device_name(0),
        }
        sparse_bytes = N * K * 5 // 8  # values + meta
        for name in paths:
            if "gemv" in kernel[name] and name.startswith("sp24"):
                rec.setdefault("gemv_gb_per_s", {})[name] = round(sparse_bytes / med[name] * 1e-3, 1)
        if boundary:
            rec["gemv_over_gemm"] = (round(med["sp24_mm_gemv"] / med["sp24_mm_gemm"], 4)
                                     if "sp24_mm_gemv" in med else None)
        else:
            rec["sp24_mm_over_int8_mm"] = round(med["sp24_mm"] / med["int8_mm"], 4)
            rec["sp24_dyn_over_int8_dyn"] = round(med["sp24_dyn"] / med["int8_dyn"], 4)
        emit(rec)
        del graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=None)
    ap.add_argument("--boundary", action="store_true",
                    help="time the sparse scaled mm forced onto the GEMV and onto the GEMM")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sp24.py measures on the GPU; no device found")
    name = "sp24_bench_boundary.jsonl" if args.boundary else "sp24_bench.jsonl"
    out = args.out or os.path.join(ROOT, "profiles", name)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    ms = [int(m) for m in (args.ms or ("2,4,8,16" if args.boundary else
                                       ",".join(map(str, MS)))).split(",")]
    with open(out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for i in (int(v) for v in args.shapes.split(",") if v != ""):
            bench_shape(*SHAPES[i], ms, args.rounds, emit, args.boundary)


if __name__ == "__main__":
    main()
