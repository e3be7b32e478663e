"""Per-linear time of the 2:4 sparse int4 weight-only linear (csrc/int4_sparse24.hip,
Int4WeightOnlyConfig(layout=MarlinSparseLayout())) against the dense int4 g128 linear of the same
process, on one GPU:

  sp24        torch.ops.torchao.int4_sp24_weight_only_linear as routed
  sp24_gemv   the same, forced onto the sparse GEMV (left out where its tokens do not fit LDS)
  sp24_gemm   the same, forced onto the sparse MFMA GEMM
  int4_g128   the dense Int4WeightOnlyConfig(group_size=128) module on the same bf16 weight
  dequant_mm  dequantize() of the sparse weight to bf16 + F.linear (one weight copy: its time is
              the dequantizer's traffic)

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 2, 4, 8, 16, 128, 512.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 768 MiB of compressed weights per rotation, the same number of copies for
every path) are captured in one HIP graph and timed by the wall clock around `reps` replays ending
in a device synchronise. The graphs are timed in alternation for `rounds` rounds; per path the median
over rounds and the spread (max - min) / median are reported, and the achieved bytes/s over values +
meta + scales. The largest difference between the sparse paths' outputs is reported (their fp32
sums run in different orders; tests/test_gpu_int4_sp24.py compares them on exact inputs).

Nothing here is a threshold. One JSON line per (shape, M) to --out (default
profiles/int4_sp24_bench.jsonl).
python experiments/bench_int4_sp24.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,16]

--boundary (default --ms 1,2,4,8,16, --out profiles/int4_sp24_bench_boundary.jsonl): only the forced
GEMV and the forced GEMM: the measurement behind kI4Sp24GemvDefaultMaxM
(csrc/int4_sparse24_host.h).
"""

import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "torchao-fork_amd"), os.path.join(ROOT, "experiments")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import torchao  # noqa: E402,F401
from bench_mx import SHAPES, make_graph, time_graph  # noqa: E402
from torchao import _lib  # noqa: E402
from torchao.dtypes import MarlinSparseLayout  # noqa: E402
from torchao.kernel import tuning  # noqa: E402
from torchao.quantization import Int4WeightOnlyConfig, quantize_  # noqa: E402

T = torch.ops.torchao
MS = [1, 2, 4, 8, 16, 128, 512]
ROTATE_BYTES = 768 << 20  # compressed weight bytes per rotation: three times the Infinity Cache
GEMV, GEMM = 1, 2


def bench_shape(N, K, ms, rounds, emit, boundary=False):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    sparse_bytes = N * K * 3 // 8 + (K // 128) * N * 2  # values + meta + scales
    copies = max(3, -(-ROTATE_BYTES // sparse_bytes))
    base = torch.nn.Linear(K, N, bias=False, device=dev, dtype=torch.bfloat16)
    base.weight.data = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
    sparse = copy.deepcopy(base)
    quantize_(sparse, Int4WeightOnlyConfig(group_size=128, layout=MarlinSparseLayout()))
    impl = sparse.weight.tensor_impl
    sp = [(impl.int_data.clone(), impl.meta.clone(), impl.scale.clone()) for _ in range(copies)]
    dense = []
    if not boundary:
        quantize_(base, Int4WeightOnlyConfig(group_size=128))
        dense = [copy.deepcopy(base) for _ in range(copies)]
    del base
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)

        def sp24(i):
            values, meta, scale = sp[i]
            return T.int4_sp24_weight_only_linear(x, values, meta, scale, 128)

        paths = {"sp24_gemv": sp24, "sp24_gemm": sp24}
        knobs = {"sp24_gemv": {"int4_sp24": (GEMV,) + (0,) * 7},
                 "sp24_gemm": {"int4_sp24": (GEMM,) + (0,) * 7}}
        if not boundary:
            paths.update({"sp24": sp24, "int4_g128": lambda i: dense[i](x),
                          "dequant_mm": lambda i: F.linear(x, sparse.weight.dequantize())})
            knobs.update({"sp24": {}, "int4_g128": {}, "dequant_mm": {}})
        kernel, out = {}, {}
        for name, fn in list(paths.items()):
            try:
                with tuning(**knobs[name]), torch.no_grad():
                    out[name] = fn(0)
            except RuntimeError as e:  # a forced GEMV whose tokens do not fit LDS is refused
                if "tokens in LDS" not in str(e):
                    raise
                del paths[name]
                continue
            kernel[name] = _lib.lib().tao_last_kernel().decode()
        first = out["sp24_gemm"]
        diff = max(float((first.float() - o.float()).abs().max())
                   for n, o in out.items() if n.startswith("sp24"))
        launches = copies * max(1, 48 // copies)

        def run(fn):
            with torch.no_grad():
                return [fn(i % copies) for i in range(launches)]

        graphs = {name: make_graph(lambda fn=fn: run(fn), knobs[name]) for name, fn in paths.items()}
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
            "sparse_paths_max_abs_diff": diff,
            "sparse_bytes": sparse_bytes,
            "gb_per_s": {n: round(sparse_bytes / med[n] * 1e-3, 1) for n in med
                         if n.startswith("sp24")},
            "device": torch.cuda.get_device_name(0),
        }
        if "sp24_gemv" in med:
            rec["gemv_over_gemm"] = round(med["sp24_gemv"] / med["sp24_gemm"], 4)
        if not boundary:
            rec["sp24_over_int4_g128"] = round(med["sp24"] / med["int4_g128"], 4)
            rec["sp24_over_dequant_mm"] = round(med["sp24"] / med["dequant_mm"], 4)
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
                    help="time only the forced GEMV and the forced GEMM")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_int4_sp24.py measures on the GPU; no device found")
    name = "int4_sp24_bench_boundary.jsonl" if args.boundary else "int4_sp24_bench.jsonl"
    out = args.out or os.path.join(ROOT, "profiles", name)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    ms = [int(m) for m in (args.ms or ("1,2,4,8,16" if args.boundary else
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
