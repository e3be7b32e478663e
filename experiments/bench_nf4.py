"""Per-linear time of the NF4 linear (csrc/nf4.hip) against what a user has without it and against
the int4 weight-only linears, in one process on one GPU:

  nf4             torch.ops.torchao.nf4_linear as routed
  nf4_gemv        the same, forced onto the decode GEMV (8-token launches; timed up to M = 32)
  nf4_dequant_mm  the same, forced onto the HIP dequantizer + F.linear (a bf16 temporary)
  torch_dequant   the plain-torch dequantize (nf4tensor._dequantize_plain: shifts, two
                  gathers, a division, an add, two multiplies, stack, reshape) + F.linear: the
                  reference's formulation on the same device, what LinearNF4 costs without the kernels
  int4_g32, int4_g64   torch.ops.torchao.int4_weight_only_linear at group sizes 32 and 64

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 16, 128, 512, 4096, and at 4096^2
the quantizer: to_nf4 on the HIP block quantizer against the plain-torch formulation on the device.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 512 MiB of packed codes per rotation, the same number of copies for every
format) are captured in one HIP graph and timed by the wall clock around `reps` replays ending in
a device synchronise. The graphs are timed in alternation for `rounds` rounds; per path the median
over rounds and the spread (max - min) / median are reported. Nothing here is a threshold.

One JSON line per (shape, M) to --out (default profiles/nf4_bench.jsonl).
python experiments/bench_nf4.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,16]

--boundary (default --ms 1,2,4,8,16,32): only nf4 on both forced routes and as routed: the
measurement behind the route's boundary (profiles/nf4_bench_boundary.jsonl).
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "torchao-fork_amd"), os.path.join(ROOT, "experiments")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import torchao  # noqa: E402,F401
from bench_mx import SHAPES, make_graph, time_graph  # noqa: E402
from torchao import _lib  # noqa: E402
from torchao.dtypes.nf4tensor import _dequantize_plain, _quantize_plain, to_nf4  # noqa: E402
from torchao.kernel import tuning  # noqa: E402

T = torch.ops.torchao
MS = [1, 16, 128, 512, 4096]
BOUNDARY_MS = [1, 2, 4, 8, 16, 32]
GEMV_MAX_M = 32
ROTATE_BYTES = 1 << 29  # packed code bytes per rotation: twice the 256 MiB Infinity Cache


def parts(t):
    return (t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean, t.nf4)


def time_quantizer(emit, rounds):
    N = K = 4096
    w = (torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16)

    def hip():
        return to_nf4(w)

    def plain():
        return _quantize_plain(w.flatten(), 64, 256, hip.t.nf4)[0]

    hip.t = hip()
    assert torch.equal(plain(), hip.t.quantized_data), "quantizers disagree"
    ms = {"to_nf4_hip": [], "to_nf4_torch": []}
    for _ in range(rounds):
        for name, fn, reps in (("to_nf4_hip", hip, 20), ("to_nf4_torch", plain, 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    med = {n: statistics.median(v) for n, v in ms.items()}
    emit({"quantizer": True, "N": N, "K": K, "rounds": rounds,
          "ms": {n: round(v, 4) for n, v in med.items()},
          "spread": {n: round((max(v) - min(v)) / med[n], 4) for n, v in ms.items()},
          "torch_over_hip": round(med["to_nf4_torch"] / med["to_nf4_hip"], 2),
          "codes_equal": True, "device": torch.cuda.get_device_name(0)})


def bench_shape(N, K, ms, rounds, emit, boundary=False):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    copies = max(3, -(-ROTATE_BYTES // (N * K // 2)))
    nf, g32, s32, g64, s64 = [], [], [], [], []
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        nf.append(to_nf4(w))
        if not boundary:
            q, s = T.int4_quantize_pack(w, 32, 1e-6)
            g32.append(q)
            s32.append(s)
            q, s = T.int4_quantize_pack(w, 64, 1e-6)
            g64.append(q)
            s64.append(s)
        del w
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)

        def nf4(i):
            return T.nf4_linear(x, *parts(nf[i]), N, None)

        paths = {"nf4": nf4, "nf4_dequant_mm": nf4}
        knobs = {"nf4": {}, "nf4_dequant_mm": {"nf4": (2, 0, 0, 0, 0)}}
        if M <= GEMV_MAX_M:
            paths["nf4_gemv"] = nf4
            knobs["nf4_gemv"] = {"nf4": (1, 0, 0, 0, 0)}
        if not boundary:
            paths.update({
                "torch_dequant": lambda i: F.linear(x, _dequantize_plain(nf[i])),
                "int4_g32": lambda i: T.int4_weight_only_linear(x, g32[i], s32[i], 32, None),
                "int4_g64": lambda i: T.int4_weight_only_linear(x, g64[i], s64[i], 64, None),
            })
            knobs.update({"torch_dequant": {}, "int4_g32": {}, "int4_g64": {}})
        kernel = {}  # the last project kernel of each path that launches one
        for name, fn in paths.items():
            with tuning(**knobs[name]):
                fn(0)
            if name != "torch_dequant":
                kernel[name] = _lib.lib().tao_last_kernel().decode()
        kernel["nf4_route"] = int(_lib.lib().tao_nf4_linear_route(M, N, K))
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
        if "nf4_gemv" in med:
            rec["gemv_over_dequant_mm"] = round(med["nf4_gemv"] / med["nf4_dequant_mm"], 4)
            # bytes the GEMV must move: codes, int8 scalers, factors; x and y once
            gb = (N * K * (0.5 + 1 / 64 + 2 / 16384) + 2 * M * (N + K)) / 1e9
            rec["gemv_gbytes_per_s"] = round(gb / (med["nf4_gemv"] * 1e-6), 1)
        if not boundary:
            rec["torch_dequant_over_nf4"] = round(med["torch_dequant"] / med["nf4"], 3)
            rec["nf4_over_int4_g32"] = round(med["nf4"] / med["int4_g32"], 4)
            rec["nf4_over_int4_g64"] = round(med["nf4"] / med["int4_g64"], 4)
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
                    help="time nf4_linear on both forced routes at each M")
    ap.add_argument("--no-quantizer", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nf4.py measures on the GPU; no device found")
    out = args.out or os.path.join(
        ROOT, "profiles", "nf4_bench_boundary.jsonl" if args.boundary else "nf4_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    ms = [int(m) for m in args.ms.split(",")] if args.ms else (BOUNDARY_MS if args.boundary else MS)
    with open(out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if not args.boundary and not args.no_quantizer:
            time_quantizer(emit, args.rounds)
        for i in (int(v) for v in args.shapes.split(",") if v != ""):
            bench_shape(*SHAPES[i], ms, args.rounds, emit, args.boundary)


if __name__ == "__main__":
    main()
