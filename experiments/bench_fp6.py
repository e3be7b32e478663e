"""Per-linear time of the FP6 weight-only linear (csrc/fp6.hip) against what a user has without it
and against the other weight-only GEMVs, in one process on one GPU:

  {fmt}              torch.ops.torchao.fp6_weight_only_linear as routed, fmt in (e3m2, e2m3)
  {fmt}_gemv         the same, forced onto the decode GEMV with the built-in 24-B lane chunk
                     (8-token launches; timed up to M = 32)
  {fmt}_gemv48       the GEMV with the 48-B lane chunk (the A/B behind fp6_host.h's default)
  {fmt}_dequant_mm   the same, forced onto the HIP dequantizer + F.linear (a bf16 temporary)
  torch_dequant      the plain-torch dequantize (unpack the bit stream, table lookup, multiply) +
                     F.linear on the same device: what a user has without the kernels
  fp8wo, int8wo      torch.ops.torchao.fp8_weight_only_linear / int8_weight_only_linear
  int4_g32           torch.ops.torchao.int4_weight_only_linear at group size 32

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 2, 4, 8, 16, 128, and at 4096^2
the quantizer: to_affine_quantized_fpx on the HIP row quantizer against the plain-torch
formulation on the device.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 512 MiB of fp6 codes per rotation, the same number of copies for every
format) are captured in one HIP graph and timed by the wall clock around `reps` replays ending in
a device synchronise. The graphs are timed in alternation for `rounds` rounds; per path the median
over rounds and the spread (max - min) / median are reported. Nothing here is a threshold.

One JSON line per (shape, M) to --out (default profiles/fp6_bench.jsonl).
python experiments/bench_fp6.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,16]

--boundary (default --ms 2,4,8,16,32): only fp6 on both forced routes and as routed: the
measurement behind the route's boundary (profiles/fp6_bench_boundary.jsonl).
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
from torchao.dtypes.floatx.floatx_tensor_core_layout import (  # noqa: E402
    pack_floatx_native,
    unpack_floatx_native,
)
from torchao.kernel.tuning import tuning  # noqa: E402
from torchao.quantization.quant_primitives import (  # noqa: E402
    _choose_qparams_affine_floatx,
    _dequantize_affine_floatx,
    _quantize_affine_floatx,
)

T = torch.ops.torchao
FORMATS = {"e3m2": (3, 2), "e2m3": (2, 3)}
MS = [1, 2, 4, 8, 16, 128]
BOUNDARY_MS = [2, 4, 8, 16, 32]
GEMV_MAX_M = 32
ROTATE_BYTES = 1 << 29  # fp6 code bytes per rotation: twice the 256 MiB Infinity Cache


def time_quantizer(emit, rounds):
    N = K = 4096
    w = (torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16)
    for fmt, (e, m) in FORMATS.items():
        def hip():
            return T.fp6_quantize_rows(w, e, m)

        def plain():
            s = _choose_qparams_affine_floatx(w, e, m)
            return pack_floatx_native(_quantize_affine_floatx(w, s, e, m)), s

        (ch, sh), (cp, sp) = hip(), plain()
        assert torch.equal(ch, cp) and torch.equal(sh, sp), "quantizers disagree"
        ms = {"hip": [], "torch": []}
        for _ in range(rounds):
            for name, fn, reps in (("hip", hip, 20), ("torch", plain, 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / reps * 1e3)
        med = {n: statistics.median(v) for n, v in ms.items()}
        emit({"quantizer": fmt, "N": N, "K": K, "rounds": rounds,
              "ms": {n: round(v, 4) for n, v in med.items()},
              "spread": {n: round((max(v) - min(v)) / med[n], 4) for n, v in ms.items()},
              "torch_over_hip": round(med["torch"] / med["hip"], 2),
              "codes_equal": True, "device": torch.cuda.get_device_name(0)})


def bench_shape(N, K, ms, rounds, emit, boundary=False):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    copies = max(3, -(-ROTATE_BYTES // (N * K * 3 // 4)))
    f6 = {fmt: [] for fmt in FORMATS}
    f8, i8, i4 = [], [], []
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        for fmt, (e, m) in FORMATS.items():
            f6[fmt].append(T.fp6_quantize_rows(w, e, m))
        if not boundary:
            q, s = T.fp8_quantize_rows(w)
            f8.append((q, s.reshape(-1).contiguous()))
            q, s = T.int8_quantize_rows(w, 1e-6)
            i8.append((q, s.reshape(-1).contiguous()))
            i4.append(T.int4_quantize_pack(w, 32, 1e-6))
        del w
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        paths, knobs = {}, {}
        for fmt, (e, m) in FORMATS.items():
            def lin(i, fmt=fmt, e=e, m=m):
                return T.fp6_weight_only_linear(x, *f6[fmt][i], e, m, None)

            paths[fmt], knobs[fmt] = lin, {}
            paths[fmt + "_dequant_mm"], knobs[fmt + "_dequant_mm"] = lin, {"fp6": (2, 0, 0, 0, 0, 0)}
            if M <= GEMV_MAX_M:
                paths[fmt + "_gemv"], knobs[fmt + "_gemv"] = lin, {"fp6": (1, 0, 0, 0, 0, 1)}
                paths[fmt + "_gemv48"], knobs[fmt + "_gemv48"] = lin, {"fp6": (1, 0, 0, 0, 0, 2)}
        if not boundary:
            def torch_dequant(i):
                c, s = f6["e3m2"][i]
                return F.linear(x, _dequantize_affine_floatx(unpack_floatx_native(c), s, 3, 2,
                                                             torch.bfloat16))

            paths.update({
                "torch_dequant": torch_dequant,
                "fp8wo": lambda i: T.fp8_weight_only_linear(x, *f8[i], None),
                "int8wo": lambda i: T.int8_weight_only_linear(x, *i8[i], None),
                "int4_g32": lambda i: T.int4_weight_only_linear(x, *i4[i], 32, None),
            })
            knobs.update({"torch_dequant": {}, "fp8wo": {}, "int8wo": {}, "int4_g32": {}})
        kernel = {}  # the last project kernel of each path that launches one
        for name, fn in paths.items():
            with tuning(**knobs[name]):
                fn(0)
            if name != "torch_dequant":
                kernel[name] = _lib.lib().tao_last_kernel().decode()
        kernel["fp6_route"] = int(_lib.lib().tao_fp6_linear_route(M, N, K))
        # the plain-torch dequantize materialises several [N, K] temporaries per launch
        launches = {name: (copies * max(1, 48 // copies) if name != "torch_dequant" else 3)
                    for name in paths}
        graphs = {name: make_graph(lambda fn=fn, n=launches[name]: [fn(i % copies) for i in range(n)],
                                   knobs[name])
                  for name, fn in paths.items()}
        reps = {name: max(3, int(0.05 / (time_graph(g, launches[name], 3) * launches[name] * 1e-6)))
                for name, g in graphs.items()}
        us = {name: [] for name in paths}
        for _ in range(rounds):
            for name, g in graphs.items():
                us[name].append(time_graph(g, launches[name], reps[name]))
        med = {n: statistics.median(v) for n, v in us.items()}
        rec = {
            "M": M, "N": N, "K": K, "copies": copies, "rounds": rounds, "kernel": kernel,
            "us": {n: round(v, 3) for n, v in med.items()},
            "us_min": {n: round(min(v), 3) for n, v in us.items()},
            "spread": {n: round((max(v) - min(v)) / med[n], 4) for n, v in us.items()},
            "device": torch.cuda.get_device_name(0),
        }
        for fmt in FORMATS:
            if fmt + "_gemv" in med:
                rec[fmt + "_gemv_over_dequant_mm"] = round(
                    med[fmt + "_gemv"] / med[fmt + "_dequant_mm"], 4)
                rec[fmt + "_gemv48_over_gemv"] = round(med[fmt + "_gemv48"] / med[fmt + "_gemv"], 4)
                # bytes the GEMV must move: codes, one bf16 scale per row; x and y once
                gb = (N * K * 0.75 + 2 * N + 2 * M * (N + K)) / 1e9
                rec[fmt + "_gemv_gbytes_per_s"] = round(gb / (med[fmt + "_gemv"] * 1e-6), 1)
            if not boundary:
                rec[fmt + "_over_fp8wo"] = round(med[fmt] / med["fp8wo"], 4)
                rec[fmt + "_over_int8wo"] = round(med[fmt] / med["int8wo"], 4)
                rec[fmt + "_over_int4_g32"] = round(med[fmt] / med["int4_g32"], 4)
        if not boundary:
            rec["torch_dequant_over_e3m2"] = round(med["torch_dequant"] / med["e3m2"], 3)
            rec["fp8wo_gbytes_per_s"] = round(
                (N * K + 4 * N + 2 * M * (N + K)) / 1e9 / (med["fp8wo"] * 1e-6), 1)
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
                    help="time fp6_weight_only_linear on both forced routes at each M")
    ap.add_argument("--no-quantizer", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp6.py measures on the GPU; no device found")
    out = args.out or os.path.join(
        ROOT, "profiles", "fp6_bench_boundary.jsonl" if args.boundary else "fp6_bench.jsonl")
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
