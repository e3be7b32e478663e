"""Per-linear time of the NVFP4 linear (csrc/nvfp4.hip) against what a user has without it and
against the other 4-bit linears, in one process on one GPU:

  wo, dyn              torch.ops.torchao.nvfp4_linear as routed, WEIGHT_ONLY / DYNAMIC, swizzled scales
  wo_gemv, dyn_gemv    the same, forced onto the decode GEMV (8-token launches; timed up to M = 32)
  wo_dequant_mm, dyn_dequant_mm   forced onto the HIP dequantizer + F.linear (a bf16 temporary)
  torch_dequant        NVFP4Tensor's plain-torch dequantize (unpack, table lookup, multiply) +
                       F.linear on the same device: what a user has without the kernels
  mxfp4w               torch.ops.torchao.mxfp4w_dyn_linear (MXFP4 weights under MXFP8 activations)
  int4_g32             torch.ops.torchao.int4_weight_only_linear at group size 32

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 2, 4, 8, 16, 128.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 512 MiB of codes per rotation) are captured in one HIP graph and timed by
the wall clock around `reps` replays ending in a device synchronise. The graphs are timed in
alternation for `rounds` rounds; per path the median over rounds and the spread (max - min) /
median are reported. Nothing here is a threshold.

One JSON line per (shape, M) to --out (default profiles/nvfp4_bench.jsonl).
python experiments/bench_nvfp4.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,16]

--boundary (default --ms 2,4,8,16,32): only the forced routes and as routed, both modes: the
measurement behind the route's boundary (profiles/nvfp4_bench_boundary.jsonl).

--mfma (default --ms 2,4,8,16,32,64,128,256,512; profiles/nvfp4_mfma_bench.jsonl): the MFMA route,
the Nvfp4WO policy of gemm_mfma_kernel (tuning(nvfp4_mfma=1), the GEMV keeping one token only),
against both forced routes, in both modes and both scale layouts:
  {wo,dyn}_mfma, {wo,dyn}_mfma_rowmajor   the MFMA route on swizzled / row-major scales
  {wo,dyn}_gemv, {wo,dyn}_dequant_mm      as above (swizzled scales)
  mxfp4w, int4_g32                        the neighbouring 4-bit linears
--mfma --boundary (default --ms 2,3,4,5,6,8; profiles/nvfp4_mfma_bench_boundary.jsonl): only the
MFMA route and the forced GEMV, and per shape one more line with the first M at which the MFMA route
beats the GEMV in each mode.
"""

import argparse
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
from torchao.kernel.tuning import tuning  # noqa: E402
from torchao.prototype.mx_formats.nvfp4_tensor import NVFP4Tensor  # noqa: E402

T = torch.ops.torchao
MS = [1, 2, 4, 8, 16, 128]
BOUNDARY_MS = [2, 4, 8, 16, 32]
MFMA_MS = [2, 4, 8, 16, 32, 64, 128, 256, 512]
MFMA_BOUNDARY_MS = [2, 3, 4, 5, 6, 8]
MFMA_KNOBS = {"nvfp4": (0, 1, 0, 0, 0), "nvfp4_mfma": 1}  # GEMV at one token only, MFMA above
GEMV_MAX_M = 32
ROTATE_BYTES = 1 << 29  # code bytes per rotation: twice the 256 MiB Infinity Cache


def bench_shape(N, K, ms, rounds, emit, boundary, mfma=False):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    copies = max(3, -(-ROTATE_BYTES // (N * K // 2)))
    nv, m4, i4, rm = [], [], [], []
    first = {}  # --mfma --boundary: mode -> the first M at which the MFMA route beats the GEMV
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        nv.append(T.nvfp4_quantize(w, None, True))
        if mfma and not boundary:  # the same codes under row-major scales
            rm.append((nv[-1][0], T.nvfp4_quantize(w, None, False)[1]))
        if not boundary:
            m4.append(T.mxfp4_quantize_rows(w))
            i4.append(T.int4_quantize_pack(w, 32, 1e-6))
        del w
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        paths, knobs = {}, {}
        for mode, dyn in (("wo", False), ("dyn", True)):
            def lin(i, dyn=dyn):
                return T.nvfp4_linear(x, *nv[i], None, None, True, dyn, None)

            if mfma:
                paths[mode + "_mfma"], knobs[mode + "_mfma"] = lin, MFMA_KNOBS
                if rm:
                    paths[mode + "_mfma_rowmajor"] = (
                        lambda i, dyn=dyn: T.nvfp4_linear(x, *rm[i], None, None, False, dyn, None))
                    knobs[mode + "_mfma_rowmajor"] = MFMA_KNOBS
            else:
                paths[mode], knobs[mode] = lin, {}
            if not (mfma and boundary):
                paths[mode + "_dequant_mm"] = lin
                knobs[mode + "_dequant_mm"] = {"nvfp4": (2, 0, 0, 0, 0)}
            if M <= GEMV_MAX_M:
                paths[mode + "_gemv"], knobs[mode + "_gemv"] = lin, {"nvfp4": (1, 0, 0, 0, 0)}
        if not boundary:
            def torch_dequant(i):
                q, s = nv[i]
                t = NVFP4Tensor(q, s.view(torch.float8_e4m3fn), None, None, 16, torch.float32, True)
                return F.linear(x, t.to_dtype(torch.float32).to(torch.bfloat16))

            paths.update({
                "torch_dequant": torch_dequant,
                "mxfp4w": lambda i: T.mxfp4w_dyn_linear(x, *m4[i], None),
                "int4_g32": lambda i: T.int4_weight_only_linear(x, *i4[i], 32, None),
            })
            if mfma:
                del paths["torch_dequant"]
            knobs.update({n: {} for n in paths if n not in knobs})
        kernel = {}  # the last project kernel of each path that launches one
        for name, fn in paths.items():
            with tuning(**knobs[name]):
                fn(0)
            if name != "torch_dequant":
                kernel[name] = _lib.lib().tao_last_kernel().decode()
        kernel["route"] = int(_lib.lib().tao_nvfp4_linear_route(M, N, K))
        if mfma:
            assert kernel["wo_mfma"] == kernel["dyn_mfma"] == "gemm_mfma_kernel", kernel
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
        for mode in ("wo", "dyn"):
            if mode + "_gemv" in med and mode + "_dequant_mm" in med:
                rec[mode + "_gemv_over_dequant_mm"] = round(
                    med[mode + "_gemv"] / med[mode + "_dequant_mm"], 4)
                # bytes the GEMV must move: codes and scale bytes; x and y once
                gb = (N * K * 0.5625 + 2 * M * (N + K)) / 1e9
                rec[mode + "_gemv_gbytes_per_s"] = round(gb / (med[mode + "_gemv"] * 1e-6), 1)
        if not boundary:
            base = "wo_mfma" if mfma else "wo"
            for other in (() if mfma else ("torch_dequant",)) + ("mxfp4w", "int4_g32"):
                rec[f"{other}_over_{base}"] = round(med[other] / med[base], 3)
        if mfma:
            for mode in ("wo", "dyn"):
                if not boundary:
                    rec[mode + "_mfma_over_dequant_mm"] = round(
                        med[mode + "_mfma"] / med[mode + "_dequant_mm"], 4)
                elif med[mode + "_mfma"] < med[mode + "_gemv"]:
                    first.setdefault(mode, M)
        emit(rec)
        del graphs
        torch.cuda.empty_cache()
    if mfma and boundary:
        emit({"N": N, "K": K, "ms": ms, "first_m_mfma_beats_gemv": first})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=None)
    ap.add_argument("--boundary", action="store_true",
                    help="time nvfp4_linear on both forced routes at each M")
    ap.add_argument("--mfma", action="store_true",
                    help="time the MFMA route (tuning(nvfp4_mfma=1)) against the forced routes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nvfp4.py measures on the GPU; no device found")
    out = args.out or os.path.join(
        ROOT, "profiles", ("nvfp4_mfma_bench" if args.mfma else "nvfp4_bench")
        + ("_boundary.jsonl" if args.boundary else ".jsonl"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    default_ms = ((MFMA_BOUNDARY_MS if args.boundary else MFMA_MS) if args.mfma
                  else (BOUNDARY_MS if args.boundary else MS))
    ms = [int(m) for m in args.ms.split(",")] if args.ms else default_ms
    with open(out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for i in (int(v) for v in args.shapes.split(",") if v != ""):
            bench_shape(*SHAPES[i], ms, args.rounds, emit, args.boundary, args.mfma)


if __name__ == "__main__":
    sys.exit(main())
