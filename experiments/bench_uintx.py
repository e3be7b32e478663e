"""Per-linear time of the uintx (1- to 7-bit) weight-only linear (csrc/uintx.hip) against what a
user has without it and against the int4 / int8 weight-only linears, in one process on one GPU:

  uintx              torch.ops.torchao.uintx_weight_only_linear as routed
  gemv               the same, forced onto the decode GEMV with the built-in lane unit
  gemv_u4/u8/u16     the GEMV with each lane unit forced (the A/B behind uintx_host.h's choice)
  gemv_xl1_u*, gemv_xlds_u*   at M = 3 .. 8: x read through L1 / staged in LDS, per lane unit (where
                     the staged x does not fit LDS, 8 tokens at K = 14336, both are the L1 form)
  dequant_mm         the same, forced onto the HIP dequantizer + F.linear (a bf16 temporary)
  torch_dequant      plain-torch unpack + dequantize_affine + F.linear on the same device: what a
                     user has without the kernels (timed for --torch-bits only, default 3)
  int4_g64, int8wo   torch.ops.torchao.int4_weight_only_linear (g 64) / int8_weight_only_linear

for every bit width at N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336, g 64, at M = 1, 2, 4, 8.
Shards are random bytes (every bit pattern is a valid code), scales and zero points random.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 512 MiB of the path's own weight bytes per rotation) are captured in one
HIP graph and timed by the wall clock around `reps` replays ending in a device synchronise. The
graphs are timed in alternation for `rounds` rounds; per path the median over rounds and the
spread (max - min) / median are reported. Nothing here is a threshold.

One JSON line per (bits, shape, M) to --out (default profiles/uintx_bench.jsonl).
python experiments/bench_uintx.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,8] [--bits 2,3]

--boundary (default --ms 4,8,12,16): only the routed linear and both forced routes: the
measurement behind the route's boundary (profiles/uintx_bench_boundary.jsonl).

--mfma (default --ms 2,4,8,16,32,64,128,256,512; profiles/uintx_mfma_bench.jsonl): the MFMA route
(tuning(uintx_mfma=1), with the GEMV boundary moved to one token so that it runs at every M > 1)
against the forced GEMV (M <= 32), the forced dequantize + matmul, int4 g64 and int8 weight-only
(these two once per shape and M, with the first width).
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
from torchao.dtypes.uintx.bitpacking import unpack  # noqa: E402
from torchao.quantization.quant_primitives import dequantize_affine  # noqa: E402

T = torch.ops.torchao
G = 64
ROTATE_BYTES = 1 << 29  # weight bytes per rotation: twice the 256 MiB Infinity Cache


def ncopies(weight_bytes):
    return max(3, -(-ROTATE_BYTES // weight_bytes))


def uintx_weights(bits, N, K, gen):
    """One random weight in op-argument order: (s4, s2, s1, scale, zero_point, bits, G)."""
    shards = [torch.randint(0, 256, (N, K * w // 8), generator=gen, device="cuda", dtype=torch.uint8)
              if bits & w else None for w in (4, 2, 1)]
    scale = (torch.rand(N, K // G, generator=gen, device="cuda") * 0.01 + 0.001).to(torch.bfloat16)
    zp = torch.randint(0, 2**bits, (N, K // G), generator=gen, device="cuda", dtype=torch.int32)
    return (*shards, scale, zp, bits, G)


def bench_shape(bits, N, K, ms, rounds, emit, boundary, torch_bits, others, mfma=False):
    gen = torch.Generator(device="cuda").manual_seed(N * 7 + K + bits)
    wbytes = N * K * bits // 8 + N * (K // G) * 6
    ux = [uintx_weights(bits, N, K, gen) for _ in range(ncopies(wbytes))]
    for M in ms:
        x = torch.randn(M, K, generator=gen, device="cuda").to(torch.bfloat16)

        def lin(i):
            return T.uintx_weight_only_linear(x, *ux[i], None)

        # name -> (fn, copies, tuning knobs)
        paths = {"uintx": (lin, len(ux), {}),
                 "dequant_mm": (lin, len(ux), {"uintx": (2, 0, 0, 0, 0, 0, 0)})}
        if M <= 32:
            paths["gemv"] = (lin, len(ux), {"uintx": (1, 0, 0, 0, 0, 0, 0)})
        if mfma:
            del paths["uintx"]
            paths["mfma"] = (lin, len(ux), {"uintx": (0, 1, 0, 0, 0, 0, 0), "uintx_mfma": 1})
        if mfma and others is not None:
            i4, i8 = others
            paths["int4_g64"] = (lambda i: T.int4_weight_only_linear(x, *i4[i], G, None), len(i4), {})
            paths["int8wo"] = (lambda i: T.int8_weight_only_linear(x, *i8[i], None), len(i8), {})
        if not boundary and not mfma:
            if M <= 8:
                for u in (4, 8, 16):
                    paths[f"gemv_u{u}"] = (lin, len(ux), {"uintx": (1, 0, 0, 0, 0, u, 0)})
            if 2 < M <= 8:  # x of the 4- / 8-token tiles through L1 or staged in LDS, per unit
                for u in (4, 8, 16):
                    paths[f"gemv_xl1_u{u}"] = (lin, len(ux), {"uintx": (1, 0, 0, 0, 0, u, 1)})
                    paths[f"gemv_xlds_u{u}"] = (lin, len(ux), {"uintx": (1, 0, 0, 0, 0, u, 2)})
            if bits in torch_bits:
                def torch_dequant(i):
                    s4, s2, s1, scale, zp, b, g = ux[i]
                    q = unpack([s for s in (s4, s2, s1) if s is not None], b)
                    return F.linear(x, dequantize_affine(q, (1, g), scale, zp, torch.uint8,
                                                         output_dtype=torch.bfloat16))

                paths["torch_dequant"] = (torch_dequant, len(ux), {})
            i4, i8 = others
            paths["int4_g64"] = (lambda i: T.int4_weight_only_linear(x, *i4[i], G, None), len(i4), {})
            paths["int8wo"] = (lambda i: T.int8_weight_only_linear(x, *i8[i], None), len(i8), {})
        launches = {n: (3 if n == "torch_dequant" else c * max(1, 48 // c))
                    for n, (_, c, _) in paths.items()}
        graphs = {n: make_graph(lambda fn=fn, c=c, k=launches[n]: [fn(i % c) for i in range(k)], kn)
                  for n, (fn, c, kn) in paths.items()}
        reps = {n: max(3, int(0.05 / (time_graph(g, launches[n], 3) * launches[n] * 1e-6)))
                for n, g in graphs.items()}
        us = {n: [] for n in paths}
        for _ in range(rounds):
            for n, g in graphs.items():
                us[n].append(time_graph(g, launches[n], reps[n]))
        med = {n: statistics.median(v) for n, v in us.items()}
        rec = {"bits": bits, "M": M, "N": N, "K": K, "g": G, "copies": len(ux), "rounds": rounds,
               "route": int(_lib.lib().tao_uintx_linear_route(M, N, K, bits)),
               "us": {n: round(v, 3) for n, v in med.items()},
               "spread": {n: round((max(v) - min(v)) / med[n], 4) for n, v in us.items()},
               "device": torch.cuda.get_device_name(0)}
        # bytes a GEMV must move: shards, scales and zero points; x and y once
        gb = (wbytes + 2 * M * (N + K)) / 1e9
        for n in med:
            if n.startswith("gemv"):
                rec[n + "_gbytes_per_s"] = round(gb / (med[n] * 1e-6), 1)
        if "gemv" in med:
            rec["gemv_over_dequant_mm"] = round(med["gemv"] / med["dequant_mm"], 4)
        if "mfma" in med:
            rec["dequant_mm_over_mfma"] = round(med["dequant_mm"] / med["mfma"], 3)
            if "gemv" in med:
                rec["gemv_over_mfma"] = round(med["gemv"] / med["mfma"], 3)
        emit(rec)
        del graphs
        torch.cuda.empty_cache()


def other_weights(N, K):
    gen = torch.Generator(device="cuda").manual_seed(N + K)
    i4, i8 = [], []
    for i in range(ncopies(N * K // 2)):
        w = (torch.randn(N, K, generator=gen, device="cuda") * 0.02).to(torch.bfloat16)
        i4.append(T.int4_quantize_pack(w, G, 1e-6))
        if i < ncopies(N * K):
            q, s = T.int8_quantize_rows(w, 1e-6)
            i8.append((q, s.reshape(-1).contiguous()))
    return i4, i8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=None)
    ap.add_argument("--bits", default="1,2,3,4,5,6,7")
    ap.add_argument("--torch-bits", default="3")
    ap.add_argument("--boundary", action="store_true",
                    help="time the linear on both forced routes at each M")
    ap.add_argument("--mfma", action="store_true",
                    help="time the MFMA route against both forced routes, int4 g64 and int8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_uintx.py measures on the GPU; no device found")
    out = args.out or os.path.join(
        ROOT, "profiles", "uintx_mfma_bench.jsonl" if args.mfma else
        "uintx_bench_boundary.jsonl" if args.boundary else "uintx_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    ms = [int(m) for m in args.ms.split(",")] if args.ms else (
        [2, 4, 8, 16, 32, 64, 128, 256, 512] if args.mfma else [4, 8, 12, 16] if args.boundary
        else [1, 2, 4, 8])
    torch_bits = {int(b) for b in args.torch_bits.split(",") if b}
    with open(out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for i in (int(v) for v in args.shapes.split(",") if v != ""):
            N, K = SHAPES[i]
            others = None if args.boundary else other_weights(N, K)
            for bits in (int(b) for b in args.bits.split(",")):
                bench_shape(bits, N, K, ms, args.rounds, emit, args.boundary, torch_bits, others,
                            args.mfma)
                if args.mfma:
                    others = None  # int4 / int8 do not depend on the width: once per shape


if __name__ == "__main__":
    main()
