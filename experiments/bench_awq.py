"""Per-linear time of the AWQ int4 linear (activation pre-scale + int4 g32 weight-only linear) in
one process on one GPU:

  fused       torch.ops.torchao.int4_prescaled_linear  the op as routed (one launch at M = 1 for K <= 4096
                                                         and N * K <= 2^24, else act_prescale + the linear)
  one_launch  tao_int4wo_prescaled_linear_bf16 itself  (M = 1 only: the division in the GEMV's x
                                                         prologue, whatever the op's routing says)
  two_launch  torch.ops.torchao.act_prescale, then torch.ops.torchao.int4_weight_only_linear
  plain       torch.ops.torchao.int4_weight_only_linear alone (no activation scale: the floor)
  torch_div   torch's x / s, then torch.ops.torchao.int4_weight_only_linear (the reference's form)

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 16, 128.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 1 GiB of packed weights per rotation) are captured in one HIP graph and
timed by the wall clock around `reps` replays ending in a device synchronise. The graphs are timed
in alternation for `rounds` rounds; per path the median over rounds and the spread
(max - min) / median are reported.

Decision rule (`one_launch_wins_m1`): at M = 1 the one launch stays the op's route for every shape
if its median is below the two-launch form's on all four shapes; otherwise each shape class goes to
whichever is faster (tao_int4wo_prescaled_linear_fused).

One JSON line per (shape, M) to --out (default profiles/awq_bench.jsonl).
python experiments/bench_awq.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,16] [--nk N,K ...]
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
from bench_mx import ROTATE_BYTES, SHAPES, make_graph, time_graph  # noqa: E402
from torchao import _lib  # noqa: E402

T = torch.ops.torchao
MS = [1, 16, 128]
G = 32


def bench_shape(N, K, ms, rounds, emit):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    copies = max(3, -(-ROTATE_BYTES // (N * K // 2)))
    qi, zi = [], []
    for _ in range(copies):
        w = (torch.randn(N, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        p, sz = T.int4_quantize_pack(w, G, 1e-6)
        qi.append(p)
        zi.append(sz)
        del w
    s = (0.25 + 4 * torch.rand(K, generator=gen, device=dev)).to(torch.bfloat16)
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        paths = {
            "fused": lambda i: T.int4_prescaled_linear(x, s, qi[i], zi[i], G, None),
            "two_launch": lambda i: T.int4_weight_only_linear(T.act_prescale(x, s), qi[i], zi[i], G,
                                                              None),
            "plain": lambda i: T.int4_weight_only_linear(x, qi[i], zi[i], G, None),
            "torch_div": lambda i: T.int4_weight_only_linear(x / s, qi[i], zi[i], G, None),
        }
        if M == 1 and K <= 16384:
            def one_launch(i):
                y = torch.empty((1, N), dtype=torch.bfloat16, device=dev)
                _lib.call("tao_int4wo_prescaled_linear_bf16", x.data_ptr(), s.data_ptr(),
                          qi[i].data_ptr(), zi[i].data_ptr(), None, y.data_ptr(), 1, N, K, G,
                          torch.cuda.current_stream().cuda_stream)
                return y
            paths["one_launch"] = one_launch
        kernel = {}
        ys = {}
        for name, fn in paths.items():
            ys[name] = fn(0)
            kernel[name] = _lib.lib().tao_last_kernel().decode()
        ref = ys["torch_div"].double()
        rel = {n: float(f"{float((y.double() - ref).norm() / ref.norm()):.3e}")
               for n, y in ys.items() if n != "plain"}
        launches = copies * max(1, 48 // copies)
        graphs = {name: make_graph(lambda fn=fn: [fn(i % copies) for i in range(launches)], {})
                  for name, fn in paths.items()}
        reps = {name: max(3, int(0.08 / (time_graph(g, launches, 3) * launches * 1e-6)))
                for name, g in graphs.items()}
        us = {name: [] for name in paths}
        for _ in range(rounds):
            for name, g in graphs.items():
                us[name].append(time_graph(g, launches, reps[name]))
        med = {n: statistics.median(v) for n, v in us.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in us.items()}
        rec = {
            "M": M, "N": N, "K": K, "group_size": G, "copies": copies,
            "launches_per_graph": launches, "rounds": rounds, "kernel": kernel,
            "us": {n: round(v, 3) for n, v in med.items()},
            "us_min": {n: round(min(v), 3) for n, v in us.items()},
            "spread": {n: round(v, 4) for n, v in spread.items()},
            "fused_over_two_launch": round(med["fused"] / med["two_launch"], 4),
            "fused_over_plain": round(med["fused"] / med["plain"], 4),
            "fused_over_torch_div": round(med["fused"] / med["torch_div"], 4),
            "rel_l2_vs_torch_div": rel,
            "device": torch.cuda.get_device_name(0),
        }
        if M == 1:
            rec["op_routes_fused"] = bool(
                _lib.lib().tao_int4wo_prescaled_linear_fused(1, N, K, 0))
            if "one_launch" in med:
                rec["one_launch_over_two_launch"] = round(med["one_launch"] / med["two_launch"], 4)
                rec["one_launch_wins_m1"] = bool(med["one_launch"] < med["two_launch"])
        emit(rec)
        del graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "awq_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    ap.add_argument("--nk", nargs="*", default=[], help="further N,K shapes, after the list's")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_awq.py measures on the GPU; no device found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ms = [int(m) for m in args.ms.split(",")]
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for i in (int(v) for v in args.shapes.split(",") if v != ""):
            bench_shape(*SHAPES[i], ms, args.rounds, emit)
        for nk in args.nk:
            bench_shape(*(int(v) for v in nk.split(",")), ms, args.rounds, emit)


if __name__ == "__main__":
    main()
