"""Time of one MoE expert FFN (Mixtral-8x7B shapes: E = 8, top-2, hidden 4096, expert 14336, int4
group size 32) over T tokens, in one process on one GPU:

  grouped            route, grouped gate-up, grouped down, combine (csrc/moe_gemm.hip) as routed by
                     csrc/moe_host.h
  grouped_bm{B}_d{n} the same with the row tile B in (16, 32, 64) forced and gate and up in two
                     launches + torch's silu and mul (d1) or one launch (d2)
  one_token_x_T      (T <= 4) T runs of the one-token grouped GEMV path: what the module would do if
                     it kept that path beyond one token
  loop               the reference's many-token sequence on the existing per-expert int4 linears
                     (argsort, bincount, cumsum, a host read of the counts, x[indices], three linears,
                     silu and mul per expert, cat, gather, mul, scatter_add): what the module would
                     do without the kernels. It synchronises with the host per call, so it cannot be
                     captured in a graph: timed eagerly by the wall clock (it calls the ops directly,
                     without the tensor-subclass dispatch the module would add)
  floor              the three plain int4 linears of every expert that has rows, at that expert's own
                     row count, and nothing else: no routing, gather, activation or combine

for T in 2, 4, 8, 16, 64, 256, 1024 and two routings: uniform (two distinct experts per token,
uniformly) and skewed (two distinct experts drawn with probability ~ 1 / (e + 1)^1.5).

Method (experiments/bench_mx.py's): every graphed path runs over layer copies rotated past the
Infinity Cache (each copy is ~0.9 GB of weights), captured in one HIP graph and timed by the wall
clock around `reps` replays ending in a device synchronise. The graphs are timed in alternation for
`rounds` rounds; per path the median over rounds and the spread (max - min) / median are
reported. Nothing here is a threshold.

One JSON line per (routing, T) to --out (default profiles/moe_bench.jsonl).
python experiments/bench_moe.py [--out FILE] [--rounds N] [--ts 2,64] [--copies N]
"""

import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "torchao-fork_amd"), os.path.join(ROOT, "experiments")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import torchao  # noqa: E402,F401
from bench_mx import make_graph, time_graph  # noqa: E402
from torchao import _lib  # noqa: E402
from torchao.kernel import moe  # noqa: E402

T_ = torch.ops.torchao
E, A, D, I, G = 8, 2, 4096, 14336, 32
TS = [2, 4, 8, 16, 64, 256, 1024]
DEV = "cuda"


def make_stack(N, K, gen):
    """A 3-D int4 weight as the kernels read it: (packed [E, N, K/8], scale_and_zero [E, N, K/g, 2])."""
    parts = [T_.int4_quantize_pack(
        (torch.randn(N, K, generator=gen, device=DEV) * 0.02).to(torch.bfloat16), G, 1e-6)
        for _ in range(E)]
    return (torch.stack([p for p, _ in parts]).contiguous(),
            torch.stack([s for _, s in parts]).contiguous())


def as_weight(stack):
    """What torchao.kernel.moe reads of a 3-D Int4WeightOnlyConfig weight."""
    return types.SimpleNamespace(
        tensor_impl=types.SimpleNamespace(packed_weight=stack[0], scale_and_zero=stack[1]),
        block_size=(1, 1, G))


def routing(Tn, kind, gen):
    if kind == "uniform":
        p = torch.ones(Tn, E, device=DEV)
    else:
        p = (1.0 / torch.arange(1, E + 1, device=DEV).float() ** 1.5).expand(Tn, E).contiguous()
    idx = torch.multinomial(p, A, generator=gen)
    w = torch.rand(Tn, A, generator=gen, device=DEV) + 0.5
    return idx, (w / w.sum(-1, keepdim=True)).to(torch.bfloat16)


def loop_ffn(x, layer, idx, w):
    (p1, s1), (p2, s2), (p3, s3) = layer
    flat = idx.reshape(-1)
    order = flat.argsort(stable=True)
    token_of = order.div(A).floor().to(torch.int64)
    ends = torch.bincount(flat, minlength=E).cumsum(0).tolist()
    outs, start = [], 0
    for e in range(E):
        cur = x[token_of[start:ends[e]]]
        y1 = F.silu(T_.int4_weight_only_linear(cur, p1[e], s1[e], G, None))
        y3 = T_.int4_weight_only_linear(cur, p3[e], s3[e], G, None)
        outs.append(T_.int4_weight_only_linear(y1 * y3, p2[e], s2[e], G, None))
        start = ends[e]
    weighted = torch.cat(outs, dim=0) * w.reshape(-1, 1)[order].view(-1, 1)
    index = token_of.unsqueeze(-1).expand(flat.numel(), D)
    return torch.zeros_like(x).scatter_add(dim=0, index=index, src=weighted)


def bench_case(Tn, kind, layers, rounds, emit):
    gen = torch.Generator(device=DEV).manual_seed(Tn * 3 + len(kind))
    x = torch.randn(Tn, D, generator=gen, device=DEV).to(torch.bfloat16)
    idx, w = routing(Tn, kind, gen)
    counts = torch.bincount(idx.reshape(-1), minlength=E).tolist()
    weights = [tuple(as_weight(s) for s in layer) for layer in layers]
    copies = len(layers)

    def grouped(i):
        w1, w2, w3 = weights[i]
        return moe.int4_moe_ffn_grouped(x, w1, w2, w3, idx, w, A)

    def one_token(i):
        w1, w2, w3 = weights[i]
        return [moe.int4_moe_ffn_one_token(x[t:t + 1], w1, w2, w3, idx[t], w[t]) for t in range(Tn)]

    xe = {e: torch.randn(c, D, generator=gen, device=DEV).to(torch.bfloat16)
          for e, c in enumerate(counts) if c}
    he = {e: torch.randn(c, I, generator=gen, device=DEV).to(torch.bfloat16)
          for e, c in enumerate(counts) if c}

    def floor(i):
        (p1, s1), (p2, s2), (p3, s3) = layers[i]
        return [(T_.int4_weight_only_linear(xe[e], p1[e], s1[e], G, None),
                 T_.int4_weight_only_linear(xe[e], p3[e], s3[e], G, None),
                 T_.int4_weight_only_linear(he[e], p2[e], s2[e], G, None)) for e in xe]

    paths = {"grouped": (grouped, {})}
    for bm in (16, 32, 64):
        for d in (1, 2):
            paths[f"grouped_bm{bm}_d{d}"] = (grouped, {"moe": (bm, d)})
    if Tn <= 4:
        paths["one_token_x_T"] = (one_token, {})
    paths["floor"] = (floor, {})
    # the grouped path against the loop before anything is timed: same routing, same weights
    ref, got = loop_ffn(x, layers[0], idx, w), grouped(0)
    rel = ((got.double() - ref.double()).norm() / ref.double().norm()).item()
    n = copies * max(1, 6 // copies)
    graphs = {name: make_graph(lambda fn=fn: [fn(i % copies) for i in range(n)], knobs)
              for name, (fn, knobs) in paths.items()}
    reps = {name: max(2, int(0.05 / (time_graph(g, n, 2) * n * 1e-6))) for name, g in graphs.items()}
    us = {name: [] for name in graphs}
    us["loop"] = []
    for _ in range(rounds):
        for name, g in graphs.items():
            us[name].append(time_graph(g, n, reps[name]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            loop_ffn(x, layers[i % copies], idx, w)
        torch.cuda.synchronize()
        us["loop"].append((time.perf_counter() - t0) / n * 1e6)
    med = {k: statistics.median(v) for k, v in us.items()}
    R = Tn * A
    best = min((k for k in med if k.startswith("grouped_bm")), key=lambda k: med[k])
    emit({
        "T": Tn, "routing": kind, "counts": counts, "E": E, "top_k": A, "D": D, "I": I, "g": G,
        "copies": copies, "rounds": rounds, "launches_per_graph": n,
        "row_tile_as_routed": int(_lib.lib().tao_moe_row_tile(R, E)),
        "dual_as_routed": int(_lib.lib().tao_moe_dual(R, E)),
        "us": {k: round(v, 2) for k, v in med.items()},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in us.items()},
        "best_forced": best, "loop_timed": "eager (host sync per call; not graph-capturable)",
        "loop_over_grouped": round(med["loop"] / med["grouped"], 2),
        "grouped_over_floor": round(med["grouped"] / med["floor"], 3),
        "rel_l2_grouped_vs_loop": round(rel, 6), "device": torch.cuda.get_device_name(0),
    })
    del graphs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ts", default=None)
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--routings", default="uniform,skewed")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe.py measures on the GPU; no device found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ts = [int(t) for t in args.ts.split(",")] if args.ts else TS
    gen = torch.Generator(device=DEV).manual_seed(0)
    layers = [(make_stack(I, D, gen), make_stack(D, I, gen), make_stack(I, D, gen))
              for _ in range(args.copies)]
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for kind in args.routings.split(","):
            for Tn in ts:
                bench_case(Tn, kind, layers, args.rounds, emit)


if __name__ == "__main__":
    main()
