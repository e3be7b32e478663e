"""Per-linear time of the SmoothQuant int8 linear (activation / smoothing factor, int8 dynamic or
static activation quantization, int8 x int8 linear) in one process on one GPU:

  new_dyn, new_static        torch.ops.torchao.int8_smooth_dyn_linear / int8_smooth_static_linear as
                             routed (M = 1: one launch where tao_int8_smooth_linear_fused says so;
                             else the fused smooth + quantize kernel, then int8_scaled_mm)
  parent_dyn, parent_static  what a hand-built wrapper runs without these ops: act_prescale, torch's
                             to_affine_quantized_intx / _static (eager kernels), int8_scaled_mm
  prescale_dyn               act_prescale, then the existing int8 dynamic ops (int8_dyn_linear at
                             M = 1, int8_quantize_per_token + int8_scaled_mm above): isolates the
                             division (the existing quantizer clamps at 1e-5, not 2^-7; same work)
  plain_dyn                  the existing int8 dynamic ops without smoothing: the floor
  plain_mm                   int8_scaled_mm alone on codes quantized beforehand
  M = 1 only:
  one_launch_dyn / _static   tao_int8_smooth_linear_bf16 itself, wherever it is served
  two_launch_dyn / _static   int8_smooth_quantize_per_token / _static, then int8_scaled_mm

for N x K in 4096^2, 6144x4096, 14336x4096, 4096x14336 at M = 1, 16, 128, 512.

Method (experiments/bench_mx.py's): each path's launches over weight copies rotated past the
Infinity Cache (at least 1 GiB of int8 weights per rotation) are captured in one HIP graph and
timed by the wall clock around `reps` replays ending in a device synchronise. The graphs are timed
in alternation for `rounds` rounds; per path the median over rounds and the spread
(max - min) / median are reported. Outputs of every smoothed path are compared bit for bit with
new_* before timing (prescale_dyn only where no token sits under the 2^-7 clamp).

What must hold: new_* <= parent_* beyond the spread at every shape and M; at M = 1 the one launch
is the op's route only where one_launch_* <= two_launch_* beyond the spread.

One JSON line per (shape, M) to --out (default profiles/smoothquant_bench.jsonl).
python experiments/bench_smoothquant.py [--out FILE] [--rounds N] [--shapes I,J] [--ms 1,16]
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
from torchao.dtypes import to_affine_quantized_intx, to_affine_quantized_intx_static  # noqa: E402
from torchao.quantization.quant_primitives import MappingType  # noqa: E402

T = torch.ops.torchao
MS = [1, 16, 128, 512]


def bench_shape(N, K, ms, rounds, emit):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(N * 7 + K)
    copies = max(3, -(-ROTATE_BYTES // (N * K)))
    wq = [torch.randint(-127, 128, (N, K), generator=gen, device=dev, dtype=torch.int8)
          for _ in range(copies)]
    ws = (0.001 + 0.02 * torch.rand(N, generator=gen, device=dev)).to(torch.bfloat16)
    s = (0.25 + 4 * torch.rand(K, generator=gen, device=dev)).to(torch.bfloat16)
    act = torch.tensor(0.05, dtype=torch.bfloat16, device=dev)
    zp = torch.zeros((), dtype=torch.int64, device=dev)
    for M in ms:
        x = torch.randn(M, K, generator=gen, device=dev).to(torch.bfloat16)
        xq0, xs0 = T.int8_quantize_per_token(x)

        def parent_dyn(i):
            a = to_affine_quantized_intx(T.act_prescale(x, s), MappingType.SYMMETRIC, [1, K],
                                         torch.int8, -127)
            return T.int8_scaled_mm(a.tensor_impl.int_data, a.tensor_impl.scale, wq[i], ws, None)

        def parent_static(i):
            a = to_affine_quantized_intx_static(T.act_prescale(x, s), act, zp, [M, K], torch.int8,
                                                -127)
            return T.int8_scaled_mm(a.tensor_impl.int_data,
                                    a.tensor_impl.scale.reshape(1).expand(M), wq[i], ws, None)

        def existing_dyn(t, i):
            if M == 1:
                return T.int8_dyn_linear(t, wq[i], ws, None)
            q, sc = T.int8_quantize_per_token(t)
            return T.int8_scaled_mm(q, sc, wq[i], ws, None)

        paths = {
            "new_dyn": lambda i: T.int8_smooth_dyn_linear(x, s, wq[i], ws, None),
            "new_static": lambda i: T.int8_smooth_static_linear(x, s, act, wq[i], ws, None),
            "parent_dyn": parent_dyn,
            "parent_static": parent_static,
            "prescale_dyn": lambda i: existing_dyn(T.act_prescale(x, s), i),
            "plain_dyn": lambda i: existing_dyn(x, i),
            "plain_mm": lambda i: T.int8_scaled_mm(xq0, xs0, wq[i], ws, None),
        }
        if M == 1:
            def two_launch(a):
                def run(i):
                    q, sc = (T.int8_smooth_quantize_per_token(x, s) if a is None
                             else T.int8_smooth_quantize_static(x, s, a))
                    return T.int8_scaled_mm(q, sc, wq[i], ws, None)
                return run

            def one_launch(a):
                def run(i):
                    y = torch.empty((1, N), dtype=torch.bfloat16, device=dev)
                    _lib.call("tao_int8_smooth_linear_bf16", x.data_ptr(), s.data_ptr(),
                              None if a is None else a.data_ptr(), wq[i].data_ptr(),
                              ws.data_ptr(), None, y.data_ptr(), 1, N, K,
                              torch.cuda.current_stream().cuda_stream)
                    return y
                return run

            paths["two_launch_dyn"] = two_launch(None)
            paths["two_launch_static"] = two_launch(act)
            if _lib.lib().tao_int8_smooth_linear_fused(1, N, K, 0):  # served, whatever the routing
                paths["one_launch_dyn"] = one_launch(None)
                paths["one_launch_static"] = one_launch(act)
        kernel, ys = {}, {}
        for name, fn in paths.items():
            ys[name] = fn(0)
            kernel[name] = _lib.lib().tao_last_kernel().decode()
        same = {n: bool(torch.equal(y, ys["new_static" if n.endswith("static") else "new_dyn"]))
                for n, y in ys.items() if not n.startswith("plain")}
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
            "M": M, "N": N, "K": K, "copies": copies, "launches_per_graph": launches,
            "rounds": rounds, "kernel": kernel,
            "us": {n: round(v, 3) for n, v in med.items()},
            "us_min": {n: round(min(v), 3) for n, v in us.items()},
            "spread": {n: round(v, 4) for n, v in spread.items()},
            "new_over_parent_dyn": round(med["new_dyn"] / med["parent_dyn"], 4),
            "new_over_parent_static": round(med["new_static"] / med["parent_static"], 4),
            "new_over_prescale_dyn": round(med["new_dyn"] / med["prescale_dyn"], 4),
            "new_over_plain_dyn": round(med["new_dyn"] / med["plain_dyn"], 4),
            "bit_equal_to_new": same,
            "device": torch.cuda.get_device_name(0),
        }
        if M == 1:
            rec["op_routes_one_launch"] = {
                mode: bool(_lib.lib().tao_int8_smooth_linear_fused(1, N, K, int(mode == "static")))
                for mode in ("dyn", "static")}
            for mode in ("dyn", "static"):
                if f"one_launch_{mode}" in med:
                    rec[f"one_over_two_launch_{mode}"] = round(
                        med[f"one_launch_{mode}"] / med[f"two_launch_{mode}"], 4)
        emit(rec)
        del graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smoothquant_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    ap.add_argument("--nk", nargs="*", default=[], help="further N,K shapes, after the list's")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smoothquant.py measures on the GPU; no device found")
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
