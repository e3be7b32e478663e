"""Decode attention over the int8 KV cache against the bf16 routes, Llama-3-8B heads (32 q, 8 kv,
D 128), B = 1: 32 layers with distinct caches (as one decoded token runs them) in one HIP graph, µs
per layer from HIP events on the replay stream, the variants alternating over --rounds rounds (the
median is reported, the spread beside it). Variants per key count L (cache capacity T = L rounded
up to 8):
  bf16_attn_decode     tao_attn_decode_bf16 (one pass up to 1024 rows, else the two-launch chunk
                       split): Attention.forward_fused's route outside 1025..8192 rows
  bf16_split4_merge    tao_attn_decode_split_bf16 (4 ranges) + tao_attn_merge_bf16: its route inside
  q8_s1                tao_attn_decode_q8_bf16, one range
  q8_s2 / q8_s4        2 / 4 ranges + tao_attn_merge_bf16;  *_nomerge: without the merge
  rope_kv / rope_kv_q8 the RoPE + cache-write launch alone (the int8 cache's extra launch per layer
                       against the RoPE epilogue of the wqkv GEMV)
bytes: the K and V bytes a layer's attention has to read once (bf16: 8 heads x L rows x 512 B;
int8: 8 x (L - 1) x (256 + 4) B plus the current rows), and that over the time as a fraction of
8 TB/s. One JSON line per (variant, keys) to stdout and --out.

    python experiments/bench_attn_kvq8.py [--keys 328,1024,4096,8192,32768] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchao-fork_amd"))

from torchao._models.llama import kernels  # noqa: E402
from torchao._models.llama.model import AffineQuantizedKVCache  # noqa: E402


def make_graph(fn, dev):
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fn()
        g.replay()
    s.synchronize()
    torch.cuda.current_stream(dev).wait_stream(s)
    return g, s


def time_graph(g, s, reps, n):
    with torch.cuda.stream(s):
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps):
            g.replay()
        e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", default="328,1024,4096,8192,32768")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    H, Hkv, D, NL = 32, 8, 128, a.layers
    scale = 1 / math.sqrt(D)
    gen = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(1, H, 1, D, device=dev, dtype=torch.bfloat16, generator=gen)
    qkv = torch.randn(1, 1, (H + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16, generator=gen)
    k_cur = torch.randn(1, Hkv, 1, D, device=dev, dtype=torch.bfloat16, generator=gen)
    v_cur = torch.randn(1, Hkv, 1, D, device=dev, dtype=torch.bfloat16, generator=gen)
    pos = torch.zeros(1, dtype=torch.int64, device=dev)
    out = open(a.out, "a") if a.out else None
    for L in [int(x) for x in a.keys.split(",")]:
        T = (L + 7) // 8 * 8
        pos.fill_(L - 1)
        freqs = torch.randn(T, D // 2, 2, device=dev, generator=gen)
        kcs, vcs, q8s = [], [], []
        for _ in range(NL):
            kcs.append(torch.randn(1, Hkv, T, D, device=dev, dtype=torch.bfloat16, generator=gen))
            vcs.append(torch.randn(1, Hkv, T, D, device=dev, dtype=torch.bfloat16, generator=gen))
            kv = AffineQuantizedKVCache(1, T, Hkv, D, device=dev)
            for name, src in (("k_cache", kcs[-1]), ("v_cache", vcs[-1])):
                s = src.float().abs().amax(-1, keepdim=True) / 127
                getattr(kv, name).copy_((src.float() / s).round().clamp(-127, 127))
                getattr(kv, name + "_scale").copy_(s)
            q8s.append(kv)
        keep = [None] * NL

        def bf16_attn():
            for i in range(NL):
                keep[i] = kernels.attn_decode(q, kcs[i], vcs[i], pos, scale)

        def bf16_split(merge=True):
            def f():
                for i in range(NL):
                    p = kernels.attn_decode_split(q, kcs[i], vcs[i], pos, scale, 4)
                    keep[i] = kernels.attn_merge(p, 1, H) if merge else p
            return f

        def q8(S, merge=True):
            def f():
                for i in range(NL):
                    y = kernels.attn_decode_q8(q, q8s[i], k_cur, v_cur, pos, scale, S)
                    keep[i] = kernels.attn_merge(y, 1, H) if (S > 1 and merge) else y
            return f

        def rope():
            for i in range(NL):
                keep[i] = kernels.rope_kv(qkv, freqs, pos, kcs[i], vcs[i], H)

        def rope_q8():
            for i in range(NL):
                keep[i] = kernels.rope_kv_q8(qkv, freqs, pos, q8s[i], H)

        b16 = Hkv * L * D * 2 * 2
        b8 = Hkv * ((L - 1) * (2 * D + 4) + 2 * D * 2)
        variants = [("bf16_attn_decode", bf16_attn, b16), ("bf16_split4_merge", bf16_split(), b16),
                    ("q8_s1", q8(1), b8), ("q8_s2", q8(2), b8), ("q8_s4", q8(4), b8),
                    ("q8_s2_nomerge", q8(2, False), b8), ("q8_s4_nomerge", q8(4, False), b8),
                    ("rope_kv", rope, 0), ("rope_kv_q8", rope_q8, 0)]
        graphs = [(name, *make_graph(fn, dev), nbytes) for name, fn, nbytes in variants]
        times = {name: [] for name, *_ in graphs}
        for _ in range(a.rounds):
            for name, g, s, _ in graphs:
                times[name].append(time_graph(g, s, a.reps, NL))
        for name, g, s, nbytes in graphs:
            t = times[name]
            us = statistics.median(t)
            rec = {"variant": name, "keys": L, "T": T, "layers": NL,
                   "us_per_layer_graph": round(us, 3), "us_min": round(min(t), 3),
                   "us_max": round(max(t), 3)}
            if nbytes:
                rec["kv_bytes_per_layer"] = nbytes
                rec["frac_of_8TBps"] = round(nbytes / (us * 1e-6) / 8e12, 4)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del graphs, kcs, vcs, q8s
        torch.cuda.empty_cache()
    kernels.check_decode_status()


if __name__ == "__main__":
    main()
