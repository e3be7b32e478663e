"""Decode-fused float8 GEMVs (tao_fp8wo_decode_bf16, tao_fp8dq_decode_bf16) against the chains they
replace, on the Llama-3-8B and 70B decode shapes. One graph of L launches over L distinct weight
copies (no cache reuse across layers, like the real decode step); the variants of one shape are
timed alternately in one process, three rounds, median reported. One JSON line per (format, op):

  fused_us      RMSNorm inside the GEMV + epilogue                       (1 launch)
  split_us      RMSNorm launch, then the GEMV with the epilogue          (2 launches)
  unfused_us    RMSNorm launch, the linear op, SiLU-mul / RoPE + KV write (2-3 launches)
  nonorm_us     the GEMV with the epilogue, no norm at all

    python experiments/bench_decode_fp8.py [--out profiles/fp8_decode_bench.jsonl]
    python experiments/bench_decode_fp8.py --sweep [--out profiles/fp8_decode_shape_ab.jsonl]

--sweep: the same rows under forced launch shapes (tao_tune_fp8_gemv: rows per wave, waves along
K, row groups; 0, 0, 0 = the built-in shapes), without the unfused chain.
"""
import argparse
import json
import statistics

import torch

from torchao import _lib
from torchao._models.llama import kernels

DEV = "cuda"
FP8 = torch.float8_e4m3fn
ENTRY = {"float8wo": "tao_fp8wo_decode_bf16", "float8dq": "tao_fp8dq_decode_bf16"}
EPI = {"none": 0, "swiglu": 1, "rope_kv": 2}
# where kernels.fp8wo_decode / fp8dq_decode take the norm inside the GEMV
pays = {"float8wo": lambda N, K: True, "float8dq": kernels.prologue_pays}


def time_graph(fn, L, reps=20):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(L):
            fn(i)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(L):
                fn(i)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps / L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    tunes = [(0, 0, 0)]
    if args.sweep:
        tunes += [(4, 4, 2), (8, 4, 2), (8, 8, 1), (4, 8, 1), (8, 4, 1), (4, 2, 4)]
    D, T = 128, 512
    # (model, op, N, K, epilogue, n_head)
    shapes = [
        ("8b", "wqkv_rope", 6144, 4096, "rope_kv", 32),
        ("8b", "w13_swiglu", 28672, 4096, "swiglu", 0),
        ("8b", "head", 128256, 4096, "none", 0),
        ("70b", "wqkv_rope", 10240, 8192, "rope_kv", 64),
        ("70b", "w13_swiglu", 57344, 8192, "swiglu", 0),
    ]
    Hkv = 8
    pos = torch.tensor([100], device=DEV)
    kc = torch.zeros(1, Hkv, T, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    freqs = torch.randn(T, D // 2, 2, device=DEV)
    out = open(args.out, "a") if args.out else None
    for model, op, N, K, epi, H in shapes:
        # enough copies that a graph replay streams well past the 256 MiB last-level cache
        L = max(2, min(32, -(-(3 << 29) // (N * K))))
        ws = [(torch.randint(0, 120, (N, K), dtype=torch.uint8, device=DEV).view(FP8),
               torch.rand(N, device=DEV) * 0.01 + 1e-3) for _ in range(L)]
        x = torch.randn(1, 1, K, device=DEV, dtype=torch.bfloat16)
        nw = (torch.rand(K, device=DEV) + 0.5).to(torch.bfloat16)
        rope = (freqs, pos, kc, vc, H)
        if epi == "rope_kv":
            y = torch.empty(1, H, 1, D, device=DEV, dtype=torch.bfloat16)
        else:
            y = torch.empty(1, 1, N // 2 if epi == "swiglu" else N, device=DEV,
                            dtype=torch.bfloat16)
        for fmt, entry in ENTRY.items():
            linear = (torch.ops.torchao.fp8_weight_only_linear if fmt == "float8wo"
                      else torch.ops.torchao.fp8_dyn_linear)

            def gemv(i, xin, norm):  # the C entry itself: kernels.fp8*_decode applies the rule
                w, s = ws[i]
                r = epi == "rope_kv"
                _lib.call(entry, xin.data_ptr(), w.data_ptr(), s.data_ptr(), N, K,
                          nw.data_ptr() if norm else None, 1e-5, EPI[epi], y.data_ptr(),
                          freqs.data_ptr() if r else None, pos.data_ptr() if r else None,
                          kc.data_ptr() if r else None, vc.data_ptr() if r else None,
                          H, Hkv if r else 0, D if r else 0, T if r else 0,
                          torch.cuda.current_stream().cuda_stream)

            def unfused(i):
                w, s = ws[i]
                o = linear(kernels.rmsnorm(x, nw, 1e-5).view(1, K), w, s, None)
                if epi == "swiglu":
                    kernels.silu_mul(o)
                elif epi == "rope_kv":
                    kernels.rope_kv(o.view(1, 1, N), freqs, pos, kc, vc, H)

            variants = {
                "fused_us": lambda i: gemv(i, x, True),
                "split_us": lambda i: gemv(i, kernels.rmsnorm(x, nw, 1e-5), False),
                "unfused_us": unfused,
                "nonorm_us": lambda i: gemv(i, x, False),
            }
            if args.sweep:
                del variants["unfused_us"]
            for tune in tunes:
                _lib.call("tao_tune_fp8_gemv", *tune)
                samples = {k: [] for k in variants}
                for _ in range(args.rounds):
                    for k, fn in variants.items():
                        samples[k].append(time_graph(fn, L))
                _lib.call("tao_tune_fp8_gemv", 0, 0, 0)
                res = {"model": model, "op": op, "format": fmt, "N": N, "K": K, "copies": L,
                       "tune": tune, "rule_fuses_norm": pays[fmt](N, K)}
                for k, v in samples.items():
                    res[k] = round(statistics.median(v), 3)
                    res[k.replace("_us", "_all")] = [round(t, 3) for t in v]
                line = json.dumps(res)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
        del ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
