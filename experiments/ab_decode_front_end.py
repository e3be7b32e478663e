"""Timing of the fused decode entries between two builds of the library, alternated in one visit
(the method of profiles/gemv_refactor_ab.jsonl): each run is a fresh child process on one library
(TORCHAO_MI355X_LIB); a row's launches over weight copies rotated past the Infinity Cache are
captured in one graph and event-timed, median of 5 x 30 replays per run; runs alternate parent (A)
and branch (B). A row passes when branch / parent of the medians lies inside the parent's own
run-to-run spread, (max - min) / median of its runs.

    python experiments/ab_decode_front_end.py PARENT_LIB.so [--runs 5]
        [--out profiles/decode_front_end_ab.jsonl]

Rows: int8wo and fp8wo on the four Llama-3-8B linears (wqkv with norm + rope_kv, w1||w3 with norm
+ swiglu, wo and w2 plain), fp8wo with the norm at 4096 x 3072 (2 pieces per thread under the
default 8 x 4 x 1 shape, as K = 4096 is too), and int4, int8dq and fp8dq on wqkv as controls.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

D, T = 128, 512
# (path, entry, N, K, norm, epilogue, n_head, n_kv_head)
ROWS = []
for e in ("int8wo", "fp8wo"):
    ROWS += [(f"{e}_wqkv_norm_rope_kv", e, 6144, 4096, True, 2, 32, 8),
             (f"{e}_w13_norm_swiglu", e, 28672, 4096, True, 1, 0, 0),
             (f"{e}_wo_plain", e, 4096, 4096, False, 0, 0, 0),
             (f"{e}_w2_plain", e, 4096, 14336, False, 0, 0, 0)]
ROWS += [("fp8wo_npt2_norm", "fp8wo", 4096, 3072, True, 0, 0, 0)]
ROWS += [(f"{e}_wqkv_norm_rope_kv", e, 6144, 4096, True, 2, 32, 8)
         for e in ("int4wo", "int8dq", "fp8dq")]
METHOD = ("graph of launches over weights rotated past the Infinity Cache, event-timed, median of "
          "5 x 30 replays per run; runs alternate parent (A) and branch (B) libraries in one visit")


def child(out_path):
    import torch

    from torchao import _lib

    dev, bf16 = "cuda", torch.bfloat16
    res = {}
    for path, entry, N, K, norm, epi, H, Hkv in ROWS:
        L = max(2, min(32, -(-(3 << 29) // (N * K))))
        g = torch.Generator(device=dev).manual_seed(N + K)
        ws = []
        for _ in range(L):
            if entry == "int4wo":
                w = torch.randint(-2 ** 31, 2 ** 31 - 1, (N, K // 8), dtype=torch.int32,
                                  device=dev, generator=g)
                s = (torch.rand(N, K // 32, 2, device=dev, generator=g) * 0.01).to(bf16)
            elif entry.startswith("int8"):
                w = torch.randint(-127, 128, (N, K), dtype=torch.int8, device=dev, generator=g)
                s = (torch.rand(N, device=dev, generator=g) * 0.01 + 1e-3).to(bf16)
            else:
                w = torch.randint(0, 120, (N, K), dtype=torch.uint8, device=dev,
                                  generator=g).view(torch.float8_e4m3fn)
                s = torch.rand(N, device=dev, generator=g) * 0.01 + 1e-3
            ws.append((w, s))
        x = torch.randn(1, 1, K, device=dev, generator=g).to(bf16)
        nw = (torch.rand(K, device=dev, generator=g) + 0.5).to(bf16)
        rope = epi == 2
        kc = torch.zeros(1, max(Hkv, 1), T, D, device=dev, dtype=bf16)
        vc = torch.zeros_like(kc)
        freqs = torch.randn(T, D // 2, 2, device=dev, generator=g)
        pos = torch.tensor([100], device=dev)
        y = torch.empty(H * D if rope else N // 2 if epi == 1 else N, device=dev, dtype=bf16)

        def launch(i):
            w, s = ws[i]
            args = [x.data_ptr(), w.data_ptr(), s.data_ptr(), N, K]
            if entry == "int4wo":
                args.append(32)
            _lib.call(f"tao_{entry}_decode_bf16", *args, nw.data_ptr() if norm else None, 1e-5,
                      epi, y.data_ptr(), freqs.data_ptr() if rope else None,
                      pos.data_ptr() if rope else None, kc.data_ptr() if rope else None,
                      vc.data_ptr() if rope else None, H, Hkv, D if rope else 0,
                      T if rope else 0, torch.cuda.current_stream().cuda_stream)

        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for i in range(L):
                launch(i)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                for i in range(L):
                    launch(i)
        torch.cuda.current_stream().wait_stream(st)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        kernel = _lib.lib().tao_last_kernel().decode()
        samples = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(30):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3 / 30 / L)
        res[path] = {"us": statistics.median(samples), "kernel": kernel, "copies": L}
        del ws, graph
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default=None, help="where the children write their records")
    args = ap.parse_args()
    args.tmp = args.tmp or tempfile.mkdtemp()
    os.makedirs(args.tmp, exist_ok=True)
    runs = {"parent": [], "branch": []}
    for i in range(args.runs):
        for side, lib in (("parent", os.path.abspath(args.parent_lib)), ("branch", None)):
            env = dict(os.environ)
            env.pop("TORCHAO_MI355X_LIB", None)
            if lib:
                env["TORCHAO_MI355X_LIB"] = lib
            path = os.path.join(args.tmp, f"ab_decode_front_end_{side}_{i}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env,
                           check=True, timeout=200)
            runs[side].append(json.load(open(path)))
            print(f"run {i} {side} done", file=sys.stderr, flush=True)
    out = open(args.out, "w") if args.out else None
    for path, entry, N, K, norm, epi, H, Hkv in ROWS:
        p = [round(r[path]["us"], 4) for r in runs["parent"]]
        b = [round(r[path]["us"], 4) for r in runs["branch"]]
        pm, bm = statistics.median(p), statistics.median(b)
        spread = (max(p) - min(p)) / pm
        line = json.dumps({
            "path": path, "kernel": runs["branch"][0][path]["kernel"], "M": 1, "N": N, "K": K,
            "norm": norm, "epilogue": ["none", "swiglu", "rope_kv"][epi],
            "copies": runs["branch"][0][path]["copies"], "parent_us": p, "branch_us": b,
            "parent_median_us": round(pm, 4), "branch_median_us": round(bm, 4),
            "branch_over_parent": round(bm / pm, 4), "parent_aa_spread": round(spread, 4),
            "within_spread": abs(bm / pm - 1) <= spread, "device": "MI355X", "method": METHOD})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
