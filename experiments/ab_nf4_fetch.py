"""One-token time of tao_nf4_linear_bf16 (nf4_gemv_kernel) under the library this process loads
(TORCHAO_MI355X_LIB names a variant build, see experiments/ab_nf4_fetch.sh), for the level-fetch
A/B of DESIGN 4.19. The C entry is called directly, so no op library is needed; the stored
tensors are random (every code and scaler value occurs), the same for every variant.

Method of experiments/bench_nf4.py: launches over weight copies rotated past the Infinity Cache
in one HIP graph, wall clock around replays ending in a synchronise, median of `rounds`.
Prints one JSON line per shape: us, spread, and a checksum of the output bits.
"""

import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "torchao-fork_amd")]
import torch  # noqa: E402

from torchao import _lib  # noqa: E402

SHAPES = [(4096, 4096), (6144, 4096), (14336, 4096), (4096, 14336)]
LEVELS = (-1.0, -0.6962, -0.5251, -0.3949, -0.2844, -0.1848, -0.0911, 0.0,
          0.0796, 0.1609, 0.2461, 0.3379, 0.4407, 0.5626, 0.7230, 1.0)
ROTATE_BYTES = 1 << 29


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def main():
    if not torch.cuda.is_available():
        raise SystemExit("ab_nf4_fetch.py measures on the GPU; no device found")
    label = sys.argv[1] if len(sys.argv) > 1 else "in-tree"
    rounds = 5
    dev = "cuda"
    levels = torch.tensor(LEVELS, device=dev).to(torch.bfloat16)
    mean = torch.tensor(0.02, device=dev).to(torch.bfloat16)
    for N, K in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(N + K)
        copies = max(3, -(-ROTATE_BYTES // (N * K // 2)))
        ws = []
        for _ in range(copies):
            codes = torch.randint(0, 256, (N * K // 2,), generator=gen, device=dev,
                                  dtype=torch.uint8)
            qs = torch.randint(-128, 128, (N * K // 64,), generator=gen, device=dev,
                               dtype=torch.int8)
            qf = torch.full((N * K // 16384,), 4096.0, device=dev).to(torch.bfloat16)
            ws.append((codes, qs, qf))
        x = torch.randn(1, K, generator=gen, device=dev).to(torch.bfloat16)
        y = torch.empty(copies, N, dtype=torch.bfloat16, device=dev)

        def launch_all():
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for i, (codes, qs, qf) in enumerate(ws):
                _lib.call("tao_nf4_linear_bf16", ptr(x), ptr(codes), ptr(qs), ptr(qf), ptr(mean),
                          ptr(levels), ctypes.c_void_p(0), ptr(y[i]), 1, N, K, st)

        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            launch_all()
            with torch.cuda.graph(g, stream=s):
                launch_all()
        torch.cuda.current_stream().wait_stream(s)
        g.replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(rounds):
            reps = 40
            t0 = time.perf_counter()
            for _ in range(reps):
                g.replay()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / reps / copies * 1e6)
        med = statistics.median(us)
        print(json.dumps({"lib": label, "N": N, "K": K, "us": round(med, 3),
                          "spread": round((max(us) - min(us)) / med, 4),
                          "checksum": int(y.view(torch.int16).long().sum()),
                          "finite": bool(y.float().isfinite().all())}), flush=True)
        del g, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
