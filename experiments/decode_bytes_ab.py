"""Byte comparison of the five fused decode entries (tao_{int4wo,int8wo,int8dq,fp8wo,fp8dq}
_decode_bf16) between two builds of the library: fixed seeded inputs, norm on and off, every
epilogue, on small shapes with live tail lanes (tests/test_gpu_wo8_decode.py) and on the
Llama-3-8B wqkv and w1||w3 shapes. Each library runs once in a fresh child process
(TORCHAO_MI355X_LIB); a case's record is the SHA-256 of its output and of both KV caches (or the
entry's error text), and the two children's records must be equal.

    python experiments/decode_bytes_ab.py PARENT_LIB.so [--out profiles/decode_front_end_bytes.jsonl]

(the branch is the in-tree library). One JSON line per case; exit status 1 on any difference.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ENTRIES = ("int4wo", "int8wo", "int8dq", "fp8wo", "fp8dq")
EPI = {"none": 0, "swiglu": 1, "rope_kv": 2}
D, T, POS = 128, 64, 17
# (tag, K, {epilogue: (N, n_head, n_kv_head)})
SHAPES = [(f"small_k{K}", K, {"none": (37, 0, 0), "swiglu": (38, 0, 0), "rope_kv": (1536, 4, 4)})
          for K in (480, 992, 2016)]
SHAPES += [("8b_wqkv", 4096, {"none": (6144, 0, 0), "swiglu": (6144, 0, 0),
                              "rope_kv": (6144, 32, 8)}),
           ("8b_w13", 4096, {"none": (28672, 0, 0), "swiglu": (28672, 0, 0)})]


def child(out_path):
    import torch

    from torchao import _lib

    dev = "cuda"
    bf16 = torch.bfloat16

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
                              ).hexdigest()[:32]

    def operands(entry, N, K, g):
        if entry == "int4wo":
            w = torch.randint(-2 ** 31, 2 ** 31 - 1, (N, K // 8), dtype=torch.int32, generator=g)
            s = (torch.rand(N, K // 32, 2, generator=g) * 0.01).to(bf16)
        elif entry.startswith("int8"):
            w = torch.randint(-127, 128, (N, K), dtype=torch.int8, generator=g)
            s = (torch.rand(N, generator=g) * 0.01 + 1e-3).to(bf16)
        else:  # finite e4m3fn codes
            w = (torch.randn(N, K, generator=g) * 0.05).to(torch.float8_e4m3fn)
            s = torch.rand(N, generator=g) * 0.5 + 0.25
        return w.to(dev), s.to(dev)

    records = {}
    for tag, K, by_epi in SHAPES:
        for epi, (N, H, Hkv) in by_epi.items():
            for entry in ENTRIES:
                g = torch.Generator().manual_seed(K * 7 + N + ENTRIES.index(entry))
                w, s = operands(entry, N, K, g)
                x = torch.randn(1, 1, K, generator=g).to(bf16).to(dev)
                nw = (torch.rand(K, generator=g) + 0.5).to(bf16).to(dev)
                freqs = torch.randn(T, D // 2, 2, generator=g).to(dev)
                pos = torch.tensor([POS], device=dev)
                for norm in (False, True):
                    rope = epi == "rope_kv"
                    kc = torch.randn(1, max(Hkv, 1), T, D, generator=g).to(bf16).to(dev)
                    vc = torch.randn(1, max(Hkv, 1), T, D, generator=g).to(bf16).to(dev)
                    n_out = H * D if rope else N // 2 if epi == "swiglu" else N
                    y = torch.zeros(n_out, dtype=bf16, device=dev)
                    args = [x.data_ptr(), w.data_ptr(), s.data_ptr(), N, K]
                    if entry == "int4wo":
                        args.append(32)
                    args += [nw.data_ptr() if norm else None, 1e-5, EPI[epi], y.data_ptr(),
                             freqs.data_ptr() if rope else None, pos.data_ptr() if rope else None,
                             kc.data_ptr() if rope else None, vc.data_ptr() if rope else None,
                             H, Hkv, D if rope else 0, T if rope else 0,
                             torch.cuda.current_stream().cuda_stream]
                    key = f"{entry} {tag} N={N} K={K} {epi} norm={int(norm)}"
                    try:
                        _lib.call(f"tao_{entry}_decode_bf16", *args)
                        torch.cuda.synchronize()
                        kernel = _lib.lib().tao_last_kernel().decode()
                        records[key] = {"kernel": kernel, "y": sha(y), "k_cache": sha(kc),
                                        "v_cache": sha(vc), "y_nonzero": bool(y.any())}
                    except RuntimeError as e:  # a refusal is compared too
                        records[key] = {"error": str(e)}
    with open(out_path, "w") as f:
        json.dump(records, f)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default=None, help="where the children write their records")
    args = ap.parse_args()
    args.tmp = args.tmp or tempfile.mkdtemp()
    os.makedirs(args.tmp, exist_ok=True)
    recs = {}
    for side, lib in (("parent", os.path.abspath(args.parent_lib)), ("branch", None)):
        env = dict(os.environ)
        env.pop("TORCHAO_MI355X_LIB", None)
        if lib:
            env["TORCHAO_MI355X_LIB"] = lib
        path = os.path.join(args.tmp, f"decode_bytes_{side}.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env,
                       check=True, timeout=280)
        recs[side] = json.load(open(path))
    assert recs["parent"].keys() == recs["branch"].keys()
    bad = 0
    out = open(args.out, "w") if args.out else None
    for key, p in recs["parent"].items():
        b = recs["branch"][key]
        line = json.dumps({"case": key, "equal": p == b, "parent": p, "branch": b} if p != b else
                          {"case": key, "equal": True, **p})
        bad += p != b
        print(line)
        if out:
            out.write(line + "\n")
    print(f"{len(recs['parent'])} cases, {bad} differ", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
