"""Over which magnitude range is the 128-term sum of one v_mfma_scale_f32_16x16x128_f8f6f4 exact?

One MFMA (K = 128, M = 18, N = 16 through torch.ops.torchao.fp8_scaled_mm with the MFMA route
forced, unit scales): +2^16 at k = p0, -2^16 at k = p1 and 2^e at k = p2, e = 16 - (row + column),
so the exact sum is 2^e, a bf16 number. For each (p0, p1, p2) the first ratio 2^16 / 2^e at which
the output is not 2^e is reported (it was 0 there: the small product was dropped).

Found on the MI355X (profiles/fp8dyn_mfma_exact_probe.json):
  * p2 in the same aligned group of 8 k as p0 (or as p1): first loss at a ratio of 2^14;
  * p2 in another group of 8: first loss at 2^24 - 2^25, or none up to 2^32 when that group is
    16 or more k away from both;
  * so tests that want bit-exact sums keep every product of a row within 2^12 of the largest
    (tests/exact_inputs_fp8dyn.py).
python experiments/probe_mfma_f8_exact.py [OUT.json]
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchao-fork_amd"))
import torch
import torchao  # noqa
from torchao.kernel.tuning import tuning

dev = "cuda:0"
E4 = torch.float8_e4m3fn
out = {}
K = 128
cfgs = [(0, 1, 2), (0, 1, 3), (0, 1, 4), (0, 1, 8), (0, 1, 16), (0, 1, 32), (0, 1, 64), (0, 1, 127),
        (0, 64, 1), (0, 64, 2), (0, 64, 4), (0, 64, 8), (0, 64, 16), (0, 64, 32), (0, 64, 65),
        (0, 4, 1), (0, 16, 1), (0, 32, 1), (0, 2, 1), (5, 77, 127), (5, 77, 6), (0, 3, 2)]
for pos in cfgs:
    rows = 18
    x = torch.zeros(rows, K, dtype=torch.float64)
    w = torch.zeros(16, K, dtype=torch.float64)
    w[:, pos[0]] = 256.0
    w[:, pos[1]] = 256.0
    for r in range(rows):
        x[r, pos[0]] = 256.0
        x[r, pos[1]] = -256.0
        x[r, pos[2]] = 2.0 ** (8 - r)
    for n in range(16):
        w[n, pos[2]] = 2.0 ** (8 - n)
    with tuning(fp8dyn_mfma=1):
        y = torch.ops.torchao.fp8_scaled_mm(x.to(E4).to(dev), torch.ones(rows, device=dev),
                                            w.to(E4).to(dev), torch.ones(16, device=dev)).cpu().double()
    want = x.to(E4).double() @ w.to(E4).double().T
    span = {}
    got = {}
    for r in range(rows):
        for n in range(16):
            span.setdefault(r + n, []).append(bool(y[r, n] == want[r, n]))
            got.setdefault(r + n, set()).add(float(y[r, n] / want[r, n]))
    ff = next((k for k, v in sorted(span.items()) if not all(v)), None)
    out[str(pos)] = dict(first_fail=ff, ratios_at_fail=sorted(got[ff]) if ff is not None else None,
                         passes_after=[k for k, v in sorted(span.items()) if ff is not None and k > ff and all(v)])
dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fp8dyn_mfma_exact_probe.json")
os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
json.dump(out, open(dst, "w"), indent=1)
for k, v in out.items():
    print(k, v)
