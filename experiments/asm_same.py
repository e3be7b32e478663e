"""Are the kernels of two builds the same code?  A diff of two sets of gfx950 assembly files.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/gemm_mfma.hip -o new/gemm_mfma.s
    python experiments/asm_same.py --old old/*.s --new new/*.s [--csv profiles/x.csv]

Kernels are keyed by mangled name, whichever file of a side holds them (so a kernel may move to
another source). Two things are compared per kernel: the lines from `<name>:` to its
`.Lfunc_end` (labels and instructions, comments dropped), and its `.amdhsa_kernel ...
.end_amdhsa_kernel` block. Only what depends on a kernel's position in its file is normalised
first: the function number inside local labels (.LBB<n>_<m>, .Lfunc_end<n>, .Lfunc_begin<n>) and
the __hip_cuid_* lines. One CSV row per kernel; exit status 1 if a kernel is missing, extra or
different.
"""

import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemv_asm_stats import kernels  # noqa: E402  (instruction list and .amdhsa_kernel fields)

_LABEL = re.compile(r"\.L(BB|func_end|func_begin)\d+")


def _norm(lines):
    out = []
    for line in lines:
        t = line.split(";")[0].rstrip()
        if not t.strip() or "__hip_cuid_" in t:
            continue
        out.append(_LABEL.sub(lambda m: ".L" + m.group(1) + "N", t.strip()))
    return out


def side(paths):
    """mangled name -> (file, normalised body, normalised descriptor block, stats)"""
    res = {}
    for path in paths:
        text = open(path).read()
        stats = kernels(text)
        for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
            name = m.group(1)
            body = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text,
                             re.S | re.M)
            if name in res:
                sys.exit(f"{name} is in both {res[name][0]} and {path}")
            ins, md = stats.get(name, ([], {}))
            res[name] = (os.path.basename(path), _norm(body.group(1).splitlines()) if body else None,
                         _norm(m.group(2).splitlines()), (len(ins), md))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--csv")
    a = ap.parse_args()
    old, new = side(a.old), side(a.new)
    rows = ["kernel,old_file,new_file,same,instructions,vgpr,sgpr,scratch"]
    bad = 0
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        same = o is not None and n is not None and o[1] is not None and o[1:3] == n[1:3]
        bad += not same
        cnt, md = (n or o)[3]
        rows.append(f"{name},{o[0] if o else ''},{n[0] if n else ''},{'yes' if same else 'no'},"
                    f"{cnt},{md.get('vgpr')},{md.get('sgpr')},{md.get('scratch')}")
    text = "\n".join(rows) + "\n"
    if a.csv:
        open(a.csv, "w").write(text)
    else:
        sys.stdout.write(text)
    print(f"{len(rows) - 1} kernels, {bad} missing / extra / different", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
