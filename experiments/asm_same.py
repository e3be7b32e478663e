"""Are the kernels of two builds the same code?  A diff of two sets of gfx950 assembly files.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/gemm_mfma.hip -o new/gemm_mfma.s
    python experiments/asm_same.py --old old/*.s --new new/*.s [--csv profiles/x.csv]
        [--rename REGEX=REPL ...]

Kernels are keyed by mangled name, whichever file of a side holds them (so a kernel may move to
another source). --rename (repeatable) rewrites the old side's names with re.sub(REGEX, REPL, name)
before keying, so that a renamed kernel is compared against its predecessor, e.g.
    --rename '_ZN3tao12_GLOBAL__N_114mx_gemv_kernelI(.*)EEvNS0_10MxGemvArgsE=_ZN3tao18scaled_gemv_kernelINS_12_GLOBAL__N_15MxFmtE\\1EEvNT_4ArgsE'
Two things are compared per kernel: the lines from `<name>:` to its
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


def side(paths, renames=()):
    """mangled name (after renames) -> (file, normalised body, normalised descriptor block, stats)"""
    res = {}
    for path in paths:
        text = open(path).read()
        stats = kernels(text)
        for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
            name = m.group(1)
            body = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text,
                             re.S | re.M)
            ins, md = stats.get(name, ([], {}))
            parts = [_norm(body.group(1).splitlines()) if body else None,
                     _norm(m.group(2).splitlines())]
            was = name
            for rx, repl in renames:
                name = rx.sub(repl, name)
            if name != was:  # the kernel's own name inside its text (.section, .amdhsa_kernel)
                parts = [p and [t.replace(was, name) for t in p] for p in parts]
            if name in res:
                sys.exit(f"{name} is in both {res[name][0]} and {path}")
            res[name] = (os.path.basename(path), parts[0], parts[1], (len(ins), md))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--csv")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="rewrite the old side's kernel names before keying (repeatable)")
    a = ap.parse_args()
    renames = [(re.compile(rx), repl) for rx, repl in (r.split("=", 1) for r in a.rename)]
    old, new = side(a.old, renames), side(a.new)
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
