"""Per-kernel instruction statistics of a gfx950 assembly file.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/int4_gemv.hip -o int4_gemv.s
    python experiments/gemv_asm_stats.py int4_gemv.s [substring of the demangled kernel name]

For every kernel whose name holds the substring (default: int4wo_gemv): instructions in all,
instructions ahead of the first global_load, s_waitcnt lgkmcnt ahead of it, whether a
v_rcp_iflag_f32 (the 32-bit integer division sequence) appears, VALU count, and the kernarg
segment size, VGPRs, SGPRs and scratch from the kernel's metadata.
"""

import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return out.stdout.splitlines() if out.returncode == 0 else names


def kernels(text):
    """name -> list of instruction lines, for every .amdhsa_kernel in the file"""
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        body = m.group(2)

        def field(k):
            f = re.search(rf"\.amdhsa_{k} (\d+)", body)
            return int(f.group(1)) if f else None

        meta[m.group(1)] = {"kernarg": field("kernarg_size"), "vgpr": field("next_free_vgpr"),
                            "sgpr": field("next_free_sgpr"),
                            "scratch": field("private_segment_fixed_size")}
    res = {}
    for name in meta:
        m = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)
        if not m:
            continue
        ins = []
        for line in m.group(1).splitlines():
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") or t.endswith(":"):
                continue
            ins.append(t)
        res[name] = (ins, meta[name])
    return res


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "int4wo_gemv"
    ks = kernels(open(path).read())
    names = sorted(ks)
    pretty = dict(zip(names, demangle(names)))
    print("| kernel | instr | before 1st load | lgkm waits before | v_rcp_iflag | VALU | "
          "kernarg B | VGPR | SGPR | scratch |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for n in names:
        p = re.sub(r"^void tao::\(anonymous namespace\)::", "", pretty[n])
        p = re.sub(r"\(.*$", "", p)
        if want not in p:
            continue
        ins, md = ks[n]
        first = next((i for i, t in enumerate(ins) if t.startswith("global_load")), len(ins))
        waits = sum(1 for t in ins[:first] if t.startswith("s_waitcnt") and "lgkmcnt" in t)
        rcp = any(t.startswith("v_rcp_iflag_f32") for t in ins)
        valu = sum(1 for t in ins if t.startswith("v_"))
        print(f"| `{p}` | {len(ins)} | {first} | {waits} | {'yes' if rcp else 'no'} | {valu} | "
              f"{md['kernarg']} | {md['vgpr']} | {md['sgpr']} | {md['scratch']} |")


if __name__ == "__main__":
    main()
