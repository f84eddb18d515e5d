#!/usr/bin/env python3
"""isa_mix.py -- what a kernel issues, by instruction class, from the assembly of one translation unit.

    hipcc <the Makefile's flags of the file> --cuda-device-only -S dwt_fwd.hip -o dwt_fwd.s
    python3 tools/isa_mix.py dwt_fwd.s 'k_dwt_level<6, 62u, 14u, 0, false>'

The kernel is named by its mangled symbol, or by a piece of its demangled name (c++filt / llvm-cxxfilt is asked when one
is there; every kernel whose name contains the piece is reported).  Per kernel one line of static counts:

    float64 VALU   v_* mnemonics with an f64 operand type in their name
    other VALU     every other v_*
    scalar         s_*
    LDS            ds_*
    vector memory  buffer_*, global_*, flat_*, scratch_*
    VGPRs          the kernel's "; NumVgprs:" line

and, with --top N, its N most frequent mnemonics.  Classes go by the mnemonic's prefix alone; the counts are static (an
instruction in a loop or on a path not taken counts once).
"""
import argparse
import collections
import re
import shutil
import subprocess
import sys

CLASSES = ("float64 VALU", "other VALU", "scalar", "LDS", "vector memory", "other")
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
MNEMONIC = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def classify(m):
    if m.startswith("v_"):
        return "float64 VALU" if "_f64" in m else "other VALU"
    if m.startswith("s_"):
        return "scalar"
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vector memory"
    return "other"


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: (out[i] if i < len(out) and out[i] else n) for i, n in enumerate(names)}


def kernels(lines):
    """{symbol: (mnemonic counter, vgprs)} of every .amdhsa_kernel of the file"""
    syms = [l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")]
    want = set(syms)
    res = {}
    cur = None
    for l in lines:
        m = LABEL.match(l)
        if m and m.group(1) in want:
            cur = m.group(1)
            res[cur] = [collections.Counter(), None]
            continue
        if cur is None:
            continue
        if l.startswith(".Lfunc_end") or l.lstrip().startswith(".section"):
            cur = None
            continue
        if l.lstrip().startswith(";"):
            continue
        mm = MNEMONIC.match(l)
        if mm:
            res[cur][0][mm.group(1)] += 1
    # register counts: the assembler's comment block behind each kernel ("; NumVgprs: N")
    cur = None
    for l in lines:
        m = LABEL.match(l)
        if m and m.group(1) in res:
            cur = m.group(1)
        m = re.match(r"^;\s*NumVgprs:\s*(\d+)", l)
        if m and cur is not None and res[cur][1] is None:
            res[cur][1] = int(m.group(1))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("kernel", help="mangled symbol, or a piece of the demangled name")
    ap.add_argument("--top", type=int, default=0, help="also list the N most frequent mnemonics")
    ap.add_argument("--label", default=None, help="a word in front of each line (which build this is)")
    a = ap.parse_args()
    lines = open(a.asm, errors="replace").read().split("\n")
    ks = kernels(lines)
    names = demangle(sorted(ks))
    hits = [s for s in sorted(ks) if s == a.kernel or a.kernel in names[s]]
    if not hits:
        sys.exit("no kernel matches %r (%d kernels in %s)" % (a.kernel, len(ks), a.asm))
    for s in hits:
        cnt, vg = ks[s]
        by = collections.Counter()
        for m, n in cnt.items():
            by[classify(m)] += n
        head = (a.label + " ") if a.label else ""
        print("%s%s" % (head, names[s]))
        print("  " + "  ".join("%s %d" % (c, by[c]) for c in CLASSES if c != "other" or by[c]) + "  VGPRs %s" % vg)
        if a.top:
            print("  " + ", ".join("%s %d" % (m, n) for m, n in cnt.most_common(a.top)))


if __name__ == "__main__":
    main()
