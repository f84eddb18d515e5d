#!/usr/bin/env python3
"""Do two builds hold the same gfx950 kernels?  The question behind every change that moves kernels between translation units
or touches code next to them: "the other kernels did not move".

    tools/kernels_same.py A.o[,A2.o...] B.o[,B2.o...]

Each object is a host object of spiht_amd/csrc/Makefile (the code object sits in its .hip_fatbin section) or a device-only
object (--cuda-device-only: the bundle itself).  The union of side A is compared with the union of side B, by mangled kernel
name: the names only one side has, the kernels whose metadata differ (registers, spills, LDS, scratch, kernarg size, workgroup
size), and the kernels whose instruction streams differ.  A name defined twice on one side is an error.

Streams are compared as text of `llvm-objdump -d --no-show-raw-insn` without addresses and comments.  Two things differ between
builds that hold the same code and are taken out first: the literal that `s_add_u32 / s_addc_u32 sN, sN, <literal>` adds to a
program counter read by s_getpc_b64 (the pc-relative address of a table or a function: it depends on where the kernel lies in
its unit), and the padding behind a function's last instruction.  The tool compares; it looks for no particular instruction.

Exit status 0 only when nothing differs (2: a tool failed or a name is defined twice).  The LLVM tools are taken from
$ROCM_PATH/llvm/bin (default /opt/rocm)."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")
SHOW = 3  # kernels whose first differing lines are printed


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, text=True, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE).stdout


def code_object(obj, tmp):
    """the gfx950 ELF inside obj"""
    base = os.path.join(tmp, "%d_%s" % (len(os.listdir(tmp)), os.path.basename(obj)))
    bundle = base + ".fatbin"
    try:  # a host object; the second path is objcopy's output file, so that obj itself is left alone
        run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + bundle, obj, base + ".copy")
    except subprocess.CalledProcessError:
        bundle = obj  # no such section: a device-only object
    run("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + bundle, "--targets=" + TARGET, "--output=" + base + ".elf")
    return base + ".elf"


def metadata(elf):
    """kernel name -> {key: value} for the keys of META, from the code object's notes"""
    out, cur = {}, None
    for line in run("llvm-readelf", "--notes", elf).splitlines():
        m = re.match(r"^  (- | {2})(\.\w+):\s*(.*)$", line)  # the keys of a kernel's own map (its arguments' lie deeper)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == ".name":
            out[m.group(3).strip("'\"")] = cur
        elif m.group(2) in META:
            cur[m.group(2)] = m.group(3)
    return out


PAD = re.compile(r"^(s_nop\b.*|s_code_end|\.\.\.)$")
GETPC = re.compile(r"^s_getpc_b64 s\[(\d+):(\d+)\]$")
PCADD = re.compile(r"^(s_addc?_u32) s(\d+), s(\d+), (0x[0-9a-fA-F]+|-?\d+)$")


def streams(elf):
    """function name -> its instructions, normalised"""
    out, cur = {}, None
    for line in run("llvm-objdump", "-d", "--no-show-raw-insn", elf).splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        text = " ".join(line.split("//")[0].split())
        if cur is not None and text and not text.startswith("Disassembly of section"):
            cur.append(text)
    for name, ins in out.items():
        while ins and PAD.match(ins[-1]):
            ins.pop()
        pc = set()  # scalar registers that hold a program counter whose offset has not been added yet
        for i, text in enumerate(ins):
            g = GETPC.match(text)
            if g:
                pc = {g.group(1), g.group(2)}
                continue
            a = PCADD.match(text)
            if a and a.group(2) == a.group(3) and a.group(2) in pc:
                ins[i] = "%s s%s, s%s, <pcrel>" % (a.group(1), a.group(2), a.group(2))
                pc.discard(a.group(2))
    return out


def side(objs, tmp):
    """kernel name -> (metadata, stream, object) of one side"""
    out = {}
    for obj in objs:
        elf = code_object(obj, tmp)
        md, st = metadata(elf), streams(elf)
        for name, m in md.items():
            if name in out:
                raise RuntimeError("%s is defined in %s and in %s" % (name, out[name][2], obj))
            if name not in st:
                raise RuntimeError("%s: kernel %s has metadata and no code" % (obj, name))
            out[name] = (m, st[name], obj)
    return out


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        try:
            a, b = side(sys.argv[1].split(","), tmp), side(sys.argv[2].split(","), tmp)
        except (subprocess.CalledProcessError, RuntimeError, OSError) as e:
            print("kernels_same: %s%s" % (e, ("\n" + e.stderr) if getattr(e, "stderr", None) else ""))
            return 2
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    meta = [k for k in both if a[k][0] != b[k][0]]
    code = [k for k in both if a[k][1] != b[k][1]]
    print("A: %s: %d kernels" % (sys.argv[1], len(a)))
    print("B: %s: %d kernels" % (sys.argv[2], len(b)))
    print("only in A: %d" % len(only_a))
    print("only in B: %d" % len(only_b))
    for side_name, names in (("A", only_a), ("B", only_b)):
        for k in names:
            print("  only in %s: %s" % (side_name, k))
    print("in both: %d, %d instructions in A, %d in B" % (len(both), sum(len(a[k][1]) for k in both), sum(len(b[k][1]) for k in both)))
    print("metadata differ: %d" % len(meta))
    for k in meta:
        print("  %s: %s" % (k, ", ".join("%s %s -> %s" % (f, a[k][0].get(f), b[k][0].get(f)) for f in META if a[k][0].get(f) != b[k][0].get(f))))
    print("instruction streams differ: %d" % len(code))
    for n, k in enumerate(code):
        print("  %s: %d -> %d instructions" % (k, len(a[k][1]), len(b[k][1])))
        if n < SHOW:
            i = next((i for i, (x, y) in enumerate(zip(a[k][1], b[k][1])) if x != y), min(len(a[k][1]), len(b[k][1])))
            for j in range(i, i + 4):
                print("    [%d] A: %-60s B: %s" % (j, a[k][1][j] if j < len(a[k][1]) else "-", b[k][1][j] if j < len(b[k][1]) else "-"))
    same = not (only_a or only_b or meta or code)
    print("SAME" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
