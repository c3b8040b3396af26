#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    compare_device_code.py PARENT_TREE NEW_TREE [--diag] [-j N] [--keep DIR] FILE.hip [FILE.hip ...]

Each FILE (a name under codesearch_amd/csrc/) is compiled in both trees, device side only, to assembly with the Makefile's
FLAGS (--diag adds -DCS_DIAGNOSTICS, the second library's build).  The `__hip_cuid_` lines are dropped (that symbol is a hash
of the source text), then per kernel symbol the script prints whether body and kernel descriptor are the same text and, where
they are not, the instruction counts; for every kernel the compiler's own num_vgpr / num_agpr / private_seg_size (its
`.set <sym>.…` lines) and the LDS size.  It compares text and looks for no particular instruction.  Needs hipcc, no GPU.
Exit status 1 when any file differs.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("codesearch_amd", "csrc")


def makefile_flags(tree):
    """FLAGS of the tree's Makefile, with its continuation lines joined and $(ARCH) filled in."""
    text = open(os.path.join(tree, CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {}
    for name in ("HIPCC", "ARCH", "FLAGS"):
        m = re.search(r"^%s\s*\?=\s*(.*)$" % name, text, re.M)
        if not m:
            sys.exit("no %s in %s's Makefile" % (name, tree))
        var[name] = os.environ.get(name, m.group(1).strip())
    return var["HIPCC"], var["FLAGS"].replace("$(ARCH)", var["ARCH"]).split()


def device_asm(tree, name, diag, outdir):
    hipcc, flags = makefile_flags(tree)
    out = os.path.join(outdir, name + ".s")
    cmd = [hipcc] + flags + (["-DCS_DIAGNOSTICS"] if diag else []) + ["--offload-device-only", "-S", name, "-o", out]
    subprocess.run(cmd, cwd=os.path.join(tree, CSRC), check=True)
    return [l for l in open(out).read().splitlines() if "__hip_cuid_" not in l]


def kernels(lines):
    """{symbol: {"body": [...], "desc": [...], "insts": n, "vgpr"/"agpr"/"scratch"/"lds": n}}, in file order."""
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        out[m.group(1)] = {"desc": lines[i:end]}
    label = {l.split(":")[0]: j for j, l in enumerate(lines) if l[:1] not in ("\t", " ", ".", ";", "") and ":" in l}
    sets = {}
    for l in lines:
        m = re.match(r"\s*\.set\s+(\S+)\.(num_vgpr|num_agpr|private_seg_size),\s*(.*)", l)
        if m:
            sets[(m.group(1), m.group(2))] = m.group(3).strip()
    for sym, k in out.items():
        start = label[sym]
        end = next(j for j in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[j]))
        k["body"] = lines[start:end]
        k["insts"] = sum(1 for l in k["body"] if l.startswith("\t") and l[1:2] not in (".", ";", ""))
        for key, field in (("vgpr", "num_vgpr"), ("agpr", "num_agpr"), ("scratch", "private_seg_size")):
            k[key] = sets.get((sym, field), "?")
        k["lds"] = next(l.split()[1] for l in k["desc"] if ".amdhsa_group_segment_fixed_size" in l)
    return out


def numbers(k):
    return "vgpr %s agpr %s scratch %s lds %s" % (k["vgpr"], k["agpr"], k["scratch"], k["lds"])


def compare(name, a_lines, b_lines):
    a, b = kernels(a_lines), kernels(b_lines)
    same_file = a_lines == b_lines
    same = sum(1 for s in a if s in b and a[s]["body"] == b[s]["body"] and a[s]["desc"] == b[s]["desc"])
    print("== %s: %s; %d of %d kernels identical" % (name, "byte-identical" if same_file else "DIFFERS", same, len(a)))
    for s in a:
        if s not in b:
            print("   only in parent  %s" % s)
        elif a[s]["body"] == b[s]["body"] and a[s]["desc"] == b[s]["desc"]:
            print("   identical  %s  insts %d %s" % (s, a[s]["insts"], numbers(a[s])))
        else:
            print("   DIFFERENT  %s\n      parent: insts %d %s\n      new:    insts %d %s"
                  % (s, a[s]["insts"], numbers(a[s]), b[s]["insts"], numbers(b[s])))
    for s in b:
        if s not in a:
            print("   only in new     %s" % s)
    if not same_file and same == len(a) == len(b):
        print("   (the kernels are the same text: the difference is outside them)")
    return same_file


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--diag", action="store_true", help="compile with -DCS_DIAGNOSTICS")
    ap.add_argument("-j", type=int, default=4, help="compilations at a time")
    ap.add_argument("--keep", metavar="DIR", help="leave the assembly in DIR/parent and DIR/new (to diff a kernel by hand)")
    args = ap.parse_args()
    args.parent, args.new = os.path.abspath(args.parent), os.path.abspath(args.new)  # hipcc runs inside each tree
    args.keep = args.keep and os.path.abspath(args.keep)
    if makefile_flags(args.parent)[1] != makefile_flags(args.new)[1]:
        sys.exit("the two trees' Makefiles have different FLAGS: the code would differ for that alone\n  parent: %s\n  new:    %s"
                 % (" ".join(makefile_flags(args.parent)[1]), " ".join(makefile_flags(args.new)[1])))
    print("# parent %s, new %s, flags: %s%s" % (args.parent, args.new, " ".join(makefile_flags(args.new)[1]),
                                                 " -DCS_DIAGNOSTICS" if args.diag else ""))
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        if args.keep:
            tmp = args.keep
            os.makedirs(tmp, exist_ok=True)
        dirs = {t: os.path.join(tmp, d) for t, d in ((args.parent, "parent"), (args.new, "new"))}
        for d in dirs.values():
            os.makedirs(d, exist_ok=True)
        with concurrent.futures.ThreadPoolExecutor(args.j) as pool:
            jobs = {(t, f): pool.submit(device_asm, t, f, args.diag, dirs[t]) for f in args.files for t in dirs}
            for f in args.files:
                ok &= compare(f, jobs[(args.parent, f)].result(), jobs[(args.new, f)].result())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
