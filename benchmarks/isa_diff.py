#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code of two builds: the evidence for a refactor that must not change machine code (the
timing counterpart is benchmarks/ab.sh).  Usage: benchmarks/isa_diff.py A B [-v] [--map A_SYMBOL=B_SYMBOL ...]   (A, B: two
libcgd_mi355x.so, or two executables such as the benchmarks/ubench programs).  --map compares a kernel of A with a kernel of B that carries
another name (a kernel that became a template instantiation: same code expected, other mangled name).

Extracts every gfx950 code object of both files (llvm-objdump --offloading, as tests/test_cabi.py does), disassembles them and reports,
per kernel symbol, whether the instruction stream (mnemonics, operands and encodings; load addresses are dropped) is identical, and
the VGPR / AGPR / SGPR counts, LDS size, private_segment_fixed_size and spill counts of the code object's notes.  Device functions
that were not inlined are compared like kernels, without metadata.  Exit status 1 when a symbol exists on one side only or anything
differs.  -v prints a unified diff of each differing stream.  CPU only."""
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout


def load(path):
    """{symbol: (instruction lines, metadata dict or None)} over all gfx950 code objects of `path`"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "bin")  # llvm-objdump --offloading extracts next to its input
        shutil.copy(path, f)
        run(f"{LLVM}/llvm-objdump", "--offloading", f)
        objs = sorted(glob.glob(f + ".*gfx950"))
        if not objs:
            sys.exit(f"{path}: no gfx950 code object")
        for o in objs:
            meta, rec = {}, {}
            for line in run(f"{LLVM}/llvm-readelf", "--notes", o).splitlines():
                m = re.match(r"  (- |  )\.(\w+):\s+(\S+)", line)  # a key of a kernel's record (its arguments' keys are indented deeper)
                if not m:
                    continue
                if m.group(1) == "- ":
                    rec = {}
                if m.group(2) in META:
                    rec[m.group(2)] = int(m.group(3))
                elif m.group(2) == "symbol":  # '<kernel>.kd'
                    meta[m.group(3).strip("'\"")[:-3]] = rec
            sym = None
            for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-leading-addr", o).splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
                if m:
                    sym = m.group(1)
                    while sym in out and out[sym][2] != o:  # same internal-linkage name in two translation units
                        sym += "'"
                    out[sym] = ([], meta.get(m.group(1)), o)
                elif sym and line.strip() and line.strip() != "...":  # "...": the zero fill up to the next symbol's alignment
                    out[sym][0].append(re.sub(r"//\s*[0-9A-Fa-f]+:\s*", "// ", line.strip()))
    return {k: (v[0], v[1]) for k, v in out.items()}


def main(argv):
    verbose = "-v" in argv
    argv = [a for a in argv if a != "-v"]
    renames, paths = {}, []
    while argv:
        arg = argv.pop(0)
        if arg == "--map":
            old, _, new = (argv.pop(0) if argv else "").partition("=")
            if not old or not new:
                sys.exit(__doc__)
            renames[old] = new
        else:
            paths.append(arg)
    if len(paths) != 2:
        sys.exit(__doc__)
    a, b = load(paths[0]), load(paths[1])
    for old, new in renames.items():
        if old not in a or new not in b:
            sys.exit(f"--map {old}={new}: {'A' if old not in a else 'B'} has no such symbol")
        ia, ma = a.pop(old)
        a[new] = ([line.replace(f"<{old}", f"<{new}") for line in ia], ma)  # branch targets are printed as <symbol+offset>
        print(f"A's {old} is compared with B's {new}")
    print(f"A = {paths[0]}: {len(a)} symbols, {sum(m is not None for _, m in a.values())} kernels")
    print(f"B = {paths[1]}: {len(b)} symbols, {sum(m is not None for _, m in b.values())} kernels")
    bad = 0
    for s in sorted(set(a) | set(b)):
        if s not in a or s not in b:
            print(f"ONLY IN {'A' if s in a else 'B'}  {s}")
            bad += 1
            continue
        (ia, ma), (ib, mb) = a[s], b[s]
        same = ia == ib and ma == mb
        bad += not same
        fmt = lambda m: "device function" if m is None else " ".join(f"{k.replace('_count', '').replace('_fixed_size', '')}={m.get(k, 0)}" for k in META)
        print(f"{'identical' if same else 'DIFFERENT'}  {len(ia)} instr  {fmt(ma)}  {s}")
        if not same:
            if ma != mb:
                print(f"    B: {fmt(mb)}")
            if ia != ib:
                print(f"    B: {len(ib)} instr")
                if verbose:
                    print("\n".join("    " + l for l in difflib.unified_diff(ia, ib, "A", "B", lineterm="", n=2)))
    print(f"{len(set(a) | set(b))} symbols compared, {bad} differ" if bad else f"all {len(a)} symbols identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
