#!/usr/bin/env python3
"""Order of global memory operations and vmcnt waits in every kernel, from the gfx950 assembly (no GPU needed).

usage: python tools/wait_order.py [--regs] [--full] [file.hip ...]      (default: every breakdancer_amd/csrc/*.hip)

Each .hip is compiled with the Makefile's flags for libbdx.so plus `--cuda-device-only -S`.  One line per kernel: its name
and, in program order, L for a global_load*, S for a global_store*, A for a global_atomic*, wN for an s_waitcnt that carries
vmcnt(N).  On gfx950 vmcnt counts stores as well as loads and retires in order, so a wN behind an S waits for that store's
acknowledgement too: an S in front of `L ... w0` puts a store's round trip into the chain of the load.  Program order is
not execution order (loops and branches are laid out once); the head of a line is the kernel's entry.
--regs adds .vgpr_count, .sgpr_count and the private segment (scratch) size from the code object's metadata;
--full prints whole sequences (default: the first 120 operations)."""
import argparse
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "breakdancer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("ARCH", "gfx950")
# HIPFLAGS of the Makefile (-fPIC only matters to the host half)
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-result", "-I" + os.path.join(ROOT, "include")]

OPS = (("global_load", "L"), ("global_store", "S"), ("global_atomic", "A"))
VMCNT = re.compile(r"vmcnt\((\d+)\)")
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def short(name):
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "").replace("bdx::", "")
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):  # the argument list is the first '(' outside the template arguments
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            cut = i
            break
    return name[:cut]


def kernels_of(asm):
    """-> [(symbol, sequence, meta)] in the file's order"""
    kernel_syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    want = set(kernel_syms)
    seqs, cur = {}, None
    for line in asm.split("\n"):
        m = LABEL.match(line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1) if m.group(1) in want else None
            if cur:
                seqs[cur] = []
            continue
        if cur is None:
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end") or s.startswith(".section"):
            cur = None
            continue
        for prefix, letter in OPS:
            if s.startswith(prefix):
                seqs[cur].append(letter)
                break
        else:
            if s.startswith("s_waitcnt"):
                w = VMCNT.search(s)
                if w:
                    seqs[cur].append("w" + w.group(1))
    meta = {}
    for block in re.split(r"^\s*- \.agpr_count:", asm, flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", block, re.M)
        if not name:
            continue
        get = lambda k: (re.search(r"^\s*\.%s:\s*(\d+)" % k, block, re.M) or [None, "?"])[1]
        meta[name.group(1)] = (get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"))
    return [(k, seqs.get(k, []), meta.get(k, ("?", "?", "?"))) for k in kernel_syms]


def fold(seq):
    """runs of one letter stay written out (LLLL): the picture is the point; only spaces between groups are added"""
    out, prev = [], None
    for t in seq:
        if t[0] == "w" or (prev is not None and prev[0] == "w"):
            out.append(" ")
        out.append(t)
        prev = t
    return "".join(out).strip()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--regs", action="store_true")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    files = a.files or sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    for f in files:
        r = subprocess.run([HIPCC] + FLAGS + ["--cuda-device-only", "-S", "-o", "-", f], capture_output=True, text=True)
        if r.returncode:
            sys.stderr.write(r.stderr)
            sys.exit("wait_order: %s does not compile" % f)
        ks = kernels_of(r.stdout)
        names = demangle([k for k, _, _ in ks])
        print("# " + os.path.relpath(f, ROOT))
        for sym, seq, (vgpr, sgpr, scratch) in ks:
            shown = seq if a.full else seq[:120]
            regs = "[vgpr %s sgpr %s scratch %s]  " % (vgpr, sgpr, scratch) if a.regs else ""
            print(("%-40s %s%s%s" % (short(names[sym]), regs, fold(shown), " ..." if len(shown) < len(seq) else "")).rstrip())


if __name__ == "__main__":
    main()
