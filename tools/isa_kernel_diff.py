#!/usr/bin/env python3
"""Per-kernel companion of tools/isa_diff.sh: which kernels of ONE source file changed between two device listings.
usage: isa_kernel_diff.py <parent.s> <tree.s>    (hipcc <the Makefile's FLAGS> -S --cuda-device-only file.hip -o file.s)
A kernel = its body (label .. .Lfunc_end) plus its .amdhsa_kernel descriptor block; comments are dropped and the
per-function numbers of block labels (.LBB<n>_, .Lfunc_end<n>: they shift when a kernel is added or removed ahead) are
masked.  Prints same / DIFF / NEW / GONE per symbol; exits non-zero if a symbol named on the command line (substring,
mangled) is not `same`:  isa_kernel_diff.py a.s b.s k_rulebookILi1ELb0"""
import re
import sys


def kernels(path):
    out, cur, desc = {}, None, None
    for line in open(path):
        s = line.strip()
        if s.startswith(";") or not s:
            continue
        line = re.sub(r"\s*;.*$", "", line.rstrip("\n"))
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line)
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
        if cur is not None:
            out.setdefault(cur, []).append(line)
            if s.startswith(".Lfunc_end") and s.endswith(":"):
                cur = None
        m = re.match(r"\.amdhsa_kernel (\S+)", s)
        if m:
            desc = m.group(1)
        if desc:
            out.setdefault(desc, []).append(line)
        if s == ".end_amdhsa_kernel":
            desc = None
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    must, bad = sys.argv[3:], 0
    for k in sorted(set(a) | set(b)):
        state = "NEW " if k not in a else "GONE" if k not in b else "same" if a[k] == b[k] else "DIFF"
        print(state, len(a.get(k, [])), len(b.get(k, [])), k)
        bad += state != "same" and any(m in k for m in must)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
