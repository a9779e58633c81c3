#!/usr/bin/env python3
"""Compare two builds' device assembly kernel by kernel (a text comparison).

  hipcc <Makefile FLAGS> --cuda-device-only -S csrc/<file>.hip -o <file>.s   (as tools/isa.sh)
  python3 tools/isa_same.py --a old/*.s --b new/*.s [--stats]

Kernels are matched by mangled name over all files of a side.  Compared per
kernel: the instruction text from its label to its function end, without
comments and with the per-file function numbers of the .LBB<n>_ / .Lfunc_end<n>
labels dropped, and its .amdhsa_* block.  Prints the names that differ or exist
on one side only, and the counts; --stats adds, for those, VGPRs, accum offset,
SGPRs, LDS bytes, scratch bytes and the instruction count of each side.
Exit status 1 if anything differs.
"""
import argparse
import re
import sys

NUM = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI)\d+")
FIELDS = ["next_free_vgpr", "accum_offset", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size"]


def kernels(paths):
    """{name: (code lines, {amdhsa field: value})} of every .amdhsa_kernel in the files"""
    out = {}
    for path in paths:
        lines = [NUM.sub(r".\1", ln.split(";")[0].strip()) for ln in open(path)]
        lines = [ln for ln in lines if ln]
        start = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":") and not ln.startswith(".")}
        for i, ln in enumerate(lines):
            if not ln.startswith(".amdhsa_kernel "):
                continue
            name = ln.split()[1]
            hsa = dict(f[len(".amdhsa_"):].split(None, 1) for f in lines[i + 1:lines.index(".end_amdhsa_kernel", i)])
            b = start[name]
            e = next(j for j in range(b + 1, len(lines)) if lines[j] == ".Lfunc_end:" or lines[j].startswith(".section"))
            code = lines[b + 1:e]
            if name in out:
                sys.exit("%s: kernel %s is defined twice on this side" % (path, name))
            out[name] = (code, hsa)
    return out


def stats(k):
    code, hsa = k
    n = sum(1 for ln in code if not ln.endswith(":") and not ln.startswith("."))
    return " ".join("%s=%s" % (f, hsa.get(f, "-")) for f in FIELDS) + " instructions=%d" % n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--stats", action="store_true")
    args = ap.parse_args()
    A, B = kernels(args.a), kernels(args.b)
    only = sorted(set(A) ^ set(B))
    diff = sorted(n for n in set(A) & set(B) if A[n] != B[n])
    for n in only:
        print("only in %s: %s" % ("a" if n in A else "b", n))
        if args.stats:
            print("    " + stats(A[n] if n in A else B[n]))
    for n in diff:
        what = [w for w, i in (("code", 0), ("amdhsa", 1)) if A[n][i] != B[n][i]]
        print("differs (%s): %s" % (", ".join(what), n))
        if args.stats:
            print("    a: %s\n    b: %s" % (stats(A[n]), stats(B[n])))
    print("%d kernels in a, %d in b, %d on one side only, %d different" % (len(A), len(B), len(only), len(diff)))
    return 1 if only or diff else 0


if __name__ == "__main__":
    sys.exit(main())
