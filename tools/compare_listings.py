#!/usr/bin/env python3
"""Compare two device-assembly listings of one kernel unit kernel by kernel: tools/compare_listings.py A.s B.s

For listings made with the unit's Makefile flags plus `--cuda-device-only -S` (a refactor must leave them alike).
A kernel's text runs from its `.globl` line to its `.end_amdhsa_kernel` (instructions and the .amdhsa_* block).
The function index in local labels (.LBB<n>_, .Lfunc_end<n>, BB<n>_ and %bb.<n> in comments) is dropped, since it
changes when kernels are emitted in another order, and so are the lines naming the unit's __hip_cuid_<hash>.
Prints the kernels compared and every kernel that differs or is missing on one side; the lines outside kernels
(symbol sizes, metadata) are compared as a set. Exit status 1 if anything differs."""
import re
import sys


def kernels(path):
    out, rest, name, body = {}, [], None, []
    for line in open(path):
        if "__hip_cuid_" in line:
            continue
        line = re.sub(r"(\.?L?BB|\.Lfunc_(?:begin|end)|%bb\.)\d+", r"\1N", line)
        line = re.sub(r" +;", " ;", line)  # (a comment's column follows the label's width)
        if line.startswith("\t.globl\t"):  # (a global that is no kernel never ends one: its lines are outside)
            rest += body if name is not None else []
            name, body = line.split()[1], []
        (rest if name is None else body).append(line)
        if name is not None and line.startswith("\t.end_amdhsa_kernel"):
            out[name], name = body, None
    return out, rest + (body if name is not None else [])


a, rest_a = kernels(sys.argv[1])
b, rest_b = kernels(sys.argv[2])
bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
print(f"{sys.argv[1]}: {len(a)} kernels, {sum(map(len, a.values()))} lines; {sys.argv[2]}: {len(b)} kernels, "
      f"{sum(map(len, b.values()))} lines; {len(set(a) | set(b)) - len(bad)} identical")
for k in bad:
    print("DIFFERS" if k in a and k in b else "ONLY IN " + sys.argv[1 if k in a else 2], k)
outside = sorted(rest_a) != sorted(rest_b)
if outside:
    print("lines outside the kernels differ")
sys.exit(1 if bad or outside else 0)
