#!/usr/bin/env python3
"""Are the kernels of two device-only assemblies of one .hip source the same code? usage: tools/kisa_same.py A.s B.s [name filter]
(A.s, B.s: what KEEP_ASM=A.s tools/kregs.sh FILE.hip leaves). Compares, kernel by kernel, the ISA text between the kernel's label and its descriptor, with the
function number taken out of the local labels (.LBB<n>_<m>: n follows the emission order), and the .amdhsa_ fields of its descriptor. Prints the
kernels that differ or are in one file only, then a count; exit status 0 iff every kernel is in both and none differs."""
import re
import sys


def kernels(path, flt):
    """name -> (ISA text, descriptor fields) of the kernels whose name holds flt"""
    out, name, part = {}, None, 0                   # part 1: in the ISA text of `name`, 2: in its descriptor
    for ln in open(path):
        m = re.match(r"(\S+):\s*; @(\S+)$", ln)
        if m and m.group(1) == m.group(2):
            name, part = m.group(1), 1
            out[name] = ([], [])
        elif name and ln.strip() == ".amdhsa_kernel " + name:
            part = 2
        elif name and ln.strip() == ".end_amdhsa_kernel":
            name, part = None, 0
        elif part:
            out[name][part - 1].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*$", "", ln)))       # (comments name loops by function number too)
    return {k: ("".join(a), "".join(b)) for k, (a, b) in out.items() if b and flt in k}


def main():
    a, b = (kernels(p, sys.argv[3] if len(sys.argv) > 3 else "") for p in sys.argv[1:3])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in %s: %s" % (sys.argv[1] if name in a else sys.argv[2], name))
        elif a[name][0] != b[name][0]:
            print("ISA differs: %s" % name)
        elif a[name][1] != b[name][1]:
            print(".amdhsa fields differ: %s" % name)
        else:
            continue
        bad += 1
    print("%d kernels in %s, %d in %s, %d differ or are missing" % (len(a), sys.argv[1], len(b), sys.argv[2], bad))
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(main())
