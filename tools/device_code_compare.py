#!/usr/bin/env python3
"""Compares the gfx950 device code of two trees, kernel by kernel.

    python tools/device_code_compare.py PARENT_ASM_DIR NEW_ASM_DIR [unit ...]

Each directory holds `<unit>.s` files made by

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S \
        -I acme_amd/csrc -I include acme_amd/csrc/<unit>.hip -o <unit>.s

A kernel is its instruction stream (labels renumbered in order of first appearance,
comments and blank lines dropped) and its `.amdhsa_*` block.  Prints one line per unit and
one line per kernel; a kernel that differs gets its resource figures at both sides.
"""
import os
import re
import sys

FIGURES = [("vgpr", "next_free_vgpr"), ("accum_offset", "accum_offset"), ("sgpr", "next_free_sgpr"),
           ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size")]


def parse(path):
    """{kernel symbol: (instruction lines, amdhsa lines, code bytes or None)}"""
    body, hsa, size = {}, {}, {}
    cur = inhsa = last = None  # function being read, its .amdhsa block, the one just ended
    for ln in open(path).read().split("\n"):
        m = re.match(r"^; codeLenInByte = (\d+)", ln)
        if m and last:  # the trailer of the function that ended last
            size[last], last = int(m.group(1)), None
        t = ln.split(";")[0].strip()
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if m:
            cur, last = m.group(1), None
            body[cur] = []
        elif t.startswith(".amdhsa_kernel"):
            inhsa = t.split()[1]
            hsa[inhsa] = []
        elif t == ".end_amdhsa_kernel":
            inhsa = None
        elif inhsa:
            if t:
                hsa[inhsa].append(t)
        elif t.startswith(".Lfunc_end"):
            cur, last = None, cur
        elif cur and t and (not t.startswith(".") or re.match(r"^\.L[\w$.]+:$", t)):
            body[cur].append(t)  # instructions and local labels; directives are dropped
    out = {}
    for k in hsa:  # kernels only: functions with an .amdhsa block
        names = {}

        def ren(m):
            return names.setdefault(m.group(0), ".L%d" % len(names))

        out[k] = ([re.sub(r"\.L[\w$.]+", ren, x) for x in body.get(k, [])], hsa[k], size.get(k))
    return out


def figures(k):
    d = {}
    for x in k[1]:
        p = x.split()
        if len(p) == 2:
            d[p[0].replace(".amdhsa_", "")] = p[1]
    return ", ".join("%s %s" % (n, d.get(key, "?")) for n, key in FIGURES) + ", code %s B" % k[2]


def main():
    pdir, ndir = sys.argv[1], sys.argv[2]
    units = sys.argv[3:] or sorted(f[:-2] for f in os.listdir(pdir) if f.endswith(".s"))
    issues = 0
    for u in units:
        a, b = parse(os.path.join(pdir, u + ".s")), parse(os.path.join(ndir, u + ".s"))
        gone, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        diff = [k for k in a if k in b and (a[k][0] != b[k][0] or a[k][1] != b[k][1])]
        issues += len(gone) + len(added) + len(diff)
        print("%s.s: parent %d kernels, new %d; gone %s; added %s; differing %d" %
              (u, len(a), len(b), gone, added, len(diff)))
        for k in sorted(a):
            if k not in b:
                continue
            if k not in diff:
                print("  identical (%d instructions, vgpr %s): %s" %
                      (len(a[k][0]), figures(a[k]).split(",")[0].split()[1], k))
            else:
                print("  DIFFERS: %s\n    parent: %s\n    new:    %s" % (k, figures(a[k]), figures(b[k])))
    print("TOTAL issues %d" % issues)
    return 1 if issues else 0


if __name__ == "__main__":
    sys.exit(main())
