#!/usr/bin/env python3
"""Where a kernel's SGPR spill traffic sits, by source region.

    tools/lane_spill_map.py FILE.s MANGLED_KERNEL_NAME REGIONS.txt

FILE.s is hipcc's -save-temps assembly of a build with -gline-tables-only (the .loc directives carry the source line of every
instruction; the machine code is the same as without them).  REGIONS.txt names source regions, one per line: `first last name`
(line numbers of hmm_kernel.hip, inclusive; the first region that holds a line wins).  For every region the tool prints the
static number of instructions, of v_readlane_b32 (reloads of spilled scalars), of v_writelane_b32 (spills), of s_nop and of
VALU instructions as a whole; `*` marks regions that are innermost loops (tools/isa_mix.py finds the loops the same way)."""
import collections
import re
import sys


def main():
    path, kernel, regions_path = sys.argv[1:4]
    regions = []
    for l in open(regions_path):
        p = l.split(None, 2)
        if len(p) == 3 and p[0].isdigit():
            regions.append((int(p[0]), int(p[1]), p[2].strip()))
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    main_file = None
    cur = (None, 0)
    tab = collections.OrderedDict((r[2], collections.Counter()) for r in regions)
    tab["(elsewhere)"] = collections.Counter()
    for l in lines[start + 1:end]:
        s = l.split(";")[0].strip()
        m = re.match(r"^\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            cur = (int(m.group(1)), int(m.group(2)))
            if main_file is None:
                main_file = cur[0]          # the kernel's first .loc is in its own file
            continue
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op = s.split(None, 1)[0]
        name = "(elsewhere)"
        if cur[0] == main_file:
            for a, b, n in regions:
                if a <= cur[1] <= b:
                    name = n
                    break
        c = tab[name]
        c["n"] += 1
        c["readlane"] += op == "v_readlane_b32"
        c["writelane"] += op == "v_writelane_b32"
        c["nop"] += op == "s_nop"
        c["valu"] += op.startswith("v_")
    print("%-28s %6s %9s %10s %6s %6s" % ("region", "instr", "readlane", "writelane", "s_nop", "VALU"))
    tot = collections.Counter()
    for name, c in tab.items():
        print("%-28s %6d %9d %10d %6d %6d" % (name, c["n"], c["readlane"], c["writelane"], c["nop"], c["valu"]))
        tot.update(c)
    print("%-28s %6d %9d %10d %6d %6d" % ("total", tot["n"], tot["readlane"], tot["writelane"], tot["nop"], tot["valu"]))


if __name__ == "__main__":
    main()
