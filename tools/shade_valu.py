#!/usr/bin/env python3
"""Static VALU of the shading pass by section, from a PT_SEC_MARKERS listing.

    hipcc <the Makefile's compile line for pt_render.hip> -DPT_SEC_MARKERS --cuda-device-only -S -o marked.s
    tools/shade_valu.py marked.s [kernel-regex]

For the product instance (render_unidir_wf<false,5,false> unless a regex of the mangled name is given) it prints, per
section, the `v_` instructions that follow the section's marker in listing order up to the next marker, how many of
them are `v_mov`, how many are the IEEE division / square-root helpers (v_div_*, v_sqrt_*, v_rcp_*), and the
`s_*_saveexec` levels.  "(walk)" is everything before the first marker: the walk loop and the kernel's prologue.

Limit, printed with the table: the compiler places basic blocks freely, so a section's cold blocks may sit under a
later marker and a marker's range may hold another section's tail; the borders are blurred by a few tens of
instructions.  The kernel total is exact.  Counts are static: multiply by the section execution counts of a counting
run (PT_SECTION_DUMP) for an estimate of issued VALU.
"""
import collections
import re
import sys

DEFAULT = r"^_ZN12_GLOBAL__N_116render_unidir_wfILb0ELi5ELb0EEEvNS_4ArgsE:"


def sections(path, kernel=DEFAULT):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(kernel, l))
    order, cnt = ["(walk)"], collections.defaultdict(collections.Counter)
    sec, seen = "(walk)", collections.Counter()
    for l in lines[start + 1:]:
        s = l.strip()
        if s.startswith(".Lfunc_end") or s.startswith("s_endpgm"):
            break
        m = re.match(r"; SEC (SEC_\w+)", s)
        if m:   # an inlined section has one marker per copy: "BEGIN", "BEGIN#2", ...
            seen[m.group(1)] += 1
            sec = m.group(1)[4:] + ("#%d" % seen[m.group(1)] if seen[m.group(1)] > 1 else "")
            order.append(sec)
            continue
        c = cnt[sec]
        if s.startswith("v_"):
            op = s.split()[0]
            c["valu"] += 1
            if op.startswith("v_mov"):
                c["mov"] += 1
            if op.startswith(("v_div_", "v_sqrt_", "v_rcp_", "v_rsq_")):
                c["div"] += 1
            if op.endswith("_f64") or "_f64_" in op:
                c["f64"] += 1
        elif re.match(r"s_\w+_saveexec", s):
            c["saveexec"] += 1
        elif s.startswith("s_cbranch"):
            c["branch"] += 1
    return order, cnt


def main():
    path = sys.argv[1]
    kernel = sys.argv[2] if len(sys.argv) > 2 else DEFAULT
    order, cnt = sections(path, kernel)
    print("%-12s %6s %6s %8s %5s %9s %7s" % ("section", "VALU", "v_mov", "div/sqrt", "f64", "saveexec", "branch"))
    tot = collections.Counter()
    for k in order:
        c = cnt[k]
        tot.update(c)
        print("%-12s %6d %6d %8d %5d %9d %7d" % (k, c["valu"], c["mov"], c["div"], c["f64"], c["saveexec"], c["branch"]))
    print("%-12s %6d %6d %8d %5d %9d %7d" % ("total", tot["valu"], tot["mov"], tot["div"], tot["f64"], tot["saveexec"],
                                            tot["branch"]))
    it = ("BOUNCE", "LIGHT", "COSINE", "PROBE", "BEGIN", "DEAD", "SAMPLE_END")
    print("the sections a shading iteration runs, one copy each (%s): VALU %d, v_mov %d" %
          (" ".join(it), sum(cnt[k]["valu"] for k in it), sum(cnt[k]["mov"] for k in it)))
    print("limit: block placement blurs the section borders (a section's cold blocks may be listed under a later\n"
          "marker); the total is exact, the per-section figures are good to a few tens of instructions.")


if __name__ == "__main__":
    main()
