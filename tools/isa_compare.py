#!/usr/bin/env python3
"""Compare two gfx950 listings of pt_render.hip kernel by kernel (CPU only).

usage: tools/isa_compare.py PARENT_DIR THIS_DIR [--diff SUBSTRING]

Each directory holds what tools/regcheck.sh leaves under $RC_OUT: k.s (the listing) and ru.txt (the
-Rpass-analysis=kernel-resource-usage remarks).  Per kernel, by demangled name: the verdict on its instruction
stream -- identical / same count and opcode histogram / differs -- with both instruction counts, and every
resource-usage figure that differs.  The instruction lines that differ are printed for the kernels whose demangled
name contains SUBSTRING (default: the product kernel, render_unidir_wf<false, 5, false>).
"""
import collections
import difflib
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True)
        return out.stdout.split("\n")[:len(names)]
    except (OSError, subprocess.CalledProcessError):
        return names


def kernels(path):
    """name -> instruction lines (comments and directives dropped) of every function of the listing"""
    out, cur, body = {}, None, None
    for l in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", l)
        if m and cur is None and not m.group(1).startswith(".L"):
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if l.startswith(".Lfunc_end"):
            out[cur] = body
            cur = None
            continue
        s = l.split(";")[0].strip()
        if s and not s.startswith(".") or re.match(r"^\.LBB\d+_\d+:", s):
            body.append(s)
    return out


def resources(path):
    out, cur = {}, None
    for l in open(path):
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark: \s*([^:\[]+?)(?: \[[^\]]*\])?: (\S+)", l)
        if cur and m:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def opcodes(body):
    return collections.Counter(s.split()[0] for s in body if not s.endswith(":"))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    want = "render_unidir_wf<false, 5, false>"
    if "--diff" in sys.argv:
        want = sys.argv[sys.argv.index("--diff") + 1]
        args.remove(want)
    pa, th = args
    ka, kb = kernels(pa + "/k.s"), kernels(th + "/k.s")
    ra, rb = resources(pa + "/ru.txt"), resources(th + "/ru.txt")
    names = sorted(set(ka) | set(kb))
    pretty = dict(zip(names, demangle(names)))
    tally = collections.Counter()
    for n in names:
        a, b = ka.get(n), kb.get(n)
        if a is None or b is None:
            verdict = "only in " + ("this" if a is None else "parent")
        elif a == b:
            verdict = "identical"
        elif len(a) == len(b) and opcodes(a) == opcodes(b):
            verdict = "same count and opcode histogram"
        else:
            verdict = "differs"
        tally[verdict] += 1
        ni = lambda x: "-" if x is None else str(sum(1 for s in x if not s.endswith(":")))
        print("%-32s %8s %8s  %s" % (verdict, ni(a), ni(b), pretty[n]))
        for k in sorted(set(ra.get(n, {})) | set(rb.get(n, {}))):
            va, vb = ra.get(n, {}).get(k), rb.get(n, {}).get(k)
            if va != vb:
                print("    %s: %s -> %s" % (k, va, vb))
        if a is not None and b is not None and a != b and want in pretty[n]:
            for d in difflib.unified_diff(a, b, "parent", "this", n=0, lineterm=""):
                print("    " + d)
    print("kernels: " + ", ".join("%d %s" % (v, k) for k, v in sorted(tally.items())))


if __name__ == "__main__":
    main()
