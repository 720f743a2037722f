#!/usr/bin/env python3
"""Compare the device code of two builds of a csrc file kernel by kernel, by symbol (no GPU needed):

    hipcc <build.FLAGS> --cuda-device-only -S old/downstream.hip -o old.s     (and the same for the new tree)
    tools/isa_kernel_bodies.py old.s new.s

A kernel's body is what stands between its label and its .Lfunc_end, less comment and directive lines, so that a
reordering of the instantiations in the file or a changed line number does not show.  Prints the symbols only one side
has and a unified diff of every body that differs; exit status 0 and "identical" when there is neither."""
import difflib
import re
import sys


def bodies(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name = m.group(1)
            out[name] = []
        elif name and line.startswith(".Lfunc_end"):
            name = None
        elif name:
            code = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip())   # (block labels count the functions)
            if code.strip() and (code.startswith(".LBB_") or not code.lstrip().startswith(".")):
                out[name].append(code)
    return out


def main(old, new):
    a, b = bodies(old), bodies(new)
    bad = 0
    for s in sorted(set(a) ^ set(b)):
        print("only in %s: %s" % (old if s in a else new, s))
        bad += 1
    for s in sorted(set(a) & set(b)):
        if a[s] != b[s]:
            sys.stdout.write("\n".join(difflib.unified_diff(a[s], b[s], "old " + s, "new " + s, lineterm="", n=2)) + "\n")
            bad += 1
    print("%s vs %s: %d kernels, %s" % (old, new, len(a), "identical" if not bad else "%d differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
