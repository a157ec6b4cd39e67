#!/usr/bin/env python3
"""Compare the device code of two builds of libisx, kernel by kernel (no GPU needed).

usage: tools/isa_diff.py [-v] DIR_A DIR_B

DIR_A and DIR_B are directories left by `tools/isa_stats.py --keep DIR`.  Each kernel's text is taken as isa_stats.kernels()
splits it, `;` comments and blank lines are stripped (names of inlined helpers show up in basic-block comments), and the
per-build symbol __hip_cuid_* is ignored (docs/LOG.md section 27.1).  Per kernel one verdict:
  identical   the same lines in the same order
  reordered   the same multiset of mnemonics, differing operands or order (register names, the place of an instruction)
  different   anything else, a kernel that only one build has included
-v prints a unified diff of every kernel that is not identical.  Exit status 1 if any kernel is "different".
Nothing but equality between the two builds is looked at.
"""
import collections
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_stats  # noqa: E402

ISA = "isx_api-hip-amdgcn-amd-amdhsa-gfx950.s"


def stripped(body):
    out = []
    for line in body.splitlines():
        line = line.split(";", 1)[0].strip()
        if line and "__hip_cuid_" not in line:
            out.append(re.sub(r"\s+", " ", line))
        if line == ".end_amdhsa_kernel":   # (behind the last kernel: the file's trailer, every kernel's metadata)
            break
    return out


def mnemonics(lines):
    # (labels and directives count as themselves: a changed block structure or a changed .amdhsa_ value is "different")
    return collections.Counter(l if l.endswith(":") or l.startswith(".") else l.split(" ", 1)[0] for l in lines)


def load(d):
    return {name: stripped(body) for name, body in isa_stats.kernels(os.path.join(d, ISA))}


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = load(args[0]), load(args[1])
    count = collections.Counter()
    for name in list(a) + [n for n in b if n not in a]:
        la, lb = a.get(name), b.get(name)
        if la == lb:
            verdict = "identical"
        elif la is not None and lb is not None and mnemonics(la) == mnemonics(lb):
            verdict = "reordered"
        else:
            verdict = "different"
        count[verdict] += 1
        if verdict != "identical":
            hunks = list(difflib.unified_diff(la or [], lb or [], args[0], args[1], n=2, lineterm=""))[2:]
            moved = sum(1 for l in hunks if l[:1] in "+-")
            print("%-44s %s (%d lines of %d / %d differ)" % (name, verdict, moved, len(la or []), len(lb or [])))
            if verbose:
                print("\n".join(hunks))
    print("%d identical, %d reordered, %d different" % (count["identical"], count["reordered"], count["different"]))
    sys.exit(1 if count["different"] else 0)


if __name__ == "__main__":
    main()
