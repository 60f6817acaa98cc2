#!/usr/bin/env python3
"""Compare the function bodies of two `make -C cutesv_amd/csrc asm ASM_OUT=...` outputs (no GPU needed):
    python scripts/asm_bodies.py A.s B.s
A function runs from its `name:` label to `.Lfunc_endN`.  Comment lines and trailing `;` comments are dropped and every
`.L...` label becomes one token, so only instruction lines count.  Prints the functions present on one side only and those
whose instruction lines differ, with a unified diff; exit status 1 when anything was printed."""
import difflib
import re
import sys


def bodies(path):
    out, name, lines = {}, None, []
    for raw in open(path):
        line = raw.split(";", 1)[0].rstrip()
        if name is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):$", line)
            if m and not m.group(1).startswith(".L"):
                name, lines = m.group(1), []
        elif re.match(r"^\.Lfunc_end\d+:$", line):
            out[name], name = lines, None
        elif line.strip():
            lines.append(re.sub(r"\.L[\w$.]+", ".L", line.strip()))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    for side, only in ((sys.argv[1], sorted(set(a) - set(b))), (sys.argv[2], sorted(set(b) - set(a)))):
        for n in only:
            print("only in %s: %s" % (side, n))
    common = sorted(set(a) & set(b))
    differ = [n for n in common if a[n] != b[n]]
    for n in differ:
        print("differs: %s" % n)
        print("\n".join(difflib.unified_diff(a[n], b[n], sys.argv[1], sys.argv[2], lineterm="", n=1)))
    print("%d functions in %s, %d in %s; %d of %d common bodies identical" % (len(a), sys.argv[1], len(b), sys.argv[2], len(common) - len(differ), len(common)))
    return 1 if differ or set(a) ^ set(b) else 0


if __name__ == "__main__":
    sys.exit(main())
