#!/usr/bin/env python3
"""Static instruction count of one path through a kernel in a device assembly file: path_count.py file.s <mangled-name-prefix> N[xK],N,...
N is the number of a block label (.LBB<f>_N; `entry` for the code in front of the first label); a block is everything from its label to
the next label, as in profiles/tools/r06/isa_blocks.py (which prints the blocks to choose from). NxK counts block N K times (a loop
body). Prints each block's instructions and branch targets, so that the path can be checked against the listing, and the sum."""
import re
import sys

path, name, spec = sys.argv[1], sys.argv[2], sys.argv[3]
lines = open(path, errors="replace").read().split("\n")
start = [i for i, l in enumerate(lines) if l.startswith(name) and ":" in l and not l.startswith("\t")][0]
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
blocks, cur = {"entry": [0, []]}, "entry"
for l in lines[start + 1:end]:
    m = re.match(r"^\.LBB\d+_(\d+):", l)
    if m:
        cur = m.group(1)
        blocks[cur] = [0, []]
        continue
    t = l.strip()
    if not t or t[0] in ";.":
        continue
    blocks[cur][0] += 1
    if t.startswith(("s_cbranch", "s_branch")):
        blocks[cur][1].append(t.split()[0][2:] + ">" + t.split()[1].rsplit("_", 1)[-1])
total = 0
for item in spec.split(","):
    b, _, k = item.partition("x")
    n, br = blocks[b]
    total += n * int(k or 1)
    print(f"  {b:>6s} {n:5d}" + (f" x{k}" if k else "   ") + "  " + " ".join(br))
print(f"path: {total} instructions")
