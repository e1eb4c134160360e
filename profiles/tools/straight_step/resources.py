#!/usr/bin/env python3
"""resources.py parent.s new.s: registers, scratch, LDS and static instructions of the sixteen one-step instantiations of
quadx_m0_env_kernel (Hover / Waypoints x Philox / noise off x one / two waves per SIMD x general / fixed), parent and new side by
side, from the device assembly of both builds (compile_hip(.., keep_asm=...) in __graft_entry__.py): the kernels' .amdhsa_ directives,
what -Rpass-analysis=kernel-resource-usage reports."""
import re
import sys


def kernels(path):
    lines = open(path, errors="replace").read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_ZN2pf19quadx_m0_env_kernelILi(\d)ELi(\d)ELi64ELi0ELb1ELb0ELb0ELi(\d)ELb(\d)E\w*):", lines[i])
        if not m:
            i += 1
            continue
        name, n = m.group(1), 0
        i += 1
        while not lines[i].strip().startswith("s_endpgm"):
            t = lines[i].strip()
            n += bool(t) and t[0] not in ";." and not t.endswith(":")
            i += 1
        d = {"insts": n + 1}
        while not lines[i].strip().startswith(".end_amdhsa_kernel"):
            mm = re.match(r"\s*\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size|group_segment_fixed_size|next_free_sgpr)\s+(\d+)", lines[i])
            if mm:
                d[mm.group(1)] = int(mm.group(2))
            i += 1
        out[tuple(int(m.group(k)) for k in (2, 3, 4, 5))] = d
    return out


def fmt(d):
    total, arch = d["next_free_vgpr"], d["accum_offset"]
    return f"{total:3d} registers ({max(0, total - arch):3d} AGPR) {d['private_segment_fixed_size']:3d} B scratch {d['group_segment_fixed_size']:5d} B LDS {d['insts']:6d} instructions"


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
print("task noise WPS shape :: parent | new   (registers = VGPR + AGPR; scratch per lane; LDS per workgroup; static instructions of the kernel)")
TASKS, NOISES = {1: "Hover", 2: "Waypoints", 3: "MA-Hover"}, {0: "noise off", 1: "injected", 2: "Philox"}
for sixteen in (True, False):  # the sixteen first, then the other one-step instantiations with the contact response (injected noise, the PettingZoo task)
    if not sixteen:
        print("the other one-step, mode-0, independent-lane instantiations (same source, not targets of the change):")
    for key in sorted(a):
        task, nz, wps, fixed = key
        if (task in (1, 2) and nz in (0, 2)) != sixteen:
            continue
        label = f"{TASKS[task]:9s} {NOISES[nz]:9s} WPS {wps} {'fixed' if fixed else 'general':7s}"
        print(f"{label} :: {fmt(a[key])} | {fmt(b[key]) if key in b else 'absent'}")
