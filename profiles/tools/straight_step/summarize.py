#!/usr/bin/env python3
"""summarize.py OUT: the per-kernel table of what profiles/tools/straight_step/collect.sh wrote -- per side (parent, new) and task, for
every instantiation of quadx_m0_env_kernel the run launched: dispatches and durations from the kernel trace, instructions and issue
slots per wave (median over the dispatches) from the two SQ counter passes, and the phase trace's lines."""
import collections
import csv
import glob
import os
import statistics
import sys

O = sys.argv[1]


def newest(pattern):
    fs = sorted(glob.glob(pattern, recursive=True), key=os.path.getmtime)
    return fs[-1] if fs else None


def per_wave(d):
    """{kernel: {counter: median over dispatches of value / waves}}"""
    f = newest(os.path.join(d, "**", "*counter_collection.csv"))
    by = collections.defaultdict(lambda: collections.defaultdict(dict))
    if not f:
        return {}
    for r in csv.DictReader(open(f)):
        if "quadx_m0_env_kernel" in r["Kernel_Name"] and int(r["Grid_Size"]) >= 64 * 64:
            by[r["Kernel_Name"]][r["Dispatch_Id"]][r["Counter_Name"]] = float(r["Counter_Value"])
    out = {}
    for k, disp in by.items():
        cols = collections.defaultdict(list)
        for c in disp.values():
            for name, v in c.items():
                if name != "SQ_WAVES" and c.get("SQ_WAVES"):
                    cols[name[3:]].append(v / c["SQ_WAVES"])
        out[k] = {name: statistics.median(v) for name, v in cols.items()}
        out[k]["dispatches"] = len(disp)
    return out


def short(k):
    return k[k.index("quadx_m0_env_kernel"):].split("(")[0]


for side in ("parent", "new"):
    for task in ("hover", "waypoints"):
        print(f"== {task} {side}")
        f = newest(os.path.join(O, side, f"{task}_kt", "**", "*kernel_trace.csv"))
        if f:
            dur = collections.defaultdict(list)
            for r in csv.DictReader(open(f)):
                if "quadx_m0_env_kernel" in r["Kernel_Name"]:
                    dur[r["Kernel_Name"]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            for k, v in dur.items():
                print(f"   {short(k)}: {len(v)} dispatches, duration median {statistics.median(v):.3f} us, mean {sum(v) / len(v):.3f}, min {min(v):.3f}")
        a, b = per_wave(os.path.join(O, side, f"{task}_a")), per_wave(os.path.join(O, side, f"{task}_b"))
        for k in b:
            g, h = b[k], a.get(k, {})
            print(f"   {short(k)}: per wave (median of {g['dispatches']} dispatches): issue slots SQ_ACTIVE_INST_ANY {g.get('ACTIVE_INST_ANY', 0):.0f} = VALU "
                  f"{g.get('ACTIVE_INST_VALU', 0):.0f} + scalar {g.get('ACTIVE_INST_SCA', 0):.0f} + misc {g.get('ACTIVE_INST_MISC', 0):.0f} + LDS {g.get('ACTIVE_INST_LDS', 0):.0f}"
                  f" + VMEM {g.get('ACTIVE_INST_VMEM', 0):.0f}; instructions: VALU {h.get('INSTS_VALU', 0):.0f}, SALU {h.get('INSTS_SALU', 0):.0f}, SMEM {h.get('INSTS_SMEM', 0):.0f}, "
                  f"branch {h.get('INSTS_BRANCH', 0):.0f}, LDS {h.get('INSTS_LDS', 0):.0f}, loads {h.get('INSTS_VMEM_RD', 0):.0f}, stores {h.get('INSTS_VMEM_WR', 0):.0f}")
        p = os.path.join(O, side, f"phase_trace_{task}65536.txt")
        if os.path.exists(p):
            print(f"   phase trace ({side}):")
            for l in open(p):
                if any(s in l for s in ("state unpacked", "resets done", "Aviary steps done", "obs row in LDS", "obs stores issued", "stores acknowledged", "slowest wave")):
                    print("     " + l.rstrip())
