"""Writes profiles/r07/pmc_summary.json and profiles/pmc_latest.json (what bench.py replays as roofline.traffic / roofline.issue,
keyed by the source hash of the kernels the counters were collected on) from SRC/pmc_<vehicle>_<task>_<FETCH_SIZE |
WRITE_SIZE | sq>/ (usage: summarize_profiles_r07.py SRC [NAME]: the directory the collection wrote, and the directory under profiles/ for the
summary, r07 unless given) -- the counter passes of
profiles/tools/collect_profiles_r06.sh, each in a run of its own without a tracing flag.
The first ten launches of a run are dropped (prof_cfg.py's pf_env_reset among them: with the fixed call shape it is another
instantiation than the steps)."""
import collections
import csv
import glob
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
name = sys.argv[2] if len(sys.argv) > 2 else "r07"  # (the directory under profiles/ the summary goes to)
src, dst = os.path.abspath(sys.argv[1]), os.path.join(R, "profiles", name)
os.makedirs(dst, exist_ok=True)


def counters(tag, skip, match="env_kernel"):
    out, meta = {}, {}
    for f in sorted(glob.glob(os.path.join(src, tag, "*", "*counter_collection.csv")), key=os.path.getmtime)[-1:]:  # (the newest run only)
        agg = collections.defaultdict(list)
        for r in csv.DictReader(open(f)):
            if match in r["Kernel_Name"] and int(r["Grid_Size"]) >= 64 * 64:
                agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
                meta = {k: r[k] for k in ("Kernel_Name", "Grid_Size", "Workgroup_Size", "VGPR_Count", "SGPR_Count", "LDS_Block_Size", "Scratch_Size")}
        for k, v in agg.items():
            v = v[skip:]
            out[k] = {"avg_per_launch": sum(v) / max(1, len(v)), "launches": len(v)}
    return out, meta


ALGO = {"hover": 330, "quadx_waypoints": 442, "fixedwing_waypoints": 418}
summary, latest = {}, {}
for env, (v, t) in {"hover": ("quadx", "hover"), "quadx_waypoints": ("quadx", "waypoints"), "fixedwing_waypoints": ("fixedwing", "waypoints")}.items():
    fetch, meta = counters(f"pmc_{v}_{t}_FETCH_SIZE", 10)
    write, _ = counters(f"pmc_{v}_{t}_WRITE_SIZE", 10)
    sq, _ = counters(f"pmc_{v}_{t}_sq", 10)
    if not fetch or not write or not sq:
        print("missing counters for", env)
        continue
    fe, wr = fetch["FETCH_SIZE"]["avg_per_launch"], write["WRITE_SIZE"]["avg_per_launch"]
    waves = sq["SQ_WAVES"]["avg_per_launch"]
    per_wave = {k[3:]: x["avg_per_launch"] / waves for k, x in sq.items() if k != "SQ_WAVES"}
    summary[env] = {
        "kernel": meta, "note": "rocprofv3 FETCH_SIZE / WRITE_SIZE are in KiB; on gfx950 FETCH_SIZE under-reports wide coalesced reads by 2x "
                                "(MI355X_MICROARCH.md, HBM section) -> doubled; separate --pmc passes, no tracing flags",
        "read_bytes_per_launch": 2 * fe * 1024, "write_bytes_per_launch": wr * 1024, "hbm_bytes_per_launch": (2 * fe + wr) * 1024,
        "algorithmic_bytes_per_launch": ALGO[env] * 65536, "per_wave_per_env_step": per_wave, "launches_averaged": fetch["FETCH_SIZE"]["launches"],
    }
    latest[env] = {"batch": 65536, "hbm_bytes_per_launch": (2 * fe + wr) * 1024, "valu_per_wave": per_wave.get("INSTS_VALU"),
                   "salu_per_wave": per_wave.get("INSTS_SALU"), "issue_slots_per_wave": per_wave.get("ACTIVE_INST_ANY"),
                   "clocks_per_inst": None}  # (see summarize_profiles_r06.py: SQ_WAVE_CYCLES under collection is not the product's wave life)
if len(latest) == 3:
    json.dump(summary, open(os.path.join(dst, "pmc_summary.json"), "w"), indent=1)
    import bench  # noqa: E402

    json.dump({"source_hash": bench.source_hash(), "source": f"profiles/{name}/pmc_summary.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE / SQ_*, separate passes, FETCH doubled per guide)",
               "envs": latest}, open(os.path.join(R, "profiles", "pmc_latest.json"), "w"), indent=1)
print(json.dumps(latest, indent=1))
