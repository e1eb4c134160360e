#!/bin/bash
# Where the gain of the straight-line calm path came from: collect.sh OUT PARENT_LIB PARENT_TRACE_LIB NEW_TRACE_LIB, run from the
# repository root. `parent`: the parent commit's library through PF_LIB_PATH (the Python layer is the same); `new`: this tree's.
# The trace libraries are the -DPF_PHASE_TRACE variants of both (python __graft_entry__.py --variant out.so -DPF_PHASE_TRACE).
# Per side and task (Hover, QuadX-Waypoints), 200 eager env steps at 65 536 lanes (profiles/tools/prof_cfg.py), every run under its
# own time limit, the counter passes without a tracing flag, the script ending at the first run that fails:
#   two SQ counter passes (instruction counts; issue slots by kind), rocprofv3 --kernel-trace --stats, the phase trace.
# For the new side also the passes profiles/tools/summarize_profiles_r07.py reads (FETCH_SIZE, WRITE_SIZE, SQ_* of the three 65 536-lane
# configs): `summarize_profiles_r07.py OUT/new straight_step` then writes profiles/straight_step/pmc_summary.json and profiles/pmc_latest.json.
# profiles/tools/straight_step/summarize.py OUT prints the per-kernel table.
O=$(realpath -m "$1"); PARENT=$(realpath "$2"); TP=$(realpath "$3"); TN=$(realpath "$4"); R=$PWD
rm -rf "$O"; mkdir -p "$O/parent" "$O/new"; export TMPDIR=/tmp
A="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_INSTS_BRANCH"
B="SQ_WAVES SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_MISC SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_INSTS_SENDMSG"
SQ="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_LDS"
run() { timeout -k 10 170 "$@" || { echo "FAILED ($?): $*"; exit 1; }; }
cd /tmp
for side in parent new; do
  if [ $side = parent ]; then export PF_LIB_PATH=$PARENT; T=$TP; else unset PF_LIB_PATH; T=$TN; fi
  for t in hover waypoints; do
    export VEH=quadx TASK=$t STEPS=200
    run rocprofv3 --pmc $A --output-format csv -d $O/$side/${t}_a -- python $R/profiles/tools/prof_cfg.py > $O/$side/${t}_a.log 2>&1
    run rocprofv3 --pmc $B --output-format csv -d $O/$side/${t}_b -- python $R/profiles/tools/prof_cfg.py > $O/$side/${t}_b.log 2>&1
    run rocprofv3 --kernel-trace --stats --output-format csv -d $O/$side/${t}_kt -- python $R/profiles/tools/prof_cfg.py > $O/$side/${t}_kt.log 2>&1
    PF_LIB_PATH=$T run python $R/profiles/tools/phase_trace.py > $O/$side/phase_trace_${t}65536.txt 2> $O/$side/phase_trace_${t}.log
  done
done
unset PF_LIB_PATH STEPS
for e in quadx:hover quadx:waypoints fixedwing:waypoints; do
  export VEH=${e%%:*} TASK=${e##*:}
  for c in FETCH_SIZE WRITE_SIZE; do
    run rocprofv3 --pmc $c --output-format csv -d $O/new/pmc_${VEH}_${TASK}_$c -- python $R/profiles/tools/prof_cfg.py > /dev/null 2>&1
  done
  run rocprofv3 --pmc $SQ --output-format csv -d $O/new/pmc_${VEH}_${TASK}_sq -- python $R/profiles/tools/prof_cfg.py > /dev/null 2>&1
done
find $O -name "*.db" -delete; find $O -name "*agent_info.csv" -delete
echo "collected: $(ls $O/parent | wc -l) + $(ls $O/new | wc -l) entries"
