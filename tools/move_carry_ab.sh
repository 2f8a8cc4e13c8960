#!/bin/bash
# Move carry of the queue kernel (oakgpu_set_move_carry): parent library against this tree's, threshold by threshold.
#   usage (on a machine with the GPU): tools/move_carry_ab.sh PARENT_TREE [PARENT_PROFILE_LIB]   -> $OUT (default prof_out/move_carry/)
# PARENT_TREE is a built checkout of the parent commit (its library has no oakgpu_set_move_carry, so it runs under its own Python
# package; tools/launch_caps.py there must be this tree's); the optional profile library is the parent built with
# -DOAKGPU_SITE_PROFILE (tools/site_profile.sh build) and this tree's per-pass exec_move sites.  Every GPU step runs under its own
# time limit and the script stops at the first one that fails; counters are collected in runs of their own.
# tools/move_carry_summary.py turns the output into profiles/r16_move_carry.json.
set -o pipefail
cd "$(dirname "$0")/.."
PARENT=$(realpath "$1")
PPROF=${2:+$(realpath "$2")}
HERE=$(pwd)
O=$(realpath -m "${OUT:-prof_out/move_carry}")
REPS=${REPS:-5}
THRESHOLDS=${THRESHOLDS:-"0 8 16 32 64"}
[ -n "$ONLY_PROFILES" ] || rm -rf $O   # (ONLY_PROFILES=1: keep the runs of an earlier call, take the profiles and counters only)
mkdir -p $O
export TMPDIR=/tmp
step() { # step SECONDS OUTFILE command...
  local t=$1 out=$2; shift 2
  timeout -k 10 $t "$@" > "$out" 2> "$out.err"
  local rc=$?
  if [ $rc -ne 0 ]; then echo "FAILED rc $rc: $*"; tail -20 "$out.err"; exit $rc; fi
}
variant() { # variant NAME -> the tree to run in, OAKGPU_MOVE_CARRY
  if [ "$1" = parent ]; then cd "$PARENT"; unset OAKGPU_MOVE_CARRY; else cd "$HERE"; export OAKGPU_MOVE_CARRY=${1#b}; fi
}
VARIANTS="parent"; for t in $THRESHOLDS; do VARIANTS="$VARIANTS b$t"; done
REVERSED=$(echo $VARIANTS | tr ' ' '\n' | tac | tr '\n' ' ')

if [ -z "$ONLY_PROFILES" ]; then
# 1. outputs: both commands, parent against every threshold, file for file
for v in $VARIANTS; do
  variant $v
  step 200 $O/dump_default_$v.json python3 bench.py --gpus 1 --workload rollout --no-cpu-baseline --dump-outputs $O/dump_default_$v
  step 200 $O/dump_steps20_$v.json python3 bench.py --gpus 1 --workload rollout --no-cpu-baseline --steps 20 --warmup 5 --dump-outputs $O/dump_steps20_$v
done
: > $O/dump_compare.txt
for cmd in default steps20; do
  for v in $VARIANTS; do
    [ $v = parent ] && continue
    if diff -r $O/dump_${cmd}_parent $O/dump_${cmd}_$v > /dev/null; then echo "$cmd $v identical" >> $O/dump_compare.txt; else echo "$cmd $v DIFFERENT" >> $O/dump_compare.txt; fi
  done
done
cat $O/dump_compare.txt
rm -rf $O/dump_*_b* $O/dump_*_parent   # (the arrays are large: only the verdicts travel back)

# 2. speed: alternating, both orders, a fresh process per run
for rep in $(seq 0 $((REPS - 1))); do
  if [ $((rep % 2)) = 0 ]; then order=$VARIANTS; else order=$REVERSED; fi
  for v in $order; do
    variant $v
    step 200 $O/run_default_${v}_$rep.json python3 bench.py --gpus 1 --workload rollout --no-cpu-baseline
    step 200 $O/run_steps20_${v}_$rep.json python3 bench.py --gpus 1 --workload rollout --no-cpu-baseline --steps 20 --warmup 5
  done
  echo "rep $rep done"
done
fi

# 3. region profile of one launch that fills the device (the driver command's 1.31 M playouts), per threshold; the parent's schedule first
export N=1310720
if [ -n "$PPROF" ]; then
  variant parent   # (the parent's library runs under the parent's Python package; tools/site_profile.py there must be this tree's)
  step 200 $O/site_parent.json python3 tools/site_profile.py "$PPROF"
fi
cd "$HERE"
for t in $THRESHOLDS; do
  export OAKGPU_MOVE_CARRY=$t
  step 200 $O/site_b$t.json python3 tools/site_profile.py prof_build/liboakgpu_prof.so
done
echo "site profiles done"

# 4. counters of the same launch, a profiler run of its own per variant
for v in $VARIANTS; do
  variant $v
  step 400 $O/pmc_$v.log rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_THREAD_CYCLES_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d $O/pmc_$v -- python3 tools/launch_caps.py 1000
  f=$(find $O/pmc_$v -name '*counter_collection.csv' | head -1)
  python3 - "$f" "$O/pmc_$v.log" > $O/pmc_$v.json <<'PY'
import collections, csv, json, re, sys
tot = collections.defaultdict(float)
for r in csv.DictReader(open(sys.argv[1])):
    if 'k_rollout_queue' in r['Kernel_Name']:
        tot[r['Counter_Name']] += float(r['Counter_Value'])
steps = int(re.search(r'steps (\d+)', open(sys.argv[2]).read()).group(1))
out = dict(tot)
out.update(turn_steps=steps, valu_per_turn_step=tot['SQ_INSTS_VALU'] / steps, salu_per_turn_step=tot['SQ_INSTS_SALU'] / steps,
           active_lanes_per_valu_inst=tot['SQ_THREAD_CYCLES_VALU'] / tot['SQ_INSTS_VALU'] if tot['SQ_INSTS_VALU'] else None)
print(json.dumps(out))
PY
  rm -rf $O/pmc_$v
  cat $O/pmc_$v.json
done
cd "$HERE"
echo "all done"
