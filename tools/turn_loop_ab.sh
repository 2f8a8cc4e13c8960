#!/bin/bash
# Round 18 (the queue kernel's turn loop): parent library against this tree's, dry-carry threshold by threshold.
#   usage (on a machine with the GPU): tools/turn_loop_ab.sh PARENT_TREE   -> $OUT (default prof_out/turn_loop/)
# PARENT_TREE is a built checkout of the parent commit (it runs under its own Python package; tools/launch_caps.py there must be this
# tree's).  Steps: --dump-outputs of both commands against the parent's, file for file; the alternating A/B (both orders, a fresh
# process per run); the counters of one group-sized launch, a profiler run of its own per variant with no tracing beside it.  Every
# GPU step runs under its own time limit and the script stops at the first one that fails.
# tools/turn_loop_summary.py turns the output into profiles/r18_turn_loop.json.
set -o pipefail
cd "$(dirname "$0")/.."
PARENT=$(realpath "$1")
HERE=$(pwd)
O=$(realpath -m "${OUT:-prof_out/turn_loop}")
REPS=${REPS:-6}
THRESHOLDS=${THRESHOLDS:-"0 4 8 16 32"}
mkdir -p $O
export TMPDIR=/tmp
BENCH="python3 bench.py --gpus 1 --workload rollout --no-cpu-baseline"
step() { # step SECONDS OUTFILE command...
  local t=$1 out=$2; shift 2
  timeout -k 10 $t "$@" > "$out" 2> "$out.err"
  local rc=$?
  if [ $rc -ne 0 ]; then echo "FAILED rc $rc: $*"; tail -20 "$out.err"; exit $rc; fi
}
variant() { # parent | bN: this tree with OAKGPU_MOVE_CARRY_DRY=N
  if [ "$1" = parent ]; then cd "$PARENT"; unset OAKGPU_MOVE_CARRY_DRY; else cd "$HERE"; export OAKGPU_MOVE_CARRY_DRY=${1#b}; fi
}
VARIANTS="parent"; for t in $THRESHOLDS; do VARIANTS="$VARIANTS b$t"; done
REVERSED=$(echo $VARIANTS | tr ' ' '\n' | tac | tr '\n' ' ')

# 1. outputs: both commands, parent against every threshold, file for file
D=$(mktemp -d)
for v in $VARIANTS; do
  variant $v
  step 200 $O/dump_default_$v.json $BENCH --dump-outputs $D/default_$v
  step 200 $O/dump_steps20_$v.json $BENCH --steps 20 --warmup 5 --dump-outputs $D/steps20_$v
done
: > $O/dump_compare.txt
for cmd in default steps20; do
  for v in $VARIANTS; do
    [ $v = parent ] && continue
    if diff -r $D/${cmd}_parent $D/${cmd}_$v > /dev/null; then echo "$cmd $v identical" >> $O/dump_compare.txt; else echo "$cmd $v DIFFERENT" >> $O/dump_compare.txt; fi
  done
done
cat $O/dump_compare.txt
rm -rf $D   # (the arrays are large: only the verdicts are kept)

# 2. speed: alternating, both orders, a fresh process per run
for rep in $(seq 0 $((REPS - 1))); do
  if [ $((rep % 2)) = 0 ]; then order=$VARIANTS; else order=$REVERSED; fi
  for v in $order; do
    variant $v
    step 120 $O/run_default_${v}_$rep.json $BENCH
    step 120 $O/run_steps20_${v}_$rep.json $BENCH --steps 20 --warmup 5
  done
  echo "rep $rep done"
done

# 3. counters of one launch that fills the device (1.31 M playouts, a group launch's size), a profiler run of its own per variant
export N=1310720
for v in ${PMC_VARIANTS:-parent b0 b8}; do
  variant $v
  step 400 $O/pmc_$v.log rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_THREAD_CYCLES_VALU SQ_WAVE_CYCLES --output-format csv -d $O/pmc_$v -- python3 tools/launch_caps.py 1000
  cp "$(find $O/pmc_$v -name '*counter_collection.csv' | head -1)" $O/pmc_$v.csv || exit 1
  rm -rf $O/pmc_$v
done
cd "$HERE"
echo "all done"
