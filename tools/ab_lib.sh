#!/bin/bash
# dev helper: A/B library builds on the same box, alternating (headline step + forward sweep).  usage: ab_lib.sh repeats lib1.so lib2.so ...  ("-" = the default build)
# Stops at the first benchmark run that fails; a fault, an abort or a time limit (124, 134, 137, 139) ends the script with that status.
set -o pipefail
n=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
run() {
  if [ "$1" != "-" ]; then export SMG_HIP_LIB=$ROOT/$1; else unset SMG_HIP_LIB; fi
  out=$(timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --cpu-samples 0 --batched-scenes 0 --no-roofline --no-configs 2>/dev/null | tail -1)
  rc=$?
  [ $rc -eq 0 ] || return $rc
  echo "[$1] $(echo "$out" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(round(d['ms_per_step'],2), round(d.get('sweep_fwd_ms',0),2), d.get('train_step_ms'))")"
}
for i in $(seq $n); do
  for v in "$@"; do
    run "$v"; rc=$?
    if [ $rc -ne 0 ]; then echo "[$v] benchmark run failed with status $rc: stopping" >&2; exit $rc; fi
  done
done
