#!/bin/bash
# whole-step A/B on one box: bench.py per library build, alternating (ACATTN_LIB; "default" = the in-tree build)
# usage: tools/gpu_ab.sh <rounds> <lib|default> [<lib|default> ...] [-- <bench.py arguments>]
#   bench.py always gets --steps 300 --warmup 20; without a "--" part also --no-cpu-baseline
rounds=$1; shift
libs=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do libs+=("$1"); shift; done
if [ "$1" = "--" ]; then shift; else set -- --no-cpu-baseline; fi
logs=$(mktemp -d) || exit 1
echo "# bench.py output of the last run: $logs/ab_bench.log, $logs/ab_bench.err"
for r in $(seq "$rounds"); do
  for lib in "${libs[@]}"; do
    if [ "$lib" != "default" ]; then export ACATTN_LIB=$PWD/$lib; else unset ACATTN_LIB; fi
    timeout -k 10 300 python bench.py --steps 300 --warmup 20 "$@" > "$logs/ab_bench.log" 2> "$logs/ab_bench.err" || { echo "$lib failed"; tail -n 3 "$logs/ab_bench.err"; exit 1; }
    echo "$lib: $(tail -n 1 "$logs/ab_bench.log" | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["ms_per_step"], d["value"])')"
  done
done
