#!/bin/bash
# A/B timing of plugin variants on ONE box, interleaved: tools/ab.sh "<bench args>" variant1 variant2 ... ("" = product build)
RESULTS=${RESULTS:-bench_out}; mkdir -p "$RESULTS"      # the runs' lines and logs
ARGS="$1"; shift
for round in 1 2; do
  for v in "$@"; do
    name=${v:-product}
    SB_LIB_VARIANT=$v python bench.py --full $ARGS --no-cpu-baseline --no-parity --allow-stale-traffic > $RESULTS/ab_${name}_r${round}.json 2> $RESULTS/ab_${name}_r${round}.err
    python tools/show_bench.py $RESULTS/ab_${name}_r${round}.json | head -3
  done
done
