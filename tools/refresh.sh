#!/bin/bash
# Measurement refresh (on a GPU): tools/refresh.sh TAG. Roofline profiles of the cfg2 1-lane
# command (trace, FETCH, WRITE, SQ/TCC counters) into $OUT/TAG_roof (OUT defaults to bench_out),
# traffic.json, the full cfg2 / cfg3 bench lines, and the strong-scaling shard probes (every rank).
set -o pipefail
T=${1:-r03}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
PMC_DETAIL=1 tools/profile_roofline.sh "$OUT/${T}_roof" --config cfg2 || exit 1
python3 tools/update_traffic.py "$OUT/${T}_roof" --build "$(cat BUILD_COMMIT 2>/dev/null)" --commit-dir profiles/${T}_roof || exit 1
cp profiles/traffic.json "$OUT/traffic.json"  # (then copy $OUT/${T}_roof to profiles/${T}_roof, the path it records)
timeout -k 10 300 python -u bench.py --full > "$OUT/${T}_bench_cfg2.json" 2> "$OUT/${T}_bench_cfg2.err" || exit 1
cat "$OUT/${T}_bench_cfg2.json"
timeout -k 10 300 python -u bench.py --full --config cfg3 > "$OUT/${T}_bench_cfg3.json" 2> "$OUT/${T}_bench_cfg3.err" || exit 1
if [ -n "$PROBES" ]; then
  for c in cfg2 cfg4 cfg5; do
    timeout -k 10 600 python -u tools/shard_probe.py --config $c --worlds 1,2,4,8 --reps 1 --all-ranks > "$OUT/${T}_probe_$c.log" 2>&1 || exit 1
    tail -1 "$OUT/${T}_probe_$c.log"
  done
fi
