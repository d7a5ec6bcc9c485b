#!/bin/bash
# The default bench line (with its roofline passes) N times in a row on one machine (run-to-run
# spread of the headline): tools/repeat_bench.sh [N]; results under $OUT (default bench_out/).
set -o pipefail
N=${1:-5}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for i in $(seq $N); do
  timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > "$OUT/rep_$i.json" 2> "$OUT/rep_$i.err" || exit 1
  python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print(d['value'], d['ms_per_step'], d['roofline']['frac'] if d.get('roofline') else None)" "$OUT/rep_$i.json"
done
