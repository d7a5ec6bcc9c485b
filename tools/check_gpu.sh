#!/bin/bash
# GPU check: the GPU suite, smoke, then (SWEEP=1) the cfg5 replica sweep on one GPU (the
# N = 8 share and the whole sweep, with their parity checks) and (REHEARSE=1) a two-rank
# torchrun rehearsal of the N > 1 line (gloo, both ranks on GPU 0) with its strong_cfg4
# object. Results under $OUT (default bench_out/).
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || { tail -40 "$OUT/pytest_gpu.log"; exit 1; }
tail -1 "$OUT/pytest_gpu.log"
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.log" 2>&1 || { tail -20 "$OUT/smoke.log"; exit 1; }
tail -1 "$OUT/smoke.log"
if [ -n "$SWEEP" ]; then
  timeout -k 10 300 python -u bench.py --full --config cfg5sweep --sim-world 8 --steps 1 --warmup 1 --no-cpu-baseline > "$OUT/sweep_sim8.json" 2> "$OUT/sweep_sim8.err" || { tail -20 "$OUT/sweep_sim8.err"; exit 1; }
  cat "$OUT/sweep_sim8.json"
  timeout -k 10 400 python -u bench.py --full --config cfg5sweep --steps 1 --warmup 0 > "$OUT/sweep_1gpu.json" 2> "$OUT/sweep_1gpu.err" || { tail -20 "$OUT/sweep_1gpu.err"; exit 1; }
  cat "$OUT/sweep_1gpu.json"
fi
if [ -n "$REHEARSE" ]; then
  RT_BENCH_DEVICE_MOD=1 RT_BENCH_BACKEND=gloo timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --full --gpus 2 --steps 1 --warmup 1 --no-stats --no-roofline-pass > "$OUT/rehearse_n2.json" 2> "$OUT/rehearse_n2.err" || { tail -30 "$OUT/rehearse_n2.err"; exit 1; }
  cat "$OUT/rehearse_n2.json"
fi
