"""The paths the adaptive code is off, parent commit's library against this build's, on one MI355X (cfg2):
bench.py's default line, the untracked 4 x 16 progression (tools/noise_bench.py --untracked-only) and the tracked
4 x 16 progression (tools/adaptive_bench.py --uniform-only), each in a process of its own with RT_HIP_LIB naming
the library, alternating parent / this build round by round.

  python tools/adaptive_parent_ab.py --parent PATH/librt_hip.so [--rounds 4] [--regs regs.json]
                                     [--out profiles/adaptive_parent_ab.json]

--regs: a JSON file of tools/kernel_regs.py figures of both builds, copied into the result as it is.
A step that fails or runs past its limit ends the run: nothing more is started on the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, lib, limit):
    env = dict(os.environ)
    if lib:
        env["RT_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, *cmd], cwd=REPO, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"{cmd} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--regs", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adaptive_parent_ab.json"))
    a = ap.parse_args()
    libs = {"parent": os.path.abspath(a.parent), "pr": ""}
    res = {"what": "bench.py --gpus 1 --steps 5 --warmup 2, the untracked 4 x 16 progression (noise_bench.py --untracked-only "
                   "--prog-reps 3) and the tracked 4 x 16 progression (adaptive_bench.py --uniform-only --rounds 3), cfg2 "
                   f"1920x1080 x 64 spp x 8 bounces, parent library and this build alternating, {a.rounds} rounds, one MI355X",
           "bench_ms_per_step": {k: [] for k in libs}, "untracked_4x16_ms": {k: [] for k in libs},
           "tracked_4x16_ms": {k: [] for k in libs}, "build": {}}
    tmp = tempfile.mkdtemp()
    for _ in range(a.rounds):
        for name, lib in libs.items():
            out = run(["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"], lib, 240)
            line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            res["bench_ms_per_step"][name].append(line["ms_per_step"])
            res["build"][name] = line.get("build")
            f = os.path.join(tmp, "u.json")
            run(["tools/noise_bench.py", "--untracked-only", "--prog-reps", "3", "--out", f], lib, 240)
            res["untracked_4x16_ms"][name].append(json.load(open(f))["progression_4x16"]["untracked_ms"])
            run(["tools/adaptive_bench.py", "--uniform-only", "--rounds", "3", "--out", f], lib, 240)
            res["tracked_4x16_ms"][name].append(json.load(open(f))["tracked_uniform_4x16_ms"])
    for key in ("bench_ms_per_step", "untracked_4x16_ms", "tracked_4x16_ms"):
        summary = {}
        for name in libs:
            v = np.asarray(res[key][name], np.float64).reshape(-1)
            summary[name] = {"median": round(float(np.median(v)), 3), "min": float(v.min()), "max": float(v.max()),
                             "spread": round(float(v.max() - v.min()), 3)}
        summary["pr_median_minus_parent"] = round(summary["pr"]["median"] - summary["parent"]["median"], 3)
        summary["inside_parent_range"] = bool(summary["parent"]["min"] <= summary["pr"]["median"] <= summary["parent"]["max"])
        res[key + "_summary"] = summary
    if a.regs:
        res["kernel_regs"] = json.load(open(a.regs))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k.endswith("_summary")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
