"""What adaptive sampling costs and saves on one MI355X, cfg2 at 1920x1080, total 64, 8 bounces.

1. The stage kernels by the library's hook rt_device_adapt_kernel_ms (rt_adapt.hip), on the progression after
   two uniform passes of 16: k_adapt_tiles (tile map only), k_adapt_select, k_adapt_gather and k_adapt_scatter,
   each launch alone on the default stream between two HIP events, interleaved round by round; median of --reps
   after 2 warm-up rounds, at threshold 0 (every tile listed), with the achieved GB/s on each kernel's byte model
   (tiles: 32 B per pixel; select: 20 B per tile; gather: 44 B per listed pixel; scatter: 36 B per listed pixel).
2. Wall time of [16, 16] uniform passes followed by adaptive passes of 16 until none is active, with a device
   resolve at the end, at T = 0 (every tile in every pass) against the tracked uniform 4 x 16 progression of the
   same build, alternating, --rounds rounds. At T = 0 the final frames must be equal word for word: the pass over
   the tile-ordered pixel list, under the wave plan a full-size list gets, renders what the row-ordered pass does.
3. The same at the thresholds that leave about 50 % and 10 % of the tiles active after the two uniform passes
   (quantiles of the measured tile map): ms, samples rendered, Msamples/s of rendered samples.

4. Which kernel class moves: rt_device_kernel_timing (events around every k_trace / k_step / k_tail launch) over
   one tracked uniform 4 x 16 progression and over one [16, 16] + adaptive progression at T = 0, with the wall
   time of each timed run.

  python tools/adaptive_bench.py [--reps 20] [--rounds 4] [--out profiles/adaptive_bench.json]
  python tools/adaptive_bench.py --uniform-only [--rounds 3] --out FILE
      only the tracked uniform 4 x 16 progression (it runs on the parent commit's library too, RT_HIP_LIB=...:
      tools/adaptive_parent_ab.py)
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "sycl-ray-tracing_amd"), os.path.join(REPO, "tools"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

WARMUP = 2
STEP, TOTAL = 16, 64


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--uniform-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adaptive_bench.json"))
    a = ap.parse_args()
    import torch

    import bench
    import rt_amd
    from rt_amd import _capi

    P, sky, cam17 = bench.build_inputs("cfg2")
    _, _, _, w, h, spp, nb, _ = bench.CONFIGS["cfg2"]
    assert spp == TOTAL
    rk = rt_amd.RenderKernel(w, h, spp, nb, rt_amd.Image(w, h), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), rt_amd.Image.from_rgb(sky), None, device=0)
    rk.set_camera(rt_amd.Camera(cam17[:16], cam17[16]))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_px, n_tiles = w * h, ((h + 7) // 8) * ((w + 7) // 8)
    d_out = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
    res = {"what": f"cfg2 {w}x{h}, total {TOTAL}, {nb} bounces, passes of {STEP}, on one MI355X",
           "build": _capi.lib().rt_build_id().decode()}

    def start():
        rk.progress_begin()
        rk.progress_track_noise()

    if a.uniform_only:
        def tracked_uniform():
            start()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(TOTAL // STEP):
                rk.progress_advance(STEP, stream)
            rk.progress_resolve_device(d_out.data_ptr(), stream)
            torch.cuda.synchronize(dev)
            return round((time.perf_counter() - t0) * 1e3, 2)
        tracked_uniform()
        res["tracked_uniform_4x16_ms"] = [tracked_uniform() for _ in range(a.rounds)]
        rk.progress_end()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return 0

    # the tile map after [16, 16], for the quantile thresholds; the stage kernels on that state
    start()
    rk.progress_advance(STEP, stream)
    rk.progress_advance(STEP, stream)
    tile = rk.progress_noise(0.0, tile_map=True)["tile_err"].reshape(-1)
    fin = np.sort(tile[np.isfinite(tile)])
    thresholds = {"all": 0.0, "half": float(fin[len(fin) // 2]), "tenth": float(fin[(9 * len(fin)) // 10])}
    res["tile_map_after_2x16"] = {"tiles": n_tiles, "min": float(fin[0]), "median": thresholds["half"],
                                  "p90": thresholds["tenth"], "max": float(fin[-1])}
    rk.progress_advance_adaptive(STEP, 1e30)  # (no tile above it: nothing rendered, but the progression is adaptive now)
    reps = a.reps + WARMUP
    ms = np.zeros((4, reps), np.float64)
    act = np.zeros(2, np.int32)
    rc = rk.L.rt_device_adapt_kernel_ms(rk.ctx, ctypes.c_float(0.0), reps, rt_amd.ptr(ms), rt_amd.ptr(act))
    rt_amd.check(rk.L, rc, rk.ctx, "rt_device_adapt_kernel_ms")
    models = (("k_adapt_tiles", 32 * n_px), ("k_adapt_select", 20 * n_tiles), ("k_adapt_gather", 44 * int(act[1])),
              ("k_adapt_scatter", 36 * int(act[1])))
    res["kernels"] = {"how": "rt_device_adapt_kernel_ms at threshold 0: one launch between two events, four kernels "
                             "interleaved per round", "reps": a.reps, "warmup": WARMUP,
                      "listed_tiles": int(act[0]), "listed_pixels": int(act[1])}
    for k, (name, nbytes) in enumerate(models):
        m = ms[k, WARMUP:]
        med = float(np.median(m))
        res["kernels"][name] = {"ms": med, "ms_min": float(m.min()), "ms_max": float(m.max()), "bytes": nbytes,
                                "gbps": float(nbytes / (med * 1e-3) / 1e9)}

    def uniform_ms():
        start()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(TOTAL // STEP):
            rk.progress_advance(STEP, stream)
        rk.progress_resolve_device(d_out.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, TOTAL * n_px

    def adaptive_ms(threshold):
        start()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        rk.progress_advance(STEP, stream)
        rk.progress_advance(STEP, stream)
        samples, passes = 2 * STEP * n_px, []
        while True:
            i = rk.progress_advance_adaptive(STEP, threshold, stream)
            if i["active_tiles"] == 0:
                break
            samples += STEP * i["active_pixels"]
            passes.append(i["active_tiles"])
        rk.progress_resolve_device(d_out.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, samples, passes

    uniform_ms()  # warm-up: buffers sized, code objects loaded
    adaptive_ms(0.0)
    runs = {k: [] for k in ("uniform", *thresholds)}
    frames, info = {}, {}
    for _ in range(a.rounds):  # (alternating, so drift lands on all alike)
        t, s = uniform_ms()
        runs["uniform"].append(round(t, 2))
        info["uniform"] = (s, [n_tiles] * 4)
        frames["uniform"] = d_out.clone()
        for name, thr in thresholds.items():
            t, s, passes = adaptive_ms(thr)
            runs[name].append(round(t, 2))
            info[name] = (s, passes)
            if name == "all":
                frames["all"] = d_out.clone()
    ok = bool(torch.equal(frames["all"].view(torch.int32), frames["uniform"].view(torch.int32)))
    res["runs"] = {"what": f"wall-clock ms of the whole progression and its device resolve, {a.rounds} rounds alternating; "
                           "uniform: the tracked 4 x 16 progression of this build",
                   "frames_equal_at_threshold_0": ok}
    for name, t in runs.items():
        s, passes = info[name]
        med = float(np.median(t))
        res["runs"][name] = {"threshold": None if name == "uniform" else thresholds[name], "ms": t, "median_ms": round(med, 2),
                             "spread_ms": round(max(t) - min(t), 2), "samples": int(s),
                             "msamples_per_s": round(s / (med * 1e-3) / 1e6, 1), "active_tiles_per_pass": passes}
    res["runs"]["all_excess_over_uniform_ms"] = round(res["runs"]["all"]["median_ms"] - res["runs"]["uniform"]["median_ms"], 2)
    # 4: the kernel classes' GPU time, uniform against T = 0 (every launch between two events on its lane's stream)
    rk.L.rt_device_kernel_timing.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    kms, kn = np.zeros(3, np.float64), np.zeros(3, np.int64)
    timed = {}
    for name, fn in (("uniform", uniform_ms), ("all", lambda: adaptive_ms(0.0))):
        per = []
        for _ in range(a.rounds):
            rk.L.rt_device_kernel_timing(rk.ctx, 1, None, None)
            wall = fn()[0]
            torch.cuda.synchronize(dev)
            rk.L.rt_device_kernel_timing(rk.ctx, 0, rt_amd.ptr(kms), rt_amd.ptr(kn))
            per.append({"wall_ms": round(wall, 2), "k_trace_ms": round(float(kms[0]), 2), "k_step_ms": round(float(kms[1]), 2),
                        "k_tail_ms": round(float(kms[2]), 2), "launches": [int(v) for v in kn]})
        timed[name] = per
    med = lambda name, k: float(np.median([r[k] for r in timed[name]]))
    res["kernel_classes"] = {"how": "rt_device_kernel_timing: HIP events around every launch of a class on its lane's stream, "
                                    "summed over the lanes (they overlap, so the sums exceed the wall time)",
                             "runs": timed,
                             "all_minus_uniform_ms": {k: round(med("all", k) - med("uniform", k), 2)
                                                      for k in ("wall_ms", "k_trace_ms", "k_step_ms", "k_tail_ms")}}
    rk.progress_end()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
