"""What the noise estimate of a tracked progression costs on one MI355X, cfg2 at 1920x1080.

1. k_noise_fold and k_noise_tiles (without and with the pixel map) by the library's hook
   rt_device_noise_kernel_ms (rt_noise.hip): each launch alone on the default stream between two HIP events
   recorded right before and after it, the three interleaved round by round; median of --reps after 2 warm-up
   rounds, with the achieved GB/s on each kernel's byte model (fold: 48 B per pixel; tiles: 32 B per pixel,
   36 with the pixel map). An event pair around one launch still holds the launch's fixed cost, as in
   tools/display_bench.py, whose k_display figures (profiles/display_bench.json) are quoted beside these.
2. The 4 x 16 progression of tools/progressive_bench.py (cfg2, 64 spp, 8 bounces; begin untimed, the passes
   and the final rt_progress_resolve_device timed, wall-clock ms around a device synchronize), tracked
   (rt_progress_noise_track after begin; a rt_progress_noise_device query after each pass from the second)
   against untracked on the same build, alternating. The tracked excess is reported as a share of the
   untracked time.

  python tools/noise_bench.py [--reps 20] [--prog-reps 5] [--untracked-only] [--out profiles/noise_bench.json]

--untracked-only: only the untracked 4 x 16 progression (it runs on a library without the noise calls too:
the A/B against the parent commit, RT_HIP_LIB=...).
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

KERNELS = (("k_noise_fold", 48), ("k_noise_tiles", 32), ("k_noise_tiles_pixel_map", 36))
WARMUP = 2
W, H = 1920, 1080


def stats(ms, bytes_per_pixel: int, n_px: int) -> dict:
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return {"ms": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()), "spread_ms": float(ms.max() - ms.min()),
            "bytes_per_pixel": bytes_per_pixel, "gbps": float(bytes_per_pixel * n_px / (med * 1e-3) / 1e9)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prog-reps", type=int, default=5)
    ap.add_argument("--untracked-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "noise_bench.json"))
    a = ap.parse_args()
    import torch

    import bench
    import rt_amd
    from rt_amd import _capi

    P, sky, cam17 = bench.build_inputs("cfg2")
    _, _, _, w, h, spp, nb, _ = bench.CONFIGS["cfg2"]
    assert (w, h) == (W, H)
    rk = rt_amd.RenderKernel(w, h, spp, nb, rt_amd.Image(w, h), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), rt_amd.Image.from_rgb(sky), None, device=0)
    rk.set_camera(rt_amd.Camera(cam17[:16], cam17[16]))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = w * h
    res = {"what": f"cfg2 {w}x{h} on one MI355X", "build": _capi.lib().rt_build_id().decode()}

    if not a.untracked_only:
        g = torch.Generator(device="cpu").manual_seed(0)
        d_state = (torch.rand((h, w, 4), generator=g) * 8.0).to(dev)
        d_half = (torch.rand((h, w, 4), generator=g) * 4.0).to(dev)
        d_px = torch.empty((h, w), dtype=torch.float32, device=dev)
        d_tl = torch.empty(((h + 7) // 8, (w + 7) // 8), dtype=torch.float32, device=dev)
        d_st = torch.zeros(8, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        reps = a.reps + WARMUP
        ms = np.zeros((len(KERNELS), reps), np.float64)
        vp = ctypes.c_void_p
        rc = rk.L.rt_device_noise_kernel_ms(rk.ctx, w, h, vp(d_state.data_ptr()), vp(d_half.data_ptr()), vp(d_px.data_ptr()),
                                            vp(d_tl.data_ptr()), vp(d_st.data_ptr()), reps, rt_amd.ptr(ms))
        rt_amd.check(rk.L, rc, rk.ctx, "rt_device_noise_kernel_ms")
        res["kernels"] = {"how": "rt_device_noise_kernel_ms: one launch between two events, three kernels interleaved per "
                                 "round (the tiles launches include the 32-byte memset of the stat words)",
                          "reps": a.reps, "warmup": WARMUP,
                          **{name: stats(ms[k, WARMUP:], bpp, n) for k, (name, bpp) in enumerate(KERNELS)}}
        try:
            with open(os.path.join(REPO, "profiles", "display_bench.json")) as f:
                d = json.load(f)["sizes"]["1920x1080"]
            res["kernels"]["k_display_float_recorded"] = {k: d["k_display_float"][k] for k in ("ms", "bytes_per_pixel", "gbps")}
        except (OSError, KeyError):
            pass

    d_out = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
    passes, k = 4, 16
    assert passes * k == spp

    def progression_ms(tracked: bool):
        rk.progress_begin()
        if tracked:
            rk.progress_track_noise()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for p in range(passes):
            rk.progress_advance(k, stream)
            if tracked and p >= 1:
                rt_amd.check(rk.L, rk.L.rt_progress_noise_device(rk.ctx, 0.05, ctypes.c_void_p(d_st.data_ptr()), None,
                                                                 ctypes.c_void_p(d_tl.data_ptr()), ctypes.c_void_p(stream)),
                             rk.ctx, "rt_progress_noise_device")
        rk.progress_resolve_device(d_out.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    modes = (False,) if a.untracked_only else (False, True)
    if a.untracked_only:
        d_st = d_tl = None
    progression_ms(False)  # warm-up: buffers sized, code objects loaded
    frames = {}
    ms = {m: [] for m in modes}
    for _ in range(a.prog_reps):  # (alternating, so drift lands on both alike)
        for m in modes:
            ms[m].append(round(progression_ms(m), 2))
            frames[m] = d_out.clone()
    prog = {"what": f"{passes} x {k} progression of cfg2 ({spp} spp, {nb} bounces), wall-clock ms, {a.prog_reps} repeats "
                    "alternating; tracked: rt_progress_noise_track, and a rt_progress_noise_device query (tile map, no "
                    "pixel map) after passes 2..4",
            "untracked_ms": ms[False], "untracked_min_ms": min(ms[False]),
            "untracked_spread_ms": round(max(ms[False]) - min(ms[False]), 2)}
    ok = True
    if True in ms:
        st = d_st.cpu().numpy()
        ok = bool(torch.equal(frames[True].view(torch.int32), frames[False].view(torch.int32)))
        prog.update({"tracked_ms": ms[True], "tracked_min_ms": min(ms[True]),
                     "tracked_spread_ms": round(max(ms[True]) - min(ms[True]), 2),
                     "tracked_excess_ms": round(float(np.median(ms[True]) - np.median(ms[False])), 2),
                     "tracked_excess_share_of_untracked": round(float(np.median(ms[True]) / np.median(ms[False]) - 1.0), 5),
                     "frames_equal": ok,
                     "last_query": {"tiles": int(st[0]), "tiles_over": int(st[1]), "nonfinite": int(st[2]),
                                    "max_tile": float(st[3:4].view(np.float32)[0]), "samples_a": int(st[4]),
                                    "samples_b": int(st[5]), "passes": int(st[6])}})
    rk.progress_end()
    res["progression_4x16"] = prog
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
