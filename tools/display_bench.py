"""Timing of the display stage on the GPU, at 1920x1080 and 3840x2160: k_display with the float
output, the 8-bit output (plain and flipped) and both, k_resolve_linear, and in the same session
k_resolve, the parent's tone-mapped resolve, which does k_display's arithmetic with one input buffer
more. All six kernels are timed on one footing by the library's hook rt_device_display_kernel_ms
(rt_display.hip): each launch alone on the default stream between two HIP events recorded right
before and after it, the six interleaved round by round; median of --reps after 2 warm-up rounds,
with the achieved GB/s on each kernel's byte model. An event pair around one launch still holds the
launch's fixed cost (the same for all six); the kernels' own durations come from a kernel trace of
this tool (rocprofv3 --kernel-trace, one run per size with --sizes and --no-render), which
profiles/display_bench.json holds beside these figures.

Then rt_render_linear_device beside rt_render_device on Cornell (the render minus one launch).

  python tools/display_bench.py [--reps 20] [--sizes 1920x1080,3840x2160] [--no-render]
                                [--out profiles/display_bench.json]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from stage_bench import REPO, _hip, dev_alloc, rt_amd, scenes, write_json


# the hook's kernel order, and the bytes each moves per pixel
KERNELS = (("k_resolve", 48), ("k_resolve_linear", 48), ("k_display_float", 32), ("k_display_rgba8", 20),
           ("k_display_rgba8_flip", 20), ("k_display_both", 36))
WARMUP = 2


def stats(ms, bytes_per_pixel: int, n_px: int) -> dict:
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return {"ms": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()),
            "spread_ms": float(ms.max() - ms.min()), "bytes_per_pixel": bytes_per_pixel,
            "gbps": float(bytes_per_pixel * n_px / (med * 1e-3) / 1e9)}


def kernel(w, h, spp, nb, P, sky):
    rk = rt_amd.RenderKernel(w, h, spp, nb, rt_amd.Image(1, 1), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), sky, None)
    rk.set_camera(rt_amd.Camera.preset("cornell"))
    return rk


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--no-render", action="store_true", help="skip the render comparison (kernel-trace runs)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "display_bench.json"))
    a = ap.parse_args()
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    sky = rt_amd.Image.from_rgb(scenes.make_sky("S"))
    res = {"build": rt_amd.lib().rt_build_id().decode(), "reps": a.reps, "warmup": WARMUP,
           "how": "rt_device_display_kernel_ms: one launch between two events, six kernels interleaved per round",
           "sizes": {}}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        n = w * h
        rk = kernel(w, h, 1, 1, P, sky)
        rng = np.random.default_rng(0)
        lin = rng.random((h, w, 4), dtype=np.float32) * np.float32(4.0)
        state = rng.random((h, w, 4), dtype=np.float32)
        d_lin, d_state, d_out, d_8 = dev_alloc(16 * n, lin), dev_alloc(16 * n, state), dev_alloc(16 * n), dev_alloc(4 * n)
        reps = a.reps + WARMUP
        ms = np.zeros((len(KERNELS), reps), np.float64)
        rc = rk.L.rt_device_display_kernel_ms(rk.ctx, w, h, d_lin, d_state, d_out, d_8, reps, rt_amd.ptr(ms))
        rt_amd.check(rk.L, rc, rk.ctx, "rt_device_display_kernel_ms")
        entry = {name: stats(ms[k, WARMUP:], bpp, n) for k, (name, bpp) in enumerate(KERNELS)}
        bound = entry["k_resolve"]["ms"] + entry["k_resolve"]["spread_ms"]
        entry["k_display_float_vs_k_resolve"] = {"bound_ms": bound, "holds": entry["k_display_float"]["ms"] <= bound}
        res["sizes"][size] = entry
        del rk
        for p in (d_lin, d_state, d_out, d_8):
            _hip.hipFree(p)
    if not a.no_render:
        # the render minus one launch: Cornell 1920x1080, 8 spp, 4 bounces, alternating
        w, h = 1920, 1080
        rk = kernel(w, h, 8, 4, P, sky)
        zero = np.zeros((h, w, 4), np.float32)
        d_fb = dev_alloc(16 * w * h, zero)
        rt, rl = [], []
        for rep in range(7):
            for fn, acc in ((rk.render_device, rt), (rk.render_linear_device, rl)):
                assert _hip.hipMemcpy(d_fb, zero.ctypes.data, zero.nbytes, 1) == 0
                fn(d_fb)
                assert _hip.hipDeviceSynchronize() == 0
                if rep >= 2:
                    acc.append(rk.device_last_kernel_ms())
        res["render_1920x1080_8spp_4b"] = {
            "rt_render_device_ms": float(np.median(rt)), "rt_render_device_ms_all": rt,
            "rt_render_linear_device_ms": float(np.median(rl)), "rt_render_linear_device_ms_all": rl}
        _hip.hipFree(d_fb)
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
