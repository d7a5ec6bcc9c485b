"""Timing of the guided upscale stage on the GPU.

Kernels: HIP-event ms of k_upscale_direct and k_upscale_lds (rt_device_upscale_kernel_ms: each launch alone between
two events of its own, the two in alternating order round by round) at 960x540 -> 1920x1080 and 1920x1080 ->
3840x2160, with a sigma map, on the Cornell scene's guides at both sizes and a one-sample linear render as the low frame. In the same rounds, interleaved: one k_dn_direct
pass at the output size (rt_denoise_device with one pass under dn_variant 1, timed by rt_device_denoise_pass_ms) and
k_display's 8-bit output at the output size (rt_device_display_kernel_ms). The median, minimum and maximum of --reps
rounds after two warm-up rounds. Every call reads the same buffers again (at most 0.5 GB at 4K, inside the 256 MB
last-level cache only at 1080p), so these are not cold-HBM figures.

Byte model (what a call must move once): 52 B per low pixel (16 colour + 4 sigma + 2 x 16 guides) + 52 B per output
pixel (2 x 16 guides read, 16 + 4 written).

End to end (--end-to-end, cfg2's scene and camera, 8 bounces, --samples samples; wall clock around a synchronised
call, the median of --e2e-reps after one warm-up): (a) rt_render_linear_device at 1920x1080; (b) the same at 960x540,
then the guides at both sizes and rt_upscale_device. A measurement, not a pass criterion.

  python tools/upscale_bench.py [--reps 20] [--end-to-end] [--samples 64] [--out profiles/upscale_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import time

import numpy as np

from stage_bench import REPO, _hip, cornell_kernel, dev_alloc, rt_amd, scenes, stat, sync, write_json, yardsticks

vp = ctypes.c_void_p


def features(rk, w, h, d_alb, d_nd):
    rt_amd.check(rk.L, rk.L.rt_render_features_device(rk.ctx, w, h, vp(d_alb), vp(d_nd), None), rk.ctx,
                 "rt_render_features_device")


def kernels(a) -> dict:
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    sky = rt_amd.Image.from_rgb(scenes.make_sky("S"))
    out = {}
    for (wl, hl), (w, h) in (((960, 540), (1920, 1080)), ((1920, 1080), (3840, 2160))):
        rk = cornell_kernel(wl, hl, 1, 3)
        L, ctx = rk.L, rk.ctx
        n_lo, n = wl * hl, w * h
        rng = np.random.default_rng(0)
        d_lo, d_alo, d_nlo = dev_alloc(16 * n_lo), dev_alloc(16 * n_lo), dev_alloc(16 * n_lo)
        d_sg = dev_alloc(4 * n_lo, (0.05 + 0.45 * rng.random((hl, wl), dtype=np.float32)))
        d_ahi, d_nhi, d_out, d_tmp = (dev_alloc(16 * n) for _ in range(4))
        d_sout, d_out8 = dev_alloc(4 * n), dev_alloc(4 * n)
        rk.render_linear_device(d_lo)
        features(rk, wl, hl, d_alo, d_nlo)
        features(rk, w, h, d_ahi, d_nhi)
        sync()
        t = {k: [] for k in ("k_upscale_direct", "k_upscale_lds", "k_dn_direct", "k_display")}
        two = np.zeros(2)
        with yardsticks(rk, w, h) as yard:
            for rnd in range(a.reps + 2):
                rt_amd.check(L, L.rt_device_upscale_kernel_ms(ctx, wl, hl, w, h, vp(d_lo), vp(d_sg), vp(d_alo), vp(d_nlo), vp(d_ahi),
                                                              vp(d_nhi), vp(d_out), vp(d_sout), 1, rnd, rt_amd.ptr(two)), ctx,
                             "rt_device_upscale_kernel_ms")
                dn, disp = yard(d_out, d_tmp, d_ahi, d_nhi, d_out8)
                t["k_upscale_direct"].append(two[0])
                t["k_upscale_lds"].append(two[1])
                t["k_dn_direct"].append(dn)
                t["k_display"].append(disp)
        entry = {k: stat(v) for k, v in t.items()}
        model = 52.0 * n_lo + 52.0 * n
        for k in ("k_upscale_direct", "k_upscale_lds"):
            entry[k]["model_gbps"] = float(model / (entry[k]["ms"] * 1e-3) / 1e9)
        yard = entry["k_dn_direct"]
        entry["bound_ms"] = yard["ms"] + (yard["max"] - yard["min"])
        out[f"{wl}x{hl}->{w}x{h}"] = entry
        del rk
        for q in (d_lo, d_alo, d_nlo, d_sg, d_ahi, d_nhi, d_out, d_tmp, d_sout, d_out8):
            _hip.hipFree(q)
    return out


def end_to_end(a) -> dict:
    import bench
    P, sky, cam17 = bench.build_inputs("cfg2")
    _, _, _, W, H, spp, nb, desc = bench.CONFIGS["cfg2"]
    spp = a.samples or spp
    sky_img = rt_amd.Image.from_rgb(sky)
    cdf = rt_amd.compute_env_map_cdf(sky_img)
    wl, hl = W // 2, H // 2
    res = {"workload": f"{desc}, at {spp} samples", "full": [W, H], "low": [wl, hl]}

    def kernel(w, h):
        rk = rt_amd.RenderKernel(w, h, spp, nb, rt_amd.Image(1, 1), P.triangles, P.materials, P.emissive_triangle_indices,
                                 P.material_indices, None, rt_amd.BVH(P.triangles), sky_img, cdf)
        rk.set_camera(rt_amd.Camera(cam17[:16], cam17[16]))
        return rk

    def wall(fn):
        ms = []
        for _ in range(a.e2e_reps + 1):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = np.asarray(ms[1:])
        return {"ms": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max())}

    n_lo, n = wl * hl, W * H
    d_full = dev_alloc(16 * n)
    rk = kernel(W, H)
    res["a_render_full"] = wall(lambda: rk.render_linear_device(d_full))
    del rk
    rk = kernel(wl, hl)
    d_lo, d_alo, d_nlo = (dev_alloc(16 * n_lo) for _ in range(3))
    d_ahi, d_nhi = dev_alloc(16 * n), dev_alloc(16 * n)

    def low_path():
        rk.render_linear_device(d_lo)
        features(rk, wl, hl, d_alo, d_nlo)
        features(rk, W, H, d_ahi, d_nhi)
        rk.upscale_device((wl, hl), (W, H), d_lo, d_alo, d_nlo, d_ahi, d_nhi, d_full)

    res["b_render_low_features_upscale"] = wall(low_path)
    res["b_render_low_alone"] = wall(lambda: rk.render_linear_device(d_lo))
    res["ratio_b_over_a"] = res["b_render_low_features_upscale"]["ms"] / res["a_render_full"]["ms"]
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--samples", type=int, default=0, help="end to end: samples per pixel (0: cfg2's 64)")
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "upscale_bench.json"))
    a = ap.parse_args()
    res = {"build": rt_amd.lib().rt_build_id().decode(), "reps": a.reps,
           "how": "rt_device_upscale_kernel_ms, rt_device_denoise_pass_ms (one pass, dn_variant 1) and rt_device_display_kernel_ms "
                  "(8-bit out), one launch of each per round, median / min / max of the rounds after two warm-ups; bound_ms = "
                  "k_dn_direct's median + its spread (max - min)",
           "kernels": kernels(a)}
    if a.end_to_end:
        res["end_to_end"] = end_to_end(a)
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
