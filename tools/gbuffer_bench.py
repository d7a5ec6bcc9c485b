"""Timing of the first-hit G-buffer stage (rt_render_gbuffer_device) on the GPU against the passes it can
replace, at 1920x1080 on Cornell and on cfg2's scene (the dragon stand-in) under their preset cameras.

Per round, interleaved, each call between the stage's two events (rt_device_last_kernel_ms after a
synchronise): rt_render_gbuffer_device under gb_variant 1 (plain rounds), 2 (refill) and 0 (the product's
choice), the same with RT_GBUFFER_EXACT (the octet walk for every pixel), rt_render_features_device, and
rt_query_device(CLOSEST) on the camera rays. --reps rounds after two warm-ups, reported as median (min .. max),
with rt_gbuffer_last_exact alongside. Criterion (cfg2 only): the median of the product's variant, and of the
EXACT form, lies below the minimum of rt_render_features_device over the same rounds.

End to end (--end-to-end, cfg2, 8 bounces, --samples samples; wall clock around a synchronised call, median of
--e2e-reps after one warm-up): chain (b) of tools/upscale_bench.py, the render at 960x540, the guides at both
sizes and rt_upscale_device, with the guides from rt_render_features_device and from rt_render_gbuffer_device.

  python tools/gbuffer_bench.py [--reps 20] [--end-to-end] [--samples 64] [--out profiles/gbuffer_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

from stage_bench import REPO, _hip, dev_alloc, rt_amd, scenes, stat, sync, write_json

vp = ctypes.c_void_p
W, H = 1920, 1080


def features(rk, w, h, d_alb, d_nd):
    rt_amd.check(rk.L, rk.L.rt_render_features_device(rk.ctx, w, h, vp(d_alb), vp(d_nd), None), rk.ctx,
                 "rt_render_features_device")


def stage_times(scene: str, a) -> dict:
    P = rt_amd.parse_obj(scenes.scene_path(scene))
    rk = rt_amd.RenderKernel(W, H, 1, 1, rt_amd.Image(1, 1), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), rt_amd.Image.from_rgb(scenes.make_sky("L")),
                             None)
    rk.set_camera(rt_amd.Camera.preset(scene))
    n = W * H
    rays = np.ascontiguousarray(rk.camera_rays().reshape(-1, 6))
    d_rays, d_rec = dev_alloc(rays.nbytes, rays), dev_alloc(n * 44)
    d_alb, d_nd, d_ids, d_falb, d_fnd = dev_alloc(16 * n), dev_alloc(16 * n), dev_alloc(8 * n), dev_alloc(16 * n), dev_alloc(16 * n)
    calls = {
        "gbuffer_plain": (1, lambda: rk.gbuffer_device(d_alb, d_nd, d_ids)),
        "gbuffer_refill": (2, lambda: rk.gbuffer_device(d_alb, d_nd, d_ids)),
        "gbuffer_product": (0, lambda: rk.gbuffer_device(d_alb, d_nd, d_ids)),
        "gbuffer_exact": (0, lambda: rk.gbuffer_device(d_alb, d_nd, d_ids, exact=True)),
        "features": (0, lambda: features(rk, W, H, d_falb, d_fnd)),
        "query_closest": (0, lambda: rk.query_device(d_rays, n, d_rec, mode="closest")),
    }
    t = {k: [] for k in calls}
    last_exact = {}
    for _ in range(a.reps + 2):
        for name, (variant, fn) in calls.items():
            rk.test_schedule(gb_variant=variant)
            fn()
            sync()
            t[name].append(rk.device_last_kernel_ms())
            if name.startswith("gbuffer"):
                last_exact[name] = rk.gbuffer_last_exact()
            elif name == "query_closest":
                last_exact[name] = rk.query_last_exact()
    rk.test_schedule(gb_variant=0)
    entry = {k: stat(v) for k, v in t.items()}
    for k, v in last_exact.items():
        entry[k]["last_exact"] = int(v)
    got = [np.empty((n, 4), np.float32) for _ in range(4)]
    for g, d in zip(got, (d_alb, d_nd, d_falb, d_fnd)):
        assert _hip.hipMemcpy(g.ctypes.data, d, g.nbytes, 2) == 0
    entry["exact_form_equals_features_bitwise"] = bool(np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32)) and
                                                       np.array_equal(got[1].view(np.uint32), got[3].view(np.uint32)))
    rk.gbuffer_device(d_alb, d_nd, d_ids)
    sync()
    for g, d in zip(got[:2], (d_alb, d_nd)):
        assert _hip.hipMemcpy(g.ctypes.data, d, g.nbytes, 2) == 0
    entry["pixels_differing_from_features"] = int((got[1].view(np.uint32) != got[3].view(np.uint32)).any(axis=1).sum())
    entry["pixels"] = n
    entry["camera_inside_near_box"] = bool(entry["gbuffer_product"]["last_exact"] < n)
    fmin = entry["features"]["min"]
    entry["product_median_below_features_min"] = bool(entry["gbuffer_product"]["ms"] < fmin)
    entry["exact_median_below_features_min"] = bool(entry["gbuffer_exact"]["ms"] < fmin)
    for q in (d_rays, d_rec, d_alb, d_nd, d_ids, d_falb, d_fnd):
        _hip.hipFree(q)
    return entry


def end_to_end(a) -> dict:
    import bench
    P, sky, cam17 = bench.build_inputs("cfg2")
    _, _, _, w, h, spp, nb, desc = bench.CONFIGS["cfg2"]
    spp = a.samples or spp
    sky_img = rt_amd.Image.from_rgb(sky)
    wl, hl = w // 2, h // 2
    rk = rt_amd.RenderKernel(wl, hl, spp, nb, rt_amd.Image(1, 1), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), sky_img, rt_amd.compute_env_map_cdf(sky_img))
    rk.set_camera(rt_amd.Camera(cam17[:16], cam17[16]))
    n_lo, n = wl * hl, w * h
    d_full, d_ahi, d_nhi = (dev_alloc(16 * n) for _ in range(3))
    d_lo, d_alo, d_nlo = (dev_alloc(16 * n_lo) for _ in range(3))

    def wall(fn):
        ms = []
        for _ in range(a.e2e_reps + 1):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stat(ms, 1)

    def chain(walks: bool):
        rk.render_linear_device(d_lo)
        if walks:
            rk.gbuffer_device(d_alo, d_nlo, size=(wl, hl))
            rk.gbuffer_device(d_ahi, d_nhi, size=(w, h))
        else:
            features(rk, wl, hl, d_alo, d_nlo)
            features(rk, w, h, d_ahi, d_nhi)
        rk.upscale_device((wl, hl), (w, h), d_lo, d_alo, d_nlo, d_ahi, d_nhi, d_full)

    res = {"workload": f"{desc}, at {spp} samples", "full": [w, h], "low": [wl, hl],
           "b_guides_from_features": wall(lambda: chain(False)), "b_guides_from_gbuffer": wall(lambda: chain(True)),
           "b_render_low_alone": wall(lambda: rk.render_linear_device(d_lo))}
    res["ratio_gbuffer_over_features"] = res["b_guides_from_gbuffer"]["ms"] / res["b_guides_from_features"]["ms"]
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--samples", type=int, default=0, help="end to end: samples per pixel (0: cfg2's 64)")
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gbuffer_bench.json"))
    a = ap.parse_args()
    res = {"build": rt_amd.lib().rt_build_id().decode(), "reps": a.reps, "size": [W, H],
           "how": "one call of each per round, interleaved, between the stage's two events (rt_device_last_kernel_ms after a "
                  "synchronise); median / min / max of the rounds after two warm-ups; last_exact = rt_gbuffer_last_exact / "
                  "rt_query_last_exact of the last round",
           "scenes": {}}
    for scene in ("cornell", "dragon"):
        res["scenes"][scene] = stage_times(scene, a)
        print(scene, json.dumps(res["scenes"][scene]), flush=True)
    if a.end_to_end:
        res["end_to_end"] = end_to_end(a)
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
