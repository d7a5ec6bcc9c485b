"""Timing of the batched ray queries (rt_query_device) on the MI355X against k_intersect
(rt_intersect's kernel) on the same rays in the same session: HIP-event ms, median of --reps
launches after warm-up, for RT_QUERY_EXACT and each rq_variant (0 the product's choice,
1 plain rounds, 2 per-quad refill), closest and any modes, on three ray sets over the cfg2
scene (the dragon stand-in): the 1920x1080 camera rays of rt_camera_rays, cosine-distributed
bounce rays from those rays' hit points, and the same bounce rays shuffled.

  python tools/rt_query_bench.py [--reps 20] [--out profiles/query_api_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from stage_bench import REPO, _hip, dev_alloc, rt_amd, scenes, sync


def bounce_rays(cam_rays: np.ndarray, hits: np.ndarray, seed: int = 3) -> np.ndarray:
    """One cosine-distributed ray from every camera ray's hit point, about the normal on the
    side the camera ray came from, its origin 1e-4 along that normal (misses dropped)."""
    rng = np.random.default_rng(seed)
    hit = hits[:, 0] == 1
    p = hits[hit, 3:6].view(np.float32).astype(np.float64)
    n = hits[hit, 6:9].view(np.float32).astype(np.float64)
    d_in = cam_rays[hit, 3:6].astype(np.float64)
    n = np.where((n * d_in).sum(1, keepdims=True) > 0, -n, n)
    a = np.where(np.abs(n[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = np.cross(a, n)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    u1, u2 = rng.random(p.shape[0]), rng.random(p.shape[0])
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    d = (r * np.cos(phi))[:, None] * t + (r * np.sin(phi))[:, None] * b + np.sqrt(1 - u1)[:, None] * n
    return np.ascontiguousarray(np.concatenate([p + 1e-4 * n, d], 1), dtype=np.float32)


def stats(ms: list, n: int) -> dict:
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return {"ms": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()), "mrays_per_s": n / med / 1e3}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "query_api_bench.json"))
    a = ap.parse_args()
    W, H = 1920, 1080
    P = rt_amd.parse_obj(scenes.scene_path("dragon"))
    rk = rt_amd.RenderKernel(W, H, 1, 1, rt_amd.Image(1, 1), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles),
                             rt_amd.Image.from_rgb(scenes.make_sky("L")), None)
    rk.set_camera(rt_amd.Camera.preset("dragon"))
    cam = np.ascontiguousarray(rk.camera_rays().reshape(-1, 6))
    bounce = bounce_rays(cam, rk.intersect(cam))
    shuffled = np.ascontiguousarray(bounce[np.random.default_rng(4).permutation(bounce.shape[0])])
    res = {"build": rt_amd.lib().rt_build_id().decode(), "reps": a.reps, "warmup": a.warmup, "scene": "dragon (cfg2)",
           "what": "HIP-event ms per call, median (min, max) of reps; ratio = k_intersect ms / this ms on the same rays",
           "sets": {}}
    for name, rays in (("camera_1080p", cam), ("bounce_cosine", bounce), ("bounce_cosine_shuffled", shuffled)):
        n = rays.shape[0]
        base, want = [], None
        for _ in range(a.warmup + a.reps):
            want = rk.intersect(rays)
            base.append(rk.last_kernel_ms())
        entry = {"n": n, "found": int(want[:, 0].sum()), "k_intersect": stats(base[a.warmup:], n)}
        d_rays, d_out = dev_alloc(rays.nbytes, rays), dev_alloc(n * 44)
        for mode in ("closest", "any"):
            w = want if mode == "closest" else want[:, 0]
            for label, variant, exact in (("exact", 0, True), ("plain", 1, False), ("refill", 2, False),
                                          ("product", 0, False)):
                rk.test_schedule(rq_variant=variant)
                ms = []
                for _ in range(a.warmup + a.reps):
                    rk.query_device(d_rays, n, d_out, mode=mode, exact=exact)
                    sync()
                    ms.append(rk.device_last_kernel_ms())
                got = np.empty(w.shape, np.int32)
                assert _hip.hipMemcpy(got.ctypes.data, d_out, got.nbytes, 2) == 0
                e = stats(ms[a.warmup:], n)
                e["exact_walk_share"] = rk.query_last_exact() / n
                e["ratio_to_k_intersect"] = entry["k_intersect"]["ms"] / e["ms"]
                e["bitwise_equal_to_rt_intersect"] = bool(np.array_equal(got, w))
                entry[f"{mode}_{label}"] = e
                print(name, mode, label, json.dumps(e), flush=True)
        rk.test_schedule(rq_variant=0)
        res["sets"][name] = entry
        for p in (d_rays, d_out):
            _hip.hipFree(p)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
