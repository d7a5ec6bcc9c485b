"""Timing of the motion stages on the GPU: HIP-event ms of k_mblur_lds, k_mblur_direct, k_motion_tilemax and
k_motion_vectors alone on the default stream (rt_device_motion_kernel_ms, the two gather kernels alternating order round
by round) and of the whole blur call (rt_motion_blur_device, rt_device_last_kernel_ms: the tile maximum plus the
product's dispatch), at 1920x1080 and 3840x2160 and max_radius 4, 8 and 16, on four frames: a still one (no motion: every
tile a copy), a uniform horizontal streak and a uniform diagonal streak of max_radius pixels either way (the full line in
every tile) and the real vectors of a yaw of 2 degrees over Cornell's first hits (rt_motion_vectors at shutter 1). In
the same process and on the same frame one a-trous pass at that size (rt_denoise_device with one pass under dn_variant 1,
rt_device_denoise_pass_ms, guided by Cornell's first hits) and k_display's 8-bit output (rt_device_display_kernel_ms).
The median, minimum and maximum of --reps rounds after two warm-up rounds. Every call reads the same buffers again
(inside the 256 MB last-level cache only at 1080p), so these are not cold-HBM figures.

The blur must move 44 B per pixel once (16 B colour, 16 B guide record of which 4 B are used, 8 B motion read, 16 B
written less the 12 B that overlap nothing; 4 B more with reach_out); taps are re-reads the LDS tile or the caches serve.

  python tools/motion_bench.py [--reps 20] [--out profiles/motion_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

import numpy as np

from stage_bench import REPO, _hip, cornell_kernel, dev_alloc, rt_amd, stat, sync, test_frame, write_json, yardsticks

vp = ctypes.c_void_p


def yawed(cam, deg):
    """cam turned by deg about its own y axis."""
    a = np.radians(deg)
    rot = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    return rt_amd.Camera((cam.view_matrix.astype(np.float64).reshape(4, 4) @ rot).astype(np.float32), cam.fov_dist)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "motion_bench.json"))
    a = ap.parse_args()
    res = {"reps": a.reps, "sizes": {},
           "how": "rt_device_motion_kernel_ms (one launch of each kernel per round), rt_motion_blur_device + rt_device_last_kernel_ms, "
                  "rt_device_denoise_pass_ms (one pass, dn_variant 1) and rt_device_display_kernel_ms (8-bit out); median / min / "
                  "max of the rounds after two warm-ups; buffers re-read every round (in cache at 1080p)"}
    for w, h in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        rk = cornell_kernel(w, h, 1, 3)
        cam = rt_amd.Camera.preset("cornell")
        rk.set_camera(cam)
        prev = yawed(cam, 2.0)
        L, ctx = rk.L, rk.ctx
        res["build"] = L.rt_build_id().decode()
        n = w * h
        frame = test_frame(w, h)
        d_in, d_out, d_tmp, d_alb, d_gnd = dev_alloc(16 * n, frame), *(dev_alloc(16 * n) for _ in range(4))
        d_m, d_vec, d_reach, d_out8 = dev_alloc(8 * n), dev_alloc(8 * n), dev_alloc(4 * n), dev_alloc(4 * n)
        rt_amd.check(L, L.rt_render_features_device(ctx, w, h, vp(d_alb), vp(d_gnd), None), ctx, "rt_render_features_device")
        rk.motion_vectors_device(d_gnd, prev, d_vec, width=w, height=h)
        sync()
        real = np.empty((h, w, 2), np.float32)
        assert _hip.hipMemcpy(real.ctypes.data, vp(d_vec), real.nbytes, 2) == 0
        entry = {"yaw_vectors_px": {"median": float(np.median(np.hypot(real[..., 0], real[..., 1]))),
                                    "max": float(np.hypot(real[..., 0], real[..., 1]).max())}}
        # the yardsticks on the same frame
        t = {"k_dn_direct": [], "k_display": []}
        with yardsticks(rk, w, h) as yard:
            for _ in range(a.reps + 2):
                dn, disp = yard(d_in, d_tmp, d_alb, d_gnd, d_out8)
                t["k_dn_direct"].append(dn)
                t["k_display"].append(disp)
        entry.update({k: stat(v) for k, v in t.items()})
        m = np.zeros((h, w, 2), np.float32)
        for R in (4, 8, 16):
            per_r = {}
            for name, vec in (("still", (0.0, 0.0)), ("horizontal", (2.0 * R, 0.0)), ("diagonal", (1.4142 * R, 1.4142 * R)), ("yaw", None)):
                m[...] = real if vec is None else vec
                assert _hip.hipMemcpy(vp(d_m), m.ctypes.data, m.nbytes, 1) == 0
                p = rt_amd.MotionParams(1.0, 0.05, R)
                t = {"k_mblur_direct": [], "k_mblur_lds": [], "k_motion_tilemax": [], "k_motion_vectors": [], "call": []}
                four = np.zeros(4)
                for rnd in range(a.reps + 2):
                    rt_amd.check(L, L.rt_device_motion_kernel_ms(ctx, w, h, vp(d_in), vp(d_gnd), vp(d_m), ctypes.byref(p), vp(d_out),
                                                                 vp(d_reach), rt_amd.ptr(prev.view_matrix), prev.fov_dist, vp(d_vec), 1, rnd,
                                                                 rt_amd.ptr(four)), ctx, "rt_device_motion_kernel_ms")
                    for k, key in enumerate(("k_mblur_direct", "k_mblur_lds", "k_motion_tilemax", "k_motion_vectors")):
                        t[key].append(four[k])
                    rt_amd.check(L, L.rt_motion_blur_device(ctx, w, h, vp(d_in), vp(d_gnd), vp(d_m), ctypes.byref(p), vp(d_out), vp(d_reach),
                                                            None), ctx, "rt_motion_blur_device")
                    sync()
                    t["call"].append(float(L.rt_device_last_kernel_ms(ctx)))
                e = {k: stat(v) for k, v in t.items()}
                e["lds_over_direct"] = e["k_mblur_lds"]["ms"] / e["k_mblur_direct"]["ms"]
                e["call_over_k_display"] = e["call"]["ms"] / entry["k_display"]["ms"]
                e["call_over_atrous_pass"] = e["call"]["ms"] / entry["k_dn_direct"]["ms"]
                per_r[name] = e
            entry[f"max_radius_{R}"] = per_r
        res["sizes"][f"{w}x{h}"] = entry
        for q in (d_in, d_out, d_tmp, d_alb, d_gnd, d_m, d_vec, d_reach, d_out8):
            _hip.hipFree(vp(q))
        del rk
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
