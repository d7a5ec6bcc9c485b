"""Timing of the depth-of-field stage on the GPU: HIP-event ms of k_dof_lds and of k_dof_direct alone on the default
stream (rt_device_dof_kernel_ms, the two alternating order round by round) and of the whole call (rt_dof_device,
rt_device_last_kernel_ms, the product's dispatch), at 1920x1080 and 3840x2160 and max_radius 4, 8 and 12, on two frames:
one in focus everywhere (t = focus: r = 0, one tap per pixel for the LDS kernel, whose window follows the largest radius
of the block's footprint; the direct kernel visits the rule's whole window whatever the radii) and one defocused
everywhere (t = focus / 2 with coc_inf = max_radius: r = max_radius, the full disc). In the same process and on the same
frame one a-trous pass at that size (rt_denoise_device with one pass under dn_variant 1, rt_device_denoise_pass_ms,
guided by Cornell's first hits) and k_display's 8-bit output (rt_device_display_kernel_ms). The median, minimum and
maximum of --reps rounds after two warm-up rounds. Every call reads the same buffers again (at most 0.4 GB at 4K, inside
the 256 MB last-level cache only at 1080p), so these are not cold-HBM figures.

The stage must move 36 B per pixel once (16 B colour + 16 B guide record read, of which 4 B are used, 16 B written; 4 B
more with coc_out); taps are re-reads the LDS tile or the caches serve.

  python tools/dof_bench.py [--reps 20] [--out profiles/dof_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

import numpy as np

from stage_bench import REPO, _hip, cornell_kernel, dev_alloc, rt_amd, stat, sync, test_frame, write_json, yardsticks

vp = ctypes.c_void_p
FOCUS = 2.0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dof_bench.json"))
    a = ap.parse_args()
    res = {"reps": a.reps, "sizes": {},
           "how": "rt_device_dof_kernel_ms (one launch of each kernel per round), rt_dof_device + rt_device_last_kernel_ms, "
                  "rt_device_denoise_pass_ms (one pass, dn_variant 1) and rt_device_display_kernel_ms (8-bit out); median / min / "
                  "max of the rounds after two warm-ups; buffers re-read every round (in cache at 1080p)"}
    for w, h in ((1920, 1080), (3840, 2160)):
        rk = cornell_kernel(w, h, 1, 3)
        L, ctx = rk.L, rk.ctx
        res["build"] = L.rt_build_id().decode()
        n = w * h
        frame = test_frame(w, h)
        nd = np.zeros((h, w, 4), np.float32)
        d_in, d_nd, d_out, d_tmp, d_alb, d_gnd = dev_alloc(16 * n, frame), dev_alloc(16 * n), *(dev_alloc(16 * n) for _ in range(4))
        d_coc, d_out8 = dev_alloc(4 * n), dev_alloc(4 * n)
        rt_amd.check(L, L.rt_render_features_device(ctx, w, h, vp(d_alb), vp(d_gnd), None), ctx, "rt_render_features_device")
        sync()
        entry = {}
        # the yardsticks on the same frame
        t = {"k_dn_direct": [], "k_display": []}
        with yardsticks(rk, w, h) as yard:
            for _ in range(a.reps + 2):
                dn, disp = yard(d_in, d_tmp, d_alb, d_gnd, d_out8)
                t["k_dn_direct"].append(dn)
                t["k_display"].append(disp)
        entry.update({k: stat(v) for k, v in t.items()})
        for R in (4, 8, 12):
            per_r = {}
            for name, t_frame in (("in_focus", FOCUS), ("defocused", FOCUS / 2)):
                nd[..., 3] = t_frame
                assert _hip.hipMemcpy(vp(d_nd), nd.ctypes.data, nd.nbytes, 1) == 0
                p = rt_amd.DofParams(FOCUS, float(R), R)
                t = {"k_dof_direct": [], "k_dof_lds": [], "call": []}
                two = np.zeros(2)
                for rnd in range(a.reps + 2):
                    rt_amd.check(L, L.rt_device_dof_kernel_ms(ctx, w, h, vp(d_in), vp(d_nd), ctypes.byref(p), vp(d_out), vp(d_coc), 1,
                                                              rnd, rt_amd.ptr(two)), ctx, "rt_device_dof_kernel_ms")
                    t["k_dof_direct"].append(two[0])
                    t["k_dof_lds"].append(two[1])
                    rt_amd.check(L, L.rt_dof_device(ctx, w, h, vp(d_in), vp(d_nd), ctypes.byref(p), vp(d_out), vp(d_coc), None), ctx,
                                 "rt_dof_device")
                    sync()
                    t["call"].append(float(L.rt_device_last_kernel_ms(ctx)))
                e = {k: stat(v) for k, v in t.items()}
                e["lds_over_direct"] = e["k_dof_lds"]["ms"] / e["k_dof_direct"]["ms"]
                e["call_over_k_display"] = e["call"]["ms"] / entry["k_display"]["ms"]
                e["call_over_atrous_pass"] = e["call"]["ms"] / entry["k_dn_direct"]["ms"]
                per_r[name] = e
            entry[f"max_radius_{R}"] = per_r
        res["sizes"][f"{w}x{h}"] = entry
        for q in (d_in, d_nd, d_out, d_tmp, d_alb, d_gnd, d_coc, d_out8):
            _hip.hipFree(vp(q))
        del rk
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
