"""Timing of temporal accumulation on the GPU: HIP-event ms of k_temporal (rt_temporal_accumulate_device) at
1920x1080 and 3840x2160, the median of --reps calls after two warm-up calls, on the Cornell features under
two cameras a few pixels apart, beside one k_dn_direct pass (rt_denoise_device, one pass, direct loads) on
the same buffers in the same process: the yardstick for a gather kernel of this shape.

Byte model (what the call must move, re-reads served by the caches not counted): 100 B / pixel: 36 B of this
frame read (16 B colour, 4 B sigma, 16 B guide), 40 B of history read once (16 B colour, 4 B sigma, 4 B len,
16 B guide), 24 B written (16 B colour, 4 B sigma, 4 B len). The k_dn_direct pass: 64 B / pixel, as
tools/denoise_var_bench.py counts it.

  python tools/temporal_bench.py [--reps 20] [--out profiles/temporal_bench.json]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from stage_bench import REPO, _hip, cornell_kernel, dev_alloc, rt_amd, sync, write_json

SHIFT_PIXELS = 3.0  # the previous camera's offset along x, in pixels of the back wall at 1920 columns


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_bench.json"))
    a = ap.parse_args()
    res = {"build": rt_amd.lib().rt_build_id().decode(), "reps": a.reps, "bytes_per_pixel": 100,
           "bytes_per_pixel_dn_direct_pass": 64, "sizes": {}}
    for w, h in ((1920, 1080), (3840, 2160)):
        rk = cornell_kernel(w, h, 1, 1)
        cur = rt_amd.Camera.preset("cornell")
        m = cur.view_matrix.copy()
        # the back wall is 4.5 away and the frame 2 * 4.5 * aspect / fov_dist wide there
        m[0, 3] += np.float32(SHIFT_PIXELS * 2 * 4.5 * (w / h) / cur.fov_dist / 1920)
        m[1, 3] += np.float32(0.5 * SHIFT_PIXELS * 2 * 4.5 * (w / h) / cur.fov_dist / 1920)
        prev = rt_amd.Camera(m, cur.fov_dist)
        nb = w * h * 16
        t_alb, t_nd, t_hnd = dev_alloc(nb), dev_alloc(nb), dev_alloc(nb)
        rk.set_camera(prev)
        rk.features_device(t_alb, t_hnd)
        rk.set_camera(cur)
        rk.features_device(t_alb, t_nd)
        sync()
        rng = np.random.default_rng(0)
        t_in, t_hin, t_out = (dev_alloc(nb, rng.random((h, w, 4), dtype=np.float32)) for _ in range(3))
        t_sg, t_hsg, t_sout = (dev_alloc(nb // 4, (0.05 + 0.45 * rng.random((h, w), dtype=np.float32))) for _ in range(3))
        t_hlen, t_lout = (dev_alloc(nb // 4, (1 + 7 * rng.random((h, w), dtype=np.float32))) for _ in range(2))
        rk.test_schedule(dn_variant=1)
        ms_t, ms_first, ms_d = [], [], []
        for _ in range(a.reps + 2):
            rk.temporal_accumulate_device(t_in, t_sg, t_nd, prev, t_out, t_sout, t_lout, (t_hin, t_hsg, t_hlen, t_hnd))
            sync()
            ms_t.append(rk.device_last_kernel_ms())
            rk.temporal_accumulate_device(t_in, t_sg, t_nd, prev, t_out, t_sout, t_lout)
            sync()
            ms_first.append(rk.device_last_kernel_ms())
            rk.denoise_device(t_in, t_out, t_alb, t_nd, 1.0, {"passes": 1})
            sync()
            ms_d.append(rk.device_last_kernel_ms())
        rk.test_schedule(dn_variant=0)
        length = np.empty((h, w), np.float32)
        rk.temporal_accumulate_device(t_in, t_sg, t_nd, prev, t_out, t_sout, t_lout, (t_hin, t_hsg, t_hlen, t_hnd))
        sync()
        assert _hip.hipMemcpy(length.ctypes.data, t_lout, length.nbytes, 2) == 0
        t, f, d = (float(np.median(x[2:])) for x in (ms_t, ms_first, ms_d))
        res["sizes"][f"{w}x{h}"] = {
            "k_temporal_ms": t,
            "k_temporal_gbps": float(100.0 * w * h / (t * 1e-3) / 1e9),
            "k_temporal_first_frame_ms": f,
            "k_temporal_first_frame_gbps": float(60.0 * w * h / (f * 1e-3) / 1e9),
            "k_dn_direct_pass_ms": d,
            "k_dn_direct_pass_gbps": float(64.0 * w * h / (d * 1e-3) / 1e9),
            "pixels_with_history": float((length > 1).mean()),
        }
        del rk
        for p in (t_alb, t_nd, t_hnd, t_in, t_hin, t_out, t_sg, t_hsg, t_sout, t_hlen, t_lout):
            _hip.hipFree(p)
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
