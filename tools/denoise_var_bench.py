"""Timing of the variance-guided filter on the GPU: HIP-event ms of k_dnv_prep and of each à-trous
pass of rt_denoise_var_device at 1920x1080 and 3840x2160, for the direct-load kernel and for the
LDS-halo kernel (steps 1, 2, 4), the median of --reps calls after two warm-up calls, beside
rt_denoise_device's five passes on the same buffers in the same process.

Byte model (what a pass must move, re-reads served by the caches not counted): 64 B / pixel / pass
(16 B record + 32 B guides read, 16 B written; the last pass's 16 B of the caller's input and 4 B of
sigma_out are left out so that the passes compare), 36 B / pixel for the prep (16 B colour + 4 B
sigma read, 16 B record written).

  python tools/denoise_var_bench.py [--reps 20] [--out profiles/denoise_var_bench.json]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from stage_bench import REPO, _hip, cornell_kernel, dev_alloc, rt_amd, sync, write_json

PASSES = 5


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_var_bench.json"))
    a = ap.parse_args()
    res = {"build": rt_amd.lib().rt_build_id().decode(), "reps": a.reps, "passes": PASSES, "bytes_per_pixel_pass": 64,
           "bytes_per_pixel_prep": 36, "sizes": {}}
    for w, h in ((1920, 1080), (3840, 2160)):
        rk = cornell_kernel(w, h, 1, 1)
        L, ctx = rk.L, rk.ctx
        nb = w * h * 16
        t_alb, t_nd = dev_alloc(nb), dev_alloc(nb)
        rk.features_device(t_alb, t_nd)
        sync()
        rng = np.random.default_rng(0)
        t_in, t_out = dev_alloc(nb, rng.random((h, w, 4), dtype=np.float32)), dev_alloc(nb)
        t_sg = dev_alloc(nb // 4, (0.05 + 0.45 * rng.random((h, w), dtype=np.float32)))
        t_left = dev_alloc(nb // 4)
        entry = {"variants": {}}
        assert L.rt_device_denoise_var_pass_ms(ctx, 1, None, 0) == 0
        for name, v in (("direct", 1), ("lds", 2)):
            rk.test_schedule(dn_variant=v)
            per, total = [], []
            for _ in range(a.reps + 2):
                rk.denoise_var_device(t_in, t_sg, t_out, t_alb, t_nd, 1.0, {"passes": PASSES}, d_sigma_out=t_left)
                sync()
                ms = np.zeros(PASSES + 1)
                n = L.rt_device_denoise_var_pass_ms(ctx, -1, rt_amd.ptr(ms), PASSES + 1)
                assert n == PASSES + 1, n
                per.append(ms)
                total.append(rk.device_last_kernel_ms())
            per = np.median(np.asarray(per[2:]), axis=0)
            entry["variants"][name] = {
                "prep_ms": float(per[0]),
                "prep_gbps": float(36.0 * w * h / (per[0] * 1e-3) / 1e9),
                "pass_ms": [float(x) for x in per[1:]],
                "pass_gbps": [float(64.0 * w * h / (x * 1e-3) / 1e9) for x in per[1:]],
                "kernel_of_pass": [("lds" if v == 2 and (1 << i) <= 4 else "direct") for i in range(PASSES)],
                "total_ms": float(np.median(total[2:])),
            }
        assert L.rt_device_denoise_var_pass_ms(ctx, 0, None, 0) == 0
        rk.test_schedule(dn_variant=0)
        tot, fixed = [], []
        for _ in range(a.reps + 2):
            rk.denoise_var_device(t_in, t_sg, t_out, t_alb, t_nd, 1.0, {"passes": PASSES}, d_sigma_out=t_left)
            sync()
            tot.append(rk.device_last_kernel_ms())
            rk.denoise_device(t_in, t_out, t_alb, t_nd, 1.0, {"passes": PASSES})
            sync()
            fixed.append(rk.device_last_kernel_ms())
        entry["product_filter_ms"] = float(np.median(tot[2:]))
        entry["rt_denoise_filter_ms"] = float(np.median(fixed[2:]))
        res["sizes"][f"{w}x{h}"] = entry
        del rk
        for p in (t_alb, t_nd, t_in, t_out, t_sg, t_left):
            _hip.hipFree(p)
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
