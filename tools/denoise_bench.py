"""Timing of the post stage on the GPU: HIP-event ms of the feature pass (Cornell, the
render's exact closest-hit walk) and of each à-trous pass at 1920x1080 and 3840x2160, for
the direct-load kernel and for the LDS-halo kernel (steps 1, 2, 4), with the achieved GB/s
on the 64 B / pixel / pass model (16 B colour + 32 B guides read, 16 B written).

  python tools/denoise_bench.py [--reps 20] [--out profiles/denoise_bench.json]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_bench.json"))
    a = ap.parse_args()
    res = {"build": rt_amd.lib().rt_build_id().decode(), "reps": a.reps, "bytes_per_pixel_pass": 64, "sizes": {}}
    for w, h in ((1920, 1080), (3840, 2160)):
        rk = cornell_kernel(w, h, 1, 1)
        L, ctx = rk.L, rk.ctx
        nb = w * h * 16
        t_alb, t_nd = dev_alloc(nb), dev_alloc(nb)
        feat = []
        for _ in range(a.reps + 2):
            rk.features_device(t_alb, t_nd)
            sync()
            feat.append(rk.device_last_kernel_ms())
        feat = feat[2:]
        rng = np.random.default_rng(0)
        t_in, t_out = dev_alloc(nb, rng.random((h, w, 4), dtype=np.float32)), dev_alloc(nb)
        entry = {"features_ms": float(np.median(feat)), "features_ms_min": float(np.min(feat)), "variants": {}}
        L.rt_device_denoise_pass_ms(ctx, 1, None, 0)
        for name, v in (("direct", 1), ("lds", 2)):
            rk.test_schedule(dn_variant=v)
            per, total = [], []
            for _ in range(a.reps + 2):
                rk.denoise_device(t_in, t_out, t_alb, t_nd, 1.0,
                                  {"passes": PASSES})
                sync()
                ms = np.zeros(PASSES)
                n = L.rt_device_denoise_pass_ms(ctx, -1, rt_amd.ptr(ms), PASSES)
                assert n == PASSES, n
                per.append(ms)
                total.append(rk.device_last_kernel_ms())
            per = np.median(np.asarray(per[2:]), axis=0)
            entry["variants"][name] = {
                "pass_ms": [float(x) for x in per],
                "pass_gbps": [float(64.0 * w * h / (x * 1e-3) / 1e9) for x in per],
                "kernel_of_pass": [("lds" if v == 2 and (1 << i) <= 4 else "direct") for i in range(PASSES)],
                "total_ms": float(np.median(total[2:])),
            }
        rk.test_schedule(dn_variant=0)
        tot = []
        for _ in range(a.reps + 2):
            rk.denoise_device(t_in, t_out, t_alb, t_nd, 1.0,
                              {"passes": PASSES})
            sync()
            tot.append(rk.device_last_kernel_ms())
        entry["product_filter_ms"] = float(np.median(tot[2:]))
        entry["post_stage_ms"] = entry["features_ms"] + entry["product_filter_ms"]
        res["sizes"][f"{w}x{h}"] = entry
        del rk
        for p in (t_alb, t_nd, t_in, t_out):
            _hip.hipFree(p)
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
