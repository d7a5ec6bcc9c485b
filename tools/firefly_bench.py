"""Timing of the firefly rejection stage on the GPU: HIP-event ms of k_firefly_lds and k_firefly_direct
(rt_firefly_device under ff_variant 2 and 1) at 1920x1080 and 3840x2160, radius 1 and 2, rank 2 (the default) and 8
(what an insertion into a fixed eight registers would cost at any rank), the median of --reps calls after two warm-up
calls; in the same process one k_temporal call (rt_temporal_accumulate_device with a history) and one k_dnv_prep
call (the first launch of rt_denoise_var_device) on buffers of the same size, as yardsticks.

Byte model (what a call must move, re-reads served by the caches not counted): 44 B / pixel for the stage (16 B
colour + 4 B sigma read, 16 B colour + 4 B sigma + 4 B scale written), 100 B / pixel for k_temporal and 36 B /
pixel for k_dnv_prep, as tools/temporal_bench.py and tools/denoise_var_bench.py count them. The GB/s figures are
the model over the time on buffers that every call reads again, not HBM traffic.

The input is a noisy gradient with a bright pixel in every 97th place, the default gain and floor.

  python tools/firefly_bench.py [--reps 20] [--out profiles/firefly_bench.json]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from stage_bench import REPO, _hip, cornell_kernel, dev_alloc, rt_amd, sync, test_frame, write_json

BPP, BPP_TEMPORAL, BPP_PREP = 44.0, 100.0, 36.0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "firefly_bench.json"))
    a = ap.parse_args()
    res = {"build": rt_amd.lib().rt_build_id().decode(), "reps": a.reps, "bytes_per_pixel": BPP,
           "bytes_per_pixel_k_temporal": BPP_TEMPORAL, "bytes_per_pixel_k_dnv_prep": BPP_PREP, "sizes": {}}
    for w, h in ((1920, 1080), (3840, 2160)):
        rk = cornell_kernel(w, h, 1, 1)
        cam = rt_amd.Camera.preset("cornell")
        rk.set_camera(cam)
        L, ctx = rk.L, rk.ctx
        nb = w * h * 16
        t_alb, t_nd = dev_alloc(nb), dev_alloc(nb)
        rk.features_device(t_alb, t_nd)
        sync()
        rng = np.random.default_rng(0)
        frame = test_frame(w, h, rng)
        t_in, t_hin, t_out = dev_alloc(nb, frame), dev_alloc(nb, rng.random((h, w, 4), dtype=np.float32)), dev_alloc(nb)
        t_sg, t_hsg, t_sout = (dev_alloc(nb // 4, (0.05 + 0.45 * rng.random((h, w), dtype=np.float32))) for _ in range(3))
        t_hlen, t_fout = (dev_alloc(nb // 4, (1 + 7 * rng.random((h, w), dtype=np.float32))) for _ in range(2))
        entry = {"kernels": {}}
        for radius in (1, 2):
            for rank in (2, 8):
                for name, v in (("lds", 2), ("direct", 1)):
                    rk.test_schedule(ff_variant=v)
                    ms = []
                    for _ in range(a.reps + 2):
                        rk.firefly_clamp_device(t_in, t_out, t_sg, t_sout, t_fout, {"radius": radius, "rank": rank})
                        sync()
                        ms.append(rk.device_last_kernel_ms())
                    t = float(np.median(ms[2:]))
                    entry["kernels"][f"k_firefly_{name}<{radius}> rank {rank}"] = {
                        "ms": t, "gbps": float(BPP * w * h / (t * 1e-3) / 1e9),
                        "ps_per_model_byte": float(t * 1e9 / (BPP * w * h))}
        rk.test_schedule(ff_variant=0)
        scale = np.empty((h, w), np.float32)
        rk.firefly_clamp_device(t_in, t_out, t_sg, t_sout, t_fout)
        sync()
        assert _hip.hipMemcpy(scale.ctypes.data, t_fout, scale.nbytes, 2) == 0
        entry["pixels_clamped_at_defaults"] = float((scale < 1).mean())
        # the yardsticks, same buffers' sizes, same process
        ms_t, ms_p = [], []
        assert L.rt_device_denoise_var_pass_ms(ctx, 1, None, 0) == 0
        for _ in range(a.reps + 2):
            rk.temporal_accumulate_device(t_in, t_sg, t_nd, cam, t_out, t_sout, t_fout, (t_hin, t_hsg, t_hlen, t_nd))
            sync()
            ms_t.append(rk.device_last_kernel_ms())
            rk.denoise_var_device(t_in, t_sg, t_out, t_alb, t_nd, 1.0, {"passes": 1})
            sync()
            per = np.zeros(2)
            assert L.rt_device_denoise_var_pass_ms(ctx, -1, rt_amd.ptr(per), 2) == 2
            ms_p.append(float(per[0]))
        assert L.rt_device_denoise_var_pass_ms(ctx, 0, None, 0) == 0
        t, p = float(np.median(ms_t[2:])), float(np.median(ms_p[2:]))
        entry["k_temporal"] = {"ms": t, "gbps": float(BPP_TEMPORAL * w * h / (t * 1e-3) / 1e9),
                               "ps_per_model_byte": float(t * 1e9 / (BPP_TEMPORAL * w * h))}
        entry["k_dnv_prep"] = {"ms": p, "gbps": float(BPP_PREP * w * h / (p * 1e-3) / 1e9),
                               "ps_per_model_byte": float(p * 1e9 / (BPP_PREP * w * h))}
        res["sizes"][f"{w}x{h}"] = entry
        del rk
        for q in (t_alb, t_nd, t_in, t_hin, t_out, t_sg, t_hsg, t_sout, t_hlen, t_fout):
            _hip.hipFree(q)
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
