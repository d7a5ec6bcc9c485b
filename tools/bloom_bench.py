"""Timing of the bloom stage on the GPU: HIP-event ms of every launch of a call (rt_device_bloom_kernel_ms: the
product's sequence with an event in front of each launch and one behind the last) and of the whole call
(rt_bloom_device, rt_device_last_kernel_ms), with the LDS reduce kernel and with the direct one, at 1920x1080 and
3840x2160 and 1, 5 and 8 levels, the median of --reps rounds after two warm-up rounds; in the same process k_display
(float output, rt_device_display_kernel_ms) on the same frame as the yardstick.

The stage reads the frame twice (the first reduce, the composite) and writes it once, 48 B / pixel besides the pyramid
(a third of a frame written once and read about twice); k_display reads it once and writes it once, 32 B / pixel. So
the call's time is stated as a multiple of k_display's on the same buffers. small_share is the part of the call spent
in launches whose level has fewer than 64 x 64 texels (the reduce that writes such a level, the expand that updates
it): what fusing the small levels into one launch could save at most.

The input is a noisy gradient with a bright pixel in every 97th place, the default threshold, knee and intensity.

  python tools/bloom_bench.py [--reps 20] [--out profiles/bloom_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

import numpy as np

from stage_bench import REPO, _hip, dev_alloc, rt_amd, sync, test_frame, write_json

SMALL = 64 * 64


def level_sizes(w, h, levels):
    out = []
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bloom_bench.json"))
    a = ap.parse_args()
    L = rt_amd.lib()
    ctx = ctypes.c_void_p()
    rt_amd.check(L, L.rt_create(0, ctypes.byref(ctx)), None, "rt_create")
    vp = ctypes.c_void_p
    reps = a.reps + 2
    res = {"build": L.rt_build_id().decode(), "reps": a.reps, "sizes": {}}
    for w, h in ((1920, 1080), (3840, 2160)):
        nb = w * h * 16
        frame = test_frame(w, h)
        t_in, t_out, t_layer, t_out8 = dev_alloc(nb, frame), dev_alloc(nb), dev_alloc(nb), dev_alloc(nb // 4)
        entry = {"levels": {}}
        disp = np.zeros(6 * reps)
        rt_amd.check(L, L.rt_device_display_kernel_ms(ctx, w, h, vp(t_in), vp(t_in), vp(t_out), vp(t_out8), reps, rt_amd.ptr(disp)),
                     ctx, "rt_device_display_kernel_ms")
        k_display = float(np.median(disp[2 * reps + 2:3 * reps]))
        entry["k_display_ms"] = k_display
        for levels in (1, 5, 8):
            p = rt_amd.BloomParams(1.0, 0.5, 0.2, levels)
            sizes = level_sizes(w, h, levels)
            # launch j writes level: reduces 1..levels, expands levels-1..1, the composite the frame
            written = sizes + sizes[:-1][::-1] + [(w, h)]
            names = [f"reduce {k + 1}" for k in range(levels)] + [f"expand {k}" for k in range(levels - 1, 0, -1)] + ["composite"]
            lv = {}
            for name, lds, variant in (("lds", 1, 2), ("direct", 0, 1)):
                ms = np.zeros(reps * 2 * levels)
                rt_amd.check(L, L.rt_device_bloom_kernel_ms(ctx, w, h, vp(t_in), ctypes.byref(p), vp(t_out), vp(t_layer), lds, reps,
                                                            rt_amd.ptr(ms)), ctx, "rt_device_bloom_kernel_ms")
                per = np.median(ms.reshape(reps, 2 * levels)[2:], axis=0)
                rt_amd.check(L, L.rt_test_schedule(ctx, b"bloom_variant", float(variant)), ctx, "rt_test_schedule")
                call = []
                for _ in range(reps):
                    rt_amd.check(L, L.rt_bloom_device(ctx, w, h, vp(t_in), ctypes.byref(p), vp(t_out), vp(t_layer), None), ctx,
                                 "rt_bloom_device")
                    sync()
                    call.append(float(L.rt_device_last_kernel_ms(ctx)))
                rt_amd.check(L, L.rt_test_schedule(ctx, b"bloom_variant", 0.0), ctx, "rt_test_schedule")
                t = float(np.median(call[2:]))
                small = float(sum(m for m, (lw, lh) in zip(per, written) if lw * lh < SMALL))
                lv[name] = {"launch_ms": {n: float(m) for n, m in zip(names, per)}, "launches_sum_ms": float(per.sum()),
                            "reduce_sum_ms": float(per[:levels].sum()), "call_ms": t, "call_over_k_display": t / k_display,
                            "small_levels_ms": small, "small_share_of_launches": small / float(per.sum())}
            entry["levels"][str(levels)] = lv
        res["sizes"][f"{w}x{h}"] = entry
        for q in (t_in, t_out, t_layer, t_out8):
            _hip.hipFree(q)
    L.rt_destroy(ctx)
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
