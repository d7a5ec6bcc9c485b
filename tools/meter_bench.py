"""Timing of the exposure metering stage on the GPU: HIP-event ms of k_meter_lds and k_meter_direct alone
(rt_device_meter_kernel_ms: each launch between two events of its own, the histogram cleared in front of them) at
1920x1080 and 3840x2160 on three frames, and in the same process, interleaved round by round, k_display with the
float output (rt_device_display_kernel_ms) on the same pixel counts as the yardstick; the median of --reps rounds
after two warm-up rounds, with the smallest and largest round beside it.

Frames: "rendered", the Cornell box rendered linear at the size (1 sample, 3 bounces); "noise", log-uniform
luminances over 2^-20 .. 2^12, all 256 bins; "constant", every pixel (0.25, 0.5, 0.125), one bin.

Also: the LDS kernel under forced block counts (the grid cap's sweep), the whole stage (rt_meter_device: two clears
and the kernel) as rt_device_last_kernel_ms reports it, and what auto_exposure at the defaults returns for the
benchmark frames: cfg1 (Cornell 12 triangles, 256x256, 4 samples, 3 bounces) and cfg2's scene and camera (the dragon
stand-in at 1920x1080, 8 bounces) at --dragon-samples samples.

Byte model: 16 B / pixel read for the stage, 32 B / pixel (16 read, 16 written) for k_display.

  python tools/meter_bench.py [--reps 20] [--dragon-samples 8] [--kernels-only] [--out profiles/meter_bench.json]

RT_HIP_LIB names another build of the library (make variant V=peel2 DEFS=-DMT_PEEL=2), as for every tool here.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from stage_bench import REPO, _hip, cornell_kernel, dev_alloc, rt_amd, scenes, stat, sync, write_json

SWEEP = (128, 256, 512, 1024, 2048, 4096)


def benchmark_exposure(cfg: str, samples: int | None = None) -> dict:
    import bench
    P, sky, cam17 = bench.build_inputs(cfg)
    _, _, _, W, H, spp, nb, desc = bench.CONFIGS[cfg]
    spp = samples or spp
    fb = rt_amd.Image(W, H)
    sky_img = rt_amd.Image.from_rgb(sky)
    rk = rt_amd.RenderKernel(W, H, spp, nb, fb, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices,
                             None, rt_amd.BVH(P.triangles), sky_img, rt_amd.compute_env_map_cdf(sky_img))
    rk.set_camera(rt_amd.Camera(cam17[:16], cam17[16]))
    rk.render_linear()
    r = rk.auto_exposure(fb, full=True)
    s = rt_amd.meter_stats(r.pop("hist"))
    shown = rk.display(fb, exposure=r["exposure"], want="rgba8")[..., :3]
    at15 = rk.display(fb, exposure=1.5, want="rgba8")[..., :3]
    return dict(r, workload=f"{desc}, rendered at {spp} samples", W=W, H=H, samples=spp,
                **{k: s[k] for k in ("counted", "under", "over", "nonpositive", "nonfinite")},
                mean_byte_at_auto=float(shown.mean()), mean_byte_at_1_5=float(at15.mean()))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dragon-samples", type=int, default=8)
    ap.add_argument("--kernels-only", action="store_true", help="leave out the benchmark frames' auto_exposure")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "meter_bench.json"))
    a = ap.parse_args()
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    sky = rt_amd.Image.from_rgb(scenes.make_sky("S"))
    res = {"build": rt_amd.lib().rt_build_id().decode(), "reps": a.reps, "bytes_per_pixel": 16.0,
           "bytes_per_pixel_k_display": 32.0, "sizes": {}}
    for w, h in ((1920, 1080), (3840, 2160)):
        rk = cornell_kernel(w, h, 1, 3)
        L, ctx = rk.L, rk.ctx
        nb = w * h * 16
        rng = np.random.default_rng(0)
        noise = np.empty((h, w, 4), np.float32)
        noise[..., :3] = np.exp2(rng.uniform(-20.0, 12.0, (h, w, 1))).astype(np.float32)
        noise[..., 3] = 1.0
        const = np.tile(np.array([0.25, 0.5, 0.125, 1.0], np.float32), (h, w, 1))
        frames = {"rendered": dev_alloc(nb, np.zeros((h, w, 4), np.float32)), "noise": dev_alloc(nb, noise),
                  "constant": dev_alloc(nb, const)}
        rk.render_linear_device(frames["rendered"])
        sync()
        d_state, d_out, d_out8, d_hist = dev_alloc(nb, np.zeros((h, w, 4), np.float32)), dev_alloc(nb), dev_alloc(nb // 4), \
            dev_alloc(4 * rt_amd.METER_WORDS)
        hist = np.empty(rt_amd.METER_WORDS, np.uint32)
        entry = {"frames": {}}
        ms = {f: {"k_meter_direct": [], "k_meter_lds": [], "k_display float out": [], "stage": []} for f in frames}
        two, six = np.zeros(2), np.zeros(6)
        for _ in range(a.reps + 2):  # round by round: every kernel on every frame once per round
            for f, d_in in frames.items():
                assert L.rt_device_meter_kernel_ms(ctx, w, h, d_in, d_hist, 0, 1, rt_amd.ptr(two)) == 0
                assert L.rt_device_display_kernel_ms(ctx, w, h, d_in, d_state, d_out, d_out8, 1, rt_amd.ptr(six)) == 0
                rk.meter_device(d_in, d_hist)
                sync()
                ms[f]["k_meter_direct"].append(two[0])
                ms[f]["k_meter_lds"].append(two[1])
                ms[f]["k_display float out"].append(six[2])
                ms[f]["stage"].append(rk.device_last_kernel_ms())
        for f, d_in in frames.items():
            e = {k: stat(v) for k, v in ms[f].items()}
            for k in ("k_meter_direct", "k_meter_lds"):
                e[k]["gbps"] = float(16.0 * w * h / (e[k]["ms"] * 1e-3) / 1e9)
            e["k_display float out"]["gbps"] = float(32.0 * w * h / (e["k_display float out"]["ms"] * 1e-3) / 1e9)
            sweep = {}
            for blocks in SWEEP:
                t = np.zeros(2 * (a.reps + 2))
                assert L.rt_device_meter_kernel_ms(ctx, w, h, d_in, d_hist, blocks, a.reps + 2, rt_amd.ptr(t)) == 0
                sweep[str(blocks)] = {"k_meter_direct": stat(t[:a.reps + 2])["ms"], "k_meter_lds": stat(t[a.reps + 2:])["ms"]}
            e["blocks_sweep_ms"] = sweep
            rk.meter_device(d_in, d_hist)
            sync()
            assert _hip.hipMemcpy(hist.ctypes.data, d_hist, hist.nbytes, 2) == 0
            s = rt_amd.meter_stats(hist)
            e["bins_nonzero"] = int((s["bins"] > 0).sum())
            e["largest_bin_share"] = float(s["bins"].max() / max(s["counted"], 1))
            entry["frames"][f] = e
        fr = entry["frames"]
        prod = "k_meter_lds"  # (mt_variant 0; rt_meter.hip rt_backend_meter)
        disp = fr["rendered"]["k_display float out"]
        entry["product_kernel"] = prod
        entry["rendered_vs_k_display"] = {
            "kernel_ms": fr["rendered"][prod]["ms"], "k_display_ms": disp["ms"], "k_display_spread_ms": disp["max"] - disp["min"],
            "within_bound": bool(fr["rendered"][prod]["ms"] <= disp["ms"] + (disp["max"] - disp["min"]))}
        entry["constant_over_rendered"] = {k: fr["constant"][k]["ms"] / fr["rendered"][k]["ms"]
                                           for k in ("k_meter_direct", "k_meter_lds")}
        res["sizes"][f"{w}x{h}"] = entry
        del rk
        for q in (*frames.values(), d_state, d_out, d_out8, d_hist):
            _hip.hipFree(q)
    if not a.kernels_only:
        res["auto_exposure_at_defaults"] = {"cfg1": benchmark_exposure("cfg1"),
                                            "cfg2": benchmark_exposure("cfg2", a.dragon_samples)}
    write_json(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
