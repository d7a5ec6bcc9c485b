"""What progressive passes cost on cfg2 (1920x1080 x 64 spp x 8 bounces): the whole frame as
1x64, 4x16, 16x4 and 64x1 passes (rt_progress_begin .. the final rt_progress_resolve_device)
beside rt_render_device of the same frame, one k_resolve, and the build that ran.

  python tools/progressive_bench.py [--reps 3] [--out profiles/progressive_bench.json]

Wall-clock ms around the calls and a device synchronize, as tools/knob_probe.py times a frame;
every pass pays the frame's sparse tail again, so small passes cost more: the file says how much.
The one requirement it checks: the 1x64 progression (the render's launches minus k_tonemap plus
k_resolve) exceeds rt_render_device by no more than the repeat-to-repeat spread of this run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "sycl-ray-tracing_amd"), os.path.join(REPO, "tools"), REPO):
    sys.path.insert(0, p)

SPLITS = ((1, 64), (4, 16), (16, 4), (64, 1))  # passes x samples per pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/progressive_bench.json")
    args = ap.parse_args()
    import torch

    import bench
    import rt_amd
    from rt_amd import _capi

    P, sky, cam17 = bench.build_inputs("cfg2")
    _, _, _, W, H, spp, nb, _ = bench.CONFIGS["cfg2"]
    assert all(n * k == spp for n, k in SPLITS)
    rk = rt_amd.RenderKernel(W, H, spp, nb, rt_amd.Image(W, H), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), rt_amd.Image.from_rgb(sky), None, device=0)
    rk.set_camera(rt_amd.Camera(cam17[:16], cam17[16]))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    blank = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    blank[..., 3] = 1.0  # (the bound Image's value: the progression's base)
    d_fb, d_out = blank.clone(), torch.empty_like(blank)

    def render_ms():
        d_fb.copy_(blank)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        rk.render_device(d_fb.data_ptr(), stream=stream)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def progression_ms(passes, k):
        rk.progress_begin()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(passes):
            rk.progress_advance(k, stream)
        rk.progress_resolve_device(d_out.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    render_ms()  # warm-up: buffers sized, code objects loaded
    progression_ms(1, spp)
    same = bool(torch.equal(d_out.view(torch.int32), d_fb.view(torch.int32)))
    res = {"render_device_ms": [], **{f"{n}x{k}_ms": [] for n, k in SPLITS}}
    for _ in range(args.reps):  # (the measurements alternate, so drift lands on all alike)
        res["render_device_ms"].append(round(render_ms(), 2))
        for n, k in SPLITS:
            res[f"{n}x{k}_ms"].append(round(progression_ms(n, k), 2))
            same = same and bool(torch.equal(d_out.view(torch.int32), d_fb.view(torch.int32)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    resolve = []
    for _ in range(5):
        ev[0].record()
        rk.progress_resolve_device(d_out.data_ptr(), stream)
        ev[1].record()
        torch.cuda.synchronize(dev)
        resolve.append(round(ev[0].elapsed_time(ev[1]), 4))
    rk.progress_end()
    r = res["render_device_ms"]
    spread = round(max(max(v) - min(v) for v in res.values()), 2)
    excess = round(min(res[f"1x{spp}_ms"]) - min(r), 2)
    out = {"what": f"cfg2 {W}x{H} x {spp} spp x {nb} bounces on one MI355X: rt_render_device, and the same frame as a "
                   f"progression of n passes of k samples (begin untimed; the passes and the final "
                   f"rt_progress_resolve_device timed), wall-clock ms, {args.reps} repeats alternating",
           "build": _capi.lib().rt_build_id().decode(),
           "ms": res,
           "min_ms": {k: min(v) for k, v in res.items()},
           "cost_over_render_device": {k: round(min(v) / min(r), 3) for k, v in res.items() if k != "render_device_ms"},
           "k_resolve_ms": resolve,
           "final_words_equal_render_device": same,
           "one_pass": {"excess_ms": excess, "repeat_spread_ms": spread, "within_spread": excess <= spread}}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
