"""What the stage bench tools (tools/*_bench.py) share: the import paths, plain HIP allocations, the rounds' statistics,
the Cornell kernel and the test frame they time on, the two yardsticks they quote beside a stage, and the result file."""
from __future__ import annotations

import contextlib
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "sycl-ray-tracing_amd"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rt_amd  # noqa: E402
import scenes  # noqa: E402

vp = ctypes.c_void_p
_hip = ctypes.CDLL("libamdhip64.so")
_hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
_hip.hipFree.argtypes = [ctypes.c_void_p]
_hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]


def dev_alloc(nbytes: int, src: np.ndarray | None = None) -> int:
    p = ctypes.c_void_p()
    assert _hip.hipMalloc(ctypes.byref(p), nbytes) == 0
    if src is not None:
        assert _hip.hipMemcpy(p, src.ctypes.data, src.nbytes, 1) == 0
    return p.value


def sync():
    assert _hip.hipDeviceSynchronize() == 0


def stat(ms, warm=2):
    """The rounds after the first `warm`: median, smallest and largest."""
    ms = np.asarray(ms[warm:])
    return {"ms": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max())}


def cornell_kernel(w, h, spp=1, bounces=1, camera=None):
    """The 12-triangle Cornell box under the flat sky at w x h, from its preset camera (or `camera`)."""
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    sky = rt_amd.Image.from_rgb(scenes.make_sky("S"))
    rk = rt_amd.RenderKernel(w, h, spp, bounces, rt_amd.Image(1, 1), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), sky, None)
    rk.set_camera(camera or rt_amd.Camera.preset("cornell"))
    return rk


def test_frame(w, h, rng=None):
    """[h, w, 4] float32 noise in [0, 1) with rgb 50.0 in every 97th pixel, from rng (default_rng(0) if none is given)."""
    frame = (rng or np.random.default_rng(0)).random((h, w, 4), dtype=np.float32)
    frame.reshape(-1, 4)[::97, :3] = 50.0
    return frame


@contextlib.contextmanager
def yardsticks(rk, w, h):
    """The two figures a stage is quoted beside, on its own frame in its own process: one à-trous pass at w x h
    (rt_denoise_device with one pass under dn_variant 1, rt_device_denoise_pass_ms) and k_display's 8-bit output
    (rt_device_display_kernel_ms). Gives round(d_in, d_tmp, d_alb, d_nd, d_out8) -> (pass ms, display ms)."""
    L, ctx = rk.L, rk.ctx
    six, one = np.zeros(6), np.zeros(1)

    def one_round(d_in, d_tmp, d_alb, d_nd, d_out8):
        rk.denoise_device(d_in, d_tmp, d_alb, d_nd, 1.0, {"passes": 1}, width=w, height=h)
        sync()
        assert L.rt_device_denoise_pass_ms(ctx, -1, rt_amd.ptr(one), 1) == 1
        assert L.rt_device_display_kernel_ms(ctx, w, h, vp(d_in), vp(d_tmp), vp(d_tmp), vp(d_out8), 1, rt_amd.ptr(six)) == 0
        return float(one[0]), float(six[3])
    rk.test_schedule(dn_variant=1)
    assert L.rt_device_denoise_pass_ms(ctx, 1, None, 0) == 0
    try:
        yield one_round
    finally:
        assert L.rt_device_denoise_pass_ms(ctx, 0, None, 0) == 0
        rk.test_schedule(dn_variant=0)


def write_json(res, path):
    """The result as one line on stdout and, indented, in `path`."""
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
