"""The first-hit G-buffer on the gfx950 library (rt_gbuffer.hip), bit for bit against the hostsim build
(tests/test_gbuffer.py holds that one to rt_query and rt_render_features): every kernel variant
(rt_test_schedule "gb_variant": 0 the product's, 1 plain rounds, 2 per-quad refill) at sizes across the
kernels' boundaries, in the host form and in the device form on a stream of its own with guard words behind
each output; fallback lists either side of one octet, one wave and one block of octets (gb_force_every);
the NULL-list form of the octet kernel; workspace growth; a render on either side of a call; the filters
fed from either guide source; the command line's --guides."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import gbuffer_cases as gc
import rt_cases
import scenes
from conftest import parsed_scene

import rt_amd

pytestmark = pytest.mark.gpu

VARIANTS = [0, 1, 2]
SENTINEL = 0x5A5A5A5A
GUARD_WORDS = 1024


@pytest.fixture(autouse=True)
def _reset():
    yield
    gc.reset_schedules(False)


class _Stream:
    def __init__(self):
        from hip_mem import hip
        self.hip = hip()
        self.h = ctypes.c_void_p()
        assert self.hip.hipStreamCreate(ctypes.byref(self.h)) == 0

    def sync(self):
        assert self.hip.hipStreamSynchronize(self.h) == 0

    def close(self):
        assert self.hip.hipStreamDestroy(self.h) == 0


def _device_form(rk, size, stream, ids: bool, exact: bool = False):
    """gbuffer_device on `stream` into sentinel-filled buffers with GUARD_WORDS behind each output: the
    outputs, after the guard words are seen untouched."""
    from hip_mem import DeviceBuffer
    w, h = size
    n = w * h
    words = [4 * n, 4 * n] + ([2 * n] if ids else [])
    bufs = [DeviceBuffer((k + GUARD_WORDS) * 4) for k in words]
    for b, k in zip(bufs, words):
        b.upload(np.full(k + GUARD_WORDS, SENTINEL, np.int32))
    rk.gbuffer_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr if ids else None, exact=exact, stream=stream.h.value,
                      size=size)
    assert rk.last_kernel_ms() == -1.0
    stream.sync()
    assert rk.device_last_kernel_ms() > 0.0
    out = []
    for b, k in zip(bufs, words):
        got = b.download((k + GUARD_WORDS,), np.int32)
        assert (got[k:] == SENTINEL).all(), f"{size}: wrote past its {k} words"
        out.append(got[:k])
    res = [out[0].view(np.float32).reshape(h, w, 4), out[1].view(np.float32).reshape(h, w, 4)]
    if ids:
        res.append(out[2].reshape(h, w, 2))
    return tuple(res)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scene,kind", gc.CASES)
def test_gpu_sizes_both_forms_equal_hostsim(scene, kind, variant):
    rk = gc.kernel(scene, False, kind)
    rk.test_schedule(gb_variant=variant)
    stream = _Stream()
    for size in gc.GPU_SIZES:
        want = gc.host_reference(scene, size, kind)
        what = f"{scene} {kind} {size} variant {variant}"
        gc.assert_same(rk.gbuffer(size, ids=True), want, what + ": host form")
        assert rk.last_kernel_ms() > 0.0
        routed = rk.gbuffer_last_exact()
        assert (routed <= size[0] * size[1] // 10 + 1) if gc.camera_inside(scene, kind) else routed == size[0] * size[1]
        gc.assert_same(rk.gbuffer(size), want[:2], what + ": host form, no ids")
        gc.assert_same(_device_form(rk, size, stream, True), want, what + ": device form")
        gc.assert_same(_device_form(rk, size, stream, False), want[:2], what + ": device form, no ids")
    stream.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scene,kind", [("dragon", "plain"), ("cornell", "near")])
def test_gpu_forced_lists_run_the_octet_kernel(scene, kind, variant):
    """Fallback lists of 1, 7, 9, 33, 257 and all 8710 entries at 130 x 67: the output stays hostsim's and,
    the exact walk being rt_render_features' walk, equals features() on the GPU."""
    rk = gc.kernel(scene, False, kind)
    rk.test_schedule(gb_variant=variant)
    want = gc.host_reference(scene, gc.BIG, kind)
    feat = rk.features(gc.BIG)
    gc.assert_same(want[:2], feat, f"{scene} {kind}: hostsim gbuffer vs features on the GPU")
    for every, entries in gc.FORCE.items():
        rk.test_schedule(gb_force_every=every)
        got = rk.gbuffer(gc.BIG, ids=True)
        n_exact = rk.gbuffer_last_exact()
        assert entries <= n_exact <= entries + 8710 // 10, (every, n_exact)
        gc.assert_same(got, want, f"{scene} {kind} variant {variant}: gb_force_every={every}")
        gc.assert_same(got[:2], feat, f"{scene} {kind} variant {variant}: gb_force_every={every} vs features")


@pytest.mark.parametrize("scene", gc.SCENES)
def test_gpu_null_list_form(scene):
    """A far camera (33 x 9) and exact=True (130 x 67): tickets over every pixel."""
    stream = _Stream()
    far = gc.kernel(scene, False, "far")
    want = gc.host_reference(scene, gc.FAR_SIZE, "far")
    gc.assert_same(far.gbuffer(gc.FAR_SIZE, ids=True), want, f"{scene}: far camera")
    assert far.gbuffer_last_exact() == gc.FAR_SIZE[0] * gc.FAR_SIZE[1]
    gc.assert_same(far.gbuffer(gc.FAR_SIZE), far.features(gc.FAR_SIZE), f"{scene}: far camera vs features")
    gc.assert_same(_device_form(far, gc.FAR_SIZE, stream, True), want, f"{scene}: far camera, device form")
    rk = gc.kernel(scene, False)
    want = gc.host_reference(scene, gc.BIG)
    gc.assert_same(rk.gbuffer(gc.BIG, exact=True, ids=True), want, f"{scene}: exact=True")
    assert rk.gbuffer_last_exact() == gc.BIG[0] * gc.BIG[1]
    gc.assert_same(rk.gbuffer(gc.BIG, exact=True), rk.features(gc.BIG), f"{scene}: exact=True vs features")
    gc.assert_same(_device_form(rk, gc.BIG, stream, True, exact=True), want, f"{scene}: exact=True, device form")
    stream.close()


@pytest.mark.parametrize("kind", ["spheres", "brute"])
def test_gpu_sphere_and_brute_contexts(kind):
    rk = gc.kernel("cornell", False, kind)
    got = rk.gbuffer(gc.BIG, ids=True)
    assert rk.gbuffer_last_exact() == gc.BIG[0] * gc.BIG[1]
    gc.assert_same(got, gc.host_reference("cornell", gc.BIG, kind), f"{kind}: gbuffer vs hostsim")
    gc.assert_same(got[:2], rk.features(gc.BIG), f"{kind}: gbuffer vs features")


def test_gpu_workspace_grows_between_calls():
    """A fresh context: a small frame, then a larger one (list and spill areas grow), forced and exact."""
    P = parsed_scene("dragon")
    rk = rt_amd.RenderKernel(4, 4, 1, 1, rt_amd.Image(4, 4), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), rt_amd.Image(1, 1), None)
    rk.set_camera(gc.camera("dragon"))
    rk.test_schedule(gb_force_every=3)
    for exact in (False, True):
        for size in ((5, 3), gc.BIG):
            gc.assert_same(rk.gbuffer(size, exact=exact, ids=True), gc.host_reference("dragon", size),
                           f"{size} exact={exact}")


def test_gpu_gbuffer_leaves_the_render_alone(cameras):
    """A 64x64 Cornell render, a G-buffer on the same context, the render again: equal frames."""
    P = parsed_scene("cornell")
    W, H = 64, 64
    fb = rt_amd.Image(W, H)
    rk = rt_amd.RenderKernel(W, H, 4, 3, fb, P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles),
                             rt_amd.Image.from_rgb(rt_cases.sky("S")), None)
    rk.set_camera(gc.camera("cornell", "near"))
    start = fb.pixels.copy()
    rk.render()
    first = fb.pixels.copy()
    assert not np.array_equal(first, start)
    rk.test_schedule(gb_force_every=5)
    a = rk.gbuffer(ids=True)
    fb.pixels[...] = start
    rk.render()
    assert np.array_equal(fb.pixels.view(np.uint32), first.view(np.uint32))
    gc.assert_same(rk.gbuffer(ids=True), a, "after the second render")
    gc.assert_same(a[:2], rk.features(), "gbuffer vs features")


def test_gpu_filters_fed_from_either_source(cameras):
    """denoise_var and upscale on Cornell 64x64: the same bits from gbuffer() and from features()."""
    P = parsed_scene("cornell")
    W, H = 64, 64
    fb = rt_amd.Image(W, H)
    rk = rt_amd.RenderKernel(W, H, 4, 3, fb, P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles),
                             rt_amd.Image.from_rgb(rt_cases.sky("S")), None)
    for kind in ("plain", "near"):
        rk.set_camera(gc.camera("cornell", kind))
        rk.render_linear()
        lum = fb.pixels[..., :3].mean(axis=2)
        sigma = np.ascontiguousarray(0.1 * lum + 0.01, dtype=np.float32)
        full = (2 * W, 2 * H)
        feat, feat_full = rk.features(), rk.features(size=full)
        walk, walk_full = rk.gbuffer(), rk.gbuffer(size=full)
        with np.errstate(all="ignore"):
            a = rk.denoise_var(fb, sigma, 1.0, guides=feat)
            b = rk.denoise_var(fb, sigma, 1.0, guides=walk)
            rk.guide_source = "walks"
            c = rk.denoise_var(fb, sigma, 1.0)
            rk.guide_source = "exact"
        assert np.array_equal(gc.bits(a.pixels), gc.bits(b.pixels)), kind
        assert np.array_equal(gc.bits(a.pixels), gc.bits(c.pixels)), kind
        ua = rk.upscale(fb, *feat, *feat_full)
        ub = rk.upscale(fb, *walk, *walk_full)
        assert np.array_equal(gc.bits(ua.pixels), gc.bits(ub.pixels)), kind


NAMES = ("RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png")


def test_gpu_cli_guides_walks_writes_the_same_pngs(tmp_path):
    import os
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(rt_amd.__file__)))
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    outs = {}
    for name, flags in (("plain", []), ("walks", ["--guides=walks"])):
        outs[name] = tmp_path / name
        r = subprocess.run([sys.executable, "-m", "rt_amd.cli", scenes.scene_path("cornell"), f"--sky={hdr}", "--w=48",
                            "--h=32", "--samples=2", "--bounces=2", "--camera=cornell", f"--out={outs[name]}",
                            "--upscale=2", *flags], capture_output=True, text=True, timeout=110, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
    for n in NAMES:
        assert (outs["plain"] / n).read_bytes() == (outs["walks"] / n).read_bytes(), n
