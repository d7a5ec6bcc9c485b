"""The edge-avoiding à-trous filter (rt_denoise): hostsim against a float64 numpy model of
the formula in include/rt_hip.h, its exact properties and argument errors, the CLI; on the
GPU, the gfx950 kernels against hostsim, bitwise.

Synthetic inputs: seeded uniform noise in [0, 1] over a two-tone background; guides of two
half-planes with orthogonal unit normals, different t and albedo, plus a block of misses."""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import rt_amd
import rt_cases
import scenes
from rt_amd import DenoiseParams, ptr
from stage_gpu import forced_variant

SIZES = [(1, 1), (5, 3), (37, 29), (130, 67)]
HK = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])

# |hostsim - float64 model| over SIZES x passes 1..5 x {guides, colour only}: the largest
# measured is 4.41e-7 (130x67, 5 passes, guides; float32 sums and products against float64, rt_libm's expf against
# exp); the bound is 4x that. (The project's bar for a visible pixel change is 1e-4.)
MODEL_MEASURED = 4.41e-7
MODEL_TOL = 4 * MODEL_MEASURED


def synth(w, h, seed=1):
    """(rgba, albedo, normal_depth) float32 [h, w, 4]."""
    rng = np.random.default_rng(seed)
    left = (np.arange(w) < (w + 1) // 2)[None, :].repeat(h, 0)
    rgba = np.empty((h, w, 4), np.float32)
    rgba[..., :3] = np.where(left[..., None], 0.2, 0.7) + 0.3 * rng.random((h, w, 3))
    rgba[..., 3] = rng.random((h, w))
    nd = np.zeros((h, w, 4), np.float32)
    alb = np.zeros((h, w, 4), np.float32)
    nd[left] = (1, 0, 0, 2.0)
    nd[~left] = (0, 1, 0, 3.5)
    nd[..., 3] += (0.05 * rng.random((h, w))).astype(np.float32)
    alb[left] = (0.8, 0.1, 0.1, 0)
    alb[~left] = (0.1, 0.1, 0.8, 0)
    miss = np.zeros((h, w), bool)
    miss[h // 3:h // 3 + max(1, h // 4), w // 4:w // 4 + max(1, w // 3)] = w > 1
    nd[miss] = (0, 0, 0, -1)
    alb[miss] = 0
    return rgba, alb, nd


def params(passes=5, sc=1.0, sn=0.3, sa=0.1, st=0.1):
    return DenoiseParams(passes, sc, sn, sa, st)


def model(rgba, alb, nd, p, blend):
    """float64 restatement of the filter."""
    h, w = rgba.shape[:2]
    c = rgba[..., :3].astype(np.float64)
    guides = alb is not None
    if guides:
        n, t, a = nd[..., :3].astype(np.float64), nd[..., 3].astype(np.float64), alb[..., :3].astype(np.float64)
        hit = t > 0
    for i in range(p.passes):
        s = 1 << i
        fin = np.isfinite(c).all(-1)
        num = np.zeros_like(c)
        den = np.zeros((h, w))
        sc = float(p.sigma_color) * 2.0 ** -i
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs = np.arange(h) + dy * s, np.arange(w) + dx * s
                vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
                if not vy.any() or not vx.any():
                    continue
                P = np.ix_(np.where(vy)[0], np.where(vx)[0])
                Q = np.ix_(ys[vy], xs[vx])
                ok = fin[Q] & fin[P]
                with np.errstate(all="ignore"):
                    e = ((c[P] - c[Q]) ** 2).sum(-1) / sc ** 2
                    if guides:
                        e = e + ((n[P] - n[Q]) ** 2).sum(-1) / float(p.sigma_normal) ** 2
                        e = e + ((a[P] - a[Q]) ** 2).sum(-1) / float(p.sigma_albedo) ** 2
                        both = hit[P] & hit[Q]
                        r = np.where(both, (t[P] - t[Q]) / np.where(both, np.maximum(t[P], t[Q]), 1.0), 0.0)
                        e = e + r ** 2 / float(p.sigma_depth) ** 2
                        ok &= hit[P] == hit[Q]
                    wgt = np.where(ok, HK[dy + 2] * HK[dx + 2] * np.exp(-e), 0.0)
                    num[P] += wgt[..., None] * np.where(ok[..., None], c[Q], 0.0)
                den[P] += wgt
        with np.errstate(all="ignore"):
            c = np.where(fin[..., None], num / np.where(den > 0, den, 1.0)[..., None], c)
    out = np.empty((h, w, 4))
    with np.errstate(all="ignore"):
        out[..., :3] = float(np.float32(blend)) * c + float(np.float32(1.0) - np.float32(blend)) * rgba[..., :3]
    out[..., 3] = 1.0
    return out


_ctx = {}


def ctx(hostsim=True):
    """One bare context per library: rt_denoise needs no scene."""
    if hostsim not in _ctx:
        L = rt_amd.lib(hostsim)
        h = ctypes.c_void_p()
        rt_amd.check(L, L.rt_create(0, ctypes.byref(h)), None, "rt_create")
        _ctx[hostsim] = (L, h)
    return _ctx[hostsim]


def denoise(rgba, alb, nd, p, blend, hostsim=True, code=False):
    L, h = ctx(hostsim)
    H, W = rgba.shape[:2]
    out = np.full((H, W, 4), -5.0, np.float32)
    rc = L.rt_denoise(h, W, H, ptr(rgba), ptr(alb), ptr(nd), ctypes.byref(p) if p is not None else None,
                      ctypes.c_float(blend), ptr(out))
    if code:
        return rc
    rt_amd.check(L, rc, h, "rt_denoise")
    return out


_host_cache = {}


def host_result(w, h, passes, guides, blend):
    """hostsim's output for a synthetic case, computed once and shared (read-only)."""
    key = (w, h, passes, guides, blend)
    if key not in _host_cache:
        rgba, alb, nd = synth(w, h)
        out = denoise(rgba, alb if guides else None, nd if guides else None, params(passes), blend)
        out.setflags(write=False)
        _host_cache[key] = out
    return _host_cache[key]


@pytest.mark.parametrize("guides", [True, False])
@pytest.mark.parametrize("passes", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("w,h", SIZES)
def test_hostsim_matches_float64_model(w, h, passes, guides):
    rgba, alb, nd = synth(w, h)
    got = host_result(w, h, passes, guides, 1.0)
    want = model(rgba, alb if guides else None, nd if guides else None, params(passes), 1.0)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"denoise model {w}x{h} passes {passes} guides {guides}: max abs err {err:.3e}")
    assert MODEL_TOL <= 1e-4
    assert err <= MODEL_TOL


def test_blend_zero_returns_input_bitwise():
    rgba, alb, nd = synth(37, 29)
    out = denoise(rgba, alb, nd, params(3), 0.0)
    np.testing.assert_array_equal(out[..., :3].view(np.uint32), rgba[..., :3].view(np.uint32))
    assert np.all(out[..., 3] == 1.0)


def test_huge_sigmas_are_the_b3_spline_blur():
    rgba, alb, nd = synth(37, 29)
    nd[..., 3] = np.abs(nd[..., 3])  # all hit: with a miss block the hit / miss taps are still skipped
    out = denoise(rgba, alb, nd, params(1, 1e18, 1e18, 1e18, 1e18), 1.0)
    c = rgba[..., :3].astype(np.float64)
    h, w = c.shape[:2]
    num, den = np.zeros_like(c), np.zeros((h, w))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            for y in range(max(0, -dy), min(h, h - dy)):
                xs = np.arange(max(0, -dx), min(w, w - dx))
                num[y, xs] += HK[dy + 2] * HK[dx + 2] * c[y + dy, xs + dx]
                den[y, xs] += HK[dy + 2] * HK[dx + 2]
    blur = num / den[..., None]
    assert np.abs(out[..., :3] - blur).max() <= MODEL_TOL


def test_edges_are_closed():
    """sigma_normal 0.1 across orthogonal normals: e >= 2 / 0.01 = 200 and expf(-200) is 0 in
    float32, so every output pixel lies within [min, max] of its own side's inputs; the miss
    block is closed off from the hits likewise (those taps are skipped)."""
    w, h = 37, 29
    rgba, alb, nd = synth(w, h)
    out = denoise(rgba, alb, nd, params(5, 1e18, 0.1, 1e18, 1e18), 1.0)
    miss = nd[..., 3] < 0
    left = (np.arange(w) < (w + 1) // 2)[None, :].repeat(h, 0)
    assert miss.any()
    for region in (left & ~miss, ~left & ~miss, miss):
        src, got = rgba[region][:, :3], out[region][:, :3]
        assert np.all(got >= src.min(0)) and np.all(got <= src.max(0))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_pixel_stays_alone(bad):
    rgba, alb, nd = synth(37, 29)
    rgba[10, 12, 1] = bad
    out = denoise(rgba, alb, nd, params(5), 1.0)
    nf = ~np.isfinite(out[..., :3]).all(-1)
    assert nf.sum() == 1 and nf[10, 12]


def test_nan_guide_gets_no_weight():
    """A NaN in a guide record: every tap that touches it has e = NaN and is given no weight,
    so the pixel itself passes through (no tap left, its own included) and no other pixel
    turns non-finite; away from its taps' reach nothing changes."""
    rgba, alb, nd = synth(37, 29)
    clean = denoise(rgba, alb, nd, params(2), 1.0)
    nd2 = nd.copy()
    nd2[10, 12, 0] = np.nan
    out = denoise(rgba, alb, nd2, params(2), 1.0)
    assert np.isfinite(out).all()
    np.testing.assert_array_equal(out[10, 12, :3].view(np.uint32), rgba[10, 12, :3].view(np.uint32))
    far = np.ones((29, 37), bool)
    far[max(0, 10 - 6):10 + 7, max(0, 12 - 6):12 + 7] = False  # reach of 2 passes: 2 * (1 + 2)
    np.testing.assert_array_equal(out[far].view(np.uint32), clean[far].view(np.uint32))
    assert (out != clean).any()


def test_argument_errors():
    rgba, alb, nd = synth(5, 3)
    L, h = ctx(True)

    def rc(p=None, blend=1.0, a=alb, n=nd):
        r = denoise(rgba, a, n, p if p is not None else params(), blend, code=True)
        assert r == 0 or L.rt_last_error(h)
        return r

    assert rc() == 0
    for passes in (0, 11, -1):
        assert rc(params(passes)) == rt_amd.RT_ERR_ARG
    for bad in (0.0, -1.0, np.nan, np.inf):
        for k in range(4):
            s = [1.0, 0.3, 0.1, 0.1]
            s[k] = bad
            assert rc(params(3, *s)) == rt_amd.RT_ERR_ARG
    for blend in (np.nan, np.inf, -np.inf):
        assert rc(blend=blend) == rt_amd.RT_ERR_ARG
    assert rc(a=None) == rt_amd.RT_ERR_ARG
    assert rc(n=None) == rt_amd.RT_ERR_ARG
    assert L.rt_denoise(h, 5, 3, ptr(rgba), None, None, None, ctypes.c_float(1.0), ptr(rgba)) == rt_amd.RT_ERR_ARG
    assert L.rt_last_error(h)
    tall = np.zeros((262141, 1, 4), np.float32)  # one row past what the kernels' grids tile
    assert L.rt_denoise(h, 1, 262141, ptr(tall), None, None, None, ctypes.c_float(1.0),
                        ptr(np.zeros_like(tall))) == rt_amd.RT_ERR_ARG
    assert b"262140" in L.rt_last_error(h)
    d = DenoiseParams()
    L.rt_denoise_default_params(ctypes.byref(d))
    assert 1 <= d.passes <= 10 and min(d.sigma_color, d.sigma_normal, d.sigma_albedo, d.sigma_depth) > 0


def _cornell_kernel(cameras, manifest, hostsim, W, H, spp, bounces):
    e = rt_cases.golden_case("cornell32_128", manifest)
    return rt_cases.make_kernel(e, cameras, hostsim, W=W, H=H, spp=spp, bounces=bounces)


def test_quality_denoised_is_closer_to_converged(cameras, manifest):
    """Cornell 64x64, 8 bounces: 16 spp denoised (defaults, guides) against 512 spp."""
    rk, fb = _cornell_kernel(cameras, manifest, True, 64, 64, 512, 8)
    rk.render()
    ref = fb.pixels[..., :3].astype(np.float64)
    rk16, fb16 = _cornell_kernel(cameras, manifest, True, 64, 64, 16, 8)
    rk16.render()
    den = rk16.denoise()

    def rmse(a):
        return float(np.sqrt(((a[..., :3].astype(np.float64) - ref) ** 2).mean()))

    print(f"rmse 16 spp {rmse(fb16.pixels):.5f} denoised {rmse(den.pixels):.5f}")
    assert rmse(den.pixels) < rmse(fb16.pixels)


def test_cli_writes_the_four_images(tmp_path, cameras):
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    obj = scenes.scene_path("cornell12")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(rt_amd.__file__)))
    r = subprocess.run([sys.executable, "-m", "rt_amd.cli", obj, f"--sky={hdr}", "--w=16", "--h=12", "--samples=1",
                        "--bounces=2", "--hostsim", "--camera=cornell", f"--out={tmp_path}"], capture_output=True,
                       text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    names = ["RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png"]
    for n in names:
        assert (tmp_path / n).exists(), n
    P = rt_amd.parse_obj(obj)
    sky = rt_amd.read_image_float(str(hdr))
    fb = rt_amd.Image(16, 12)
    rk = rt_amd.RenderKernel(16, 12, 1, 2, fb, P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), sky, None, hostsim=True)
    rk.set_camera(rt_amd.Camera.preset("cornell"))
    rk.render()
    rt_amd.write_image_png(fb, str(tmp_path / "want.png"))
    assert (tmp_path / "want.png").read_bytes() == (tmp_path / names[0]).read_bytes()
    rt_amd.write_image_png(rk.denoise(blend_factor=1.0), str(tmp_path / "want1.png"))
    assert (tmp_path / "want1.png").read_bytes() == (tmp_path / names[1]).read_bytes()


# ---------------------------------------------------------------------- GPU
# Which kernel a shape reaches. The product's dispatch (dn_variant 0) takes the LDS-halo
# kernel at steps 1 and 2 and the direct kernel from step 4 on, so with every shape below
# passes >= 1 reaches k_dn_lds<64, 4, 1>, passes >= 2 k_dn_lds<64, 4, 2> and passes >= 3
# k_dn_direct (257x9: two tiles across, the second one pixel wide; three tile rows, the last
# one row high; height below the reach of steps 4..16). dn_variant 1 (rt_test_schedule) runs
# the direct kernel at steps 1 and 2 as well, and dn_variant 2 adds k_dn_lds<32, 8, 4> at
# step 4 (passes >= 3): the measured alternatives of each step, which the dispatch does not
# select, held to the same bits.
GPU_SIZES = SIZES + [(257, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("guides", [True, False])
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_gpu_filter_equals_hostsim(w, h, guides, variant):
    rgba, alb, nd = synth(w, h)
    with forced_variant(ctx, "dn_variant", variant):
        for passes in (1, 2, 3, 4, 5):
            for blend in (0.0, 0.75, 1.0):
                want = host_result(w, h, passes, guides, blend)
                got = denoise(rgba, alb if guides else None, nd if guides else None, params(passes), blend,
                              hostsim=False)
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32),
                                              err_msg=f"passes {passes} blend {blend}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_gpu_nan_guide_equals_hostsim(variant):
    rgba, alb, nd = synth(37, 29)
    nd[10, 12, 0] = np.nan
    want = denoise(rgba, alb, nd, params(3), 1.0)
    with forced_variant(ctx, "dn_variant", variant):
        got = denoise(rgba, alb, nd, params(3), 1.0, hostsim=False)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


class device_array:
    """A float32 array in device memory: .ptr is the device pointer, .get() copies it back.
    A plain HIP allocation through hip_mem, as in every device-pointer test of the project:
    the test process then holds one HIP runtime, the one librt_hip.so links, while torch
    would bring a second copy of its own into it. A tensor's data_ptr() is the same kind of
    pointer; the stream argument is covered with the default stream only."""

    def __init__(self, a: np.ndarray):
        from hip_mem import DeviceBuffer
        self.shape = a.shape
        self.buf = DeviceBuffer(a.nbytes)
        self.buf.upload(a)
        self.ptr = self.buf.ptr

    def get(self) -> np.ndarray:
        return self.buf.download(self.shape, np.float32)


@pytest.mark.gpu
def test_gpu_denoise_device_pointers_and_scratch_reuse():
    L, h = ctx(False)
    for (w, hh) in [(130, 67), (37, 29)]:  # larger, then smaller: the context's scratch is reused
        rgba, alb, nd = synth(w, hh)
        want = denoise(rgba, alb, nd, params(4), 0.75, hostsim=False)
        t_in, t_alb, t_nd, t_out = (device_array(a) for a in (rgba, alb, nd, np.zeros_like(rgba)))
        p = params(4)
        rt_amd.check(L, L.rt_denoise_device(h, w, hh, t_in.ptr, t_alb.ptr, t_nd.ptr, ctypes.byref(p),
                                            ctypes.c_float(0.75), t_out.ptr, None), h, "rt_denoise_device")
        np.testing.assert_array_equal(t_out.get().view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(t_in.get().view(np.uint32), rgba.view(np.uint32))
        np.testing.assert_array_equal(want.view(np.uint32), host_result(w, hh, 4, True, 0.75).view(np.uint32))


@pytest.mark.gpu
def test_gpu_render_features_denoise_chain_equals_hostsim(cameras, manifest):
    outs = []
    for hostsim in (True, False):
        rk, fb = _cornell_kernel(cameras, manifest, hostsim, 64, 64, 4, 3)
        rk.render()
        outs.append((fb.pixels.copy(), rk.denoise(blend_factor=0.75).pixels))
    np.testing.assert_array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    np.testing.assert_array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
