"""Linear radiance and the display stage on the hostsim build: the cases of tests/display_cases.py, the
Radiance writer (host code, the same in both builds) and the command line. The GPU half
(tests/test_display_gpu.py) holds k_display and k_resolve_linear to this build bit for bit."""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import display_cases as dc
import progress_cases as pc

import rt_amd
from rt_amd import _capi
from rt_amd._capi import RT_ERR_ARG, RT_ERR_IO, RT_OK


@pytest.mark.parametrize("base", ["blank", "random"])
@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_round_trip(scene, base):
    dc.case_round_trip(True, scene, base)


@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_linear_frame_pinned_by_checkpoint(scene):
    dc.case_linear_pinned(True, scene)


def test_linear_resolve_is_pure():
    dc.case_resolve_pure(True)


@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_split_invariance(scene):
    dc.case_split(True, scene)


def test_row_shard():
    dc.case_shard(True)


def test_two_shards():
    dc.case_multi(True)


@pytest.mark.parametrize("gamma", dc.GAMMAS)
@pytest.mark.parametrize("exposure", dc.EXPOSURES)
def test_display_against_model(exposure, gamma):
    dc.case_model(True, exposure, gamma)


def test_edge_values():
    dc.case_edges(True)


@pytest.mark.parametrize("gamma", dc.GAMMAS + (1.8,))
@pytest.mark.parametrize("exposure", dc.EXPOSURES)
@pytest.mark.parametrize("buffer", ["model", "edge"])
def test_display_against_glibc(buffer, exposure, gamma):
    """rt_display's rgb is display_pixel's operations in numpy float32, in its order, with glibc's expf and powf
    (through ctypes) where it calls rt_libm's, and 1 / gamma the float division rt_display forms: bit for bit, NaN
    matching NaN. The gfx950 kernel is held to this build bitwise (tests/test_display_gpu.py), so the display stage
    is chained to glibc at caller-chosen parameters."""
    import libm_cases as lc
    m = lc.glibc()
    lin = dc.model_buffer() if buffer == "model" else dc.edge_buffer()
    s = dc.unbound(True)
    got, _ = dc.display(s, lin, exposure, gamma, want=("rgba",))
    s.close()
    e = np.float32(exposure)
    inv_gamma = float(np.float32(1.0) / np.float32(gamma))
    with np.errstate(all="ignore"):
        arg = (-lin[..., :3]) * e
        ex = np.array([m.expf(float(v)) for v in arg.ravel()], np.float32).reshape(arg.shape)
        tm = np.float32(1.0) + (-ex)
        want = np.array([m.powf(float(v), inv_gamma) for v in tm.ravel()], np.float32).reshape(tm.shape)
    assert np.array_equal(lc.np_canon(got[..., :3]), lc.np_canon(want)), f"{buffer} e={exposure} g={gamma}: rgb vs glibc"
    dc.assert_bits(got[..., 3], dc.model_alpha(lin, exposure), "alpha vs numpy float32")


@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgba8_and_shapes(shape):
    dc.case_shape(True, *shape)


def test_errors():
    dc.case_errors(True)


def test_default_params():
    p = _capi.DisplayParams(9.0, 9.0, 9)
    _capi.lib(True).rt_display_default_params(ctypes.byref(p))
    assert (p.exposure, p.gamma, p.flip_y) == (1.5, np.float32(2.2), 0)
    _capi.lib(True).rt_display_default_params(None)


def test_python_render_kernel():
    dc.case_python(True)


# ------------------------------------------------------------------ rt_write_hdr
def _img(a) -> rt_amd.Image:
    a = np.ascontiguousarray(a, np.float32)
    return rt_amd.Image(a.shape[1], a.shape[0], pixels=a)


def _exact_image(w: int, h: int) -> np.ndarray:
    """Channels m * 2^k with integer m < 256 against the largest channel's exponent: the largest channel's
    mantissa is 128..255 at exponent e, the others are integers of 2^(e - 136)'s grid below it."""
    rng = np.random.default_rng([208, w, h])
    e = rng.integers(-20, 20, (h, w, 1))
    m = rng.integers(0, 256, (h, w, 3))
    m[np.arange(h)[:, None], np.arange(w)[None, :], rng.integers(0, 3, (h, w))] = rng.integers(128, 256, (h, w))
    a = np.zeros((h, w, 4), np.float32)
    a[..., :3] = np.ldexp(m.astype(np.float64), e - 8)
    a[..., 3] = 0.75  # (dropped)
    a[0, 0, :3] = (1.0, 0.5, 0.25)
    return a


@pytest.mark.parametrize("w", [1, 7, 8, 40])
def test_write_hdr_round_trip(tmp_path, w):
    h = 5
    path = str(tmp_path / "a.hdr")
    a = _exact_image(w, h)
    assert rt_amd.write_image_hdr(_img(a), path, flipY=False)
    raw = open(path, "rb").read()
    head = f"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y {h} +X {w}\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + 4 * w * h
    assert raw[len(head):len(head) + 4] == bytes([128, 64, 32, 129]), "(1, 0.5, 0.25)"
    back = rt_amd.read_image_float(path, flipY=False)
    assert (back.width, back.height) == (w, h)
    assert np.array_equal(back.pixels[..., :3].view(np.uint32), a[..., :3].view(np.uint32)), "m * 2^k reads back exactly"
    assert (back.pixels[..., 3] == 0).all()

    # a random image: every channel within 2^(e - 8), e the frexp exponent of the pixel's largest channel
    rng = np.random.default_rng([209, w])
    r = np.zeros((h, w, 4), np.float32)
    r[..., :3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(16.0)
    r[1, 0, :3] = (1e-33, 5e-33, 0.0)   # below 1e-32: zeros
    r[2, 0, :3] = (0.0, 0.0, 0.0)
    path_r = str(tmp_path / "r.hdr")
    assert rt_amd.write_image_hdr(_img(r), path_r, flipY=False)
    got = rt_amd.read_image_float(path_r, flipY=False).pixels[..., :3]
    e = np.frexp(r[..., :3].max(axis=2).astype(np.float64))[1]
    bound = np.ldexp(1.0, e - 8)[..., None]
    d = r[..., :3].astype(np.float64) - got.astype(np.float64)
    held = r[..., :3].max(axis=2) >= np.float32(1e-32)
    assert (d >= 0).all() and (d[held] < bound[held]).all(), "truncation: 0 <= written - read < 2^(e - 8)"
    assert (got[1, 0] == 0).all() and (got[2, 0] == 0).all(), "pixels below 1e-32 come back as zeros"

    # writing what was read back reproduces the file
    again = str(tmp_path / "again.hdr")
    back_r = rt_amd.read_image_float(path_r, flipY=False)
    assert rt_amd.write_image_hdr(back_r, again, flipY=False)
    assert open(again, "rb").read() == open(path_r, "rb").read()

    # flip_y on write and on read cancel; one flip reverses the rows
    fl = str(tmp_path / "flip.hdr")
    assert rt_amd.write_image_hdr(_img(a), fl)  # (flipY defaults to True, as the reference's)
    assert np.array_equal(rt_amd.read_image_float(fl).pixels[..., :3], a[..., :3])
    assert np.array_equal(rt_amd.read_image_float(fl, flipY=False).pixels[..., :3], a[::-1, :, :3])


def test_write_hdr_errors(tmp_path):
    L = _capi.lib(True)
    a = _exact_image(4, 2)
    ok = str(tmp_path / "x.hdr").encode()
    assert L.rt_write_hdr(str(tmp_path / "no" / "such" / "dir.hdr").encode(), _capi.ptr(a), 4, 2, 0) == RT_ERR_IO
    assert b"rt_write_hdr" in L.rt_last_error(None)
    for args in ((None, _capi.ptr(a), 4, 2, 0), (ok, None, 4, 2, 0), (ok, _capi.ptr(a), 0, 2, 0), (ok, _capi.ptr(a), 4, -1, 0)):
        assert L.rt_write_hdr(*args) == RT_ERR_ARG
    assert L.rt_write_hdr(ok, _capi.ptr(a), 4, 2, 1) == RT_OK
    # what the format cannot hold is written as its nearest value, not as garbage
    b = np.zeros((1, 3, 4), np.float32)
    b[0, 0, :3] = (-1.0, 2.0, np.nan)
    b[0, 1, :3] = (np.inf, 1.0, 0.0)
    b[0, 2, :3] = (np.nan, np.nan, -np.inf)
    assert L.rt_write_hdr(ok, _capi.ptr(b), 3, 1, 0) == RT_OK
    got = rt_amd.read_image_float(ok.decode(), flipY=False).pixels[0, :, :3]
    assert np.array_equal(got[0], [0.0, 2.0, 0.0]) and (got[2] == 0).all()
    assert got[1, 0] == np.float32(255 * 2.0 ** 119) and got[1, 1] == 0.0, "+inf: the format's largest value"


# ------------------------------------------------------------------ the command line
def test_cli_display_flags(tmp_path):
    """--exposure=1.5 --gamma=2.2 writes the four PNGs of a run without flags, byte for byte; --exposure=0.5
    changes RT_output.png; --hdr-out reads back to render_linear's frame within the format's truncation;
    previews go through the display stage with the same parameters."""
    import scenes

    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(rt_amd.__file__)))
    names = ["RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png"]
    w, h, spp, nb = 16, 12, 2, 2

    def run(out, *flags):
        r = subprocess.run([sys.executable, "-m", "rt_amd.cli", scenes.scene_path("cornell12"), f"--sky={hdr}", f"--w={w}",
                            f"--h={h}", f"--samples={spp}", f"--bounces={nb}", "--hostsim", "--camera=cornell",
                            f"--out={out}", *flags], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr

    plain, same, dark, prog = (tmp_path / n for n in ("plain", "same", "dark", "prog"))
    lin_path = tmp_path / "linear.hdr"
    run(plain)
    run(same, "--exposure=1.5", "--gamma=2.2", f"--hdr-out={lin_path}")
    run(dark, "--exposure=0.5")
    run(prog, "--gamma=2.2", "--preview-every=1")
    for n in names:
        assert (same / n).read_bytes() == (plain / n).read_bytes(), n
        assert (prog / n).read_bytes() == (plain / n).read_bytes(), n
    assert (dark / names[0]).read_bytes() != (plain / names[0]).read_bytes()
    assert (prog / f"RT_preview_{spp}.png").read_bytes() == (plain / names[0]).read_bytes()
    assert not list(plain.glob("*.hdr"))

    # the .hdr file against render_linear of the same frame
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    sky = rt_amd.read_image_float(str(hdr))
    fb = rt_amd.Image(w, h)
    rk = rt_amd.RenderKernel(w, h, spp, nb, fb, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices,
                             None, rt_amd.BVH(P.triangles), sky, rt_amd.compute_env_map_cdf(sky), hostsim=True)
    rk.set_camera(rt_amd.Camera.preset("cornell"))
    rk.render_linear()
    got = rt_amd.read_image_float(str(lin_path)).pixels[..., :3].astype(np.float64)
    want = fb.pixels[..., :3].astype(np.float64)
    assert (want >= 0).all() and want.max() > 0
    e = np.frexp(want.max(axis=2))[1]
    d = want - got
    assert (d >= 0).all() and (d < np.ldexp(1.0, e - 8)[..., None]).all()
