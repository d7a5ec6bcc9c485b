"""The bloom stage on the hostsim build (rt_bloom; include/rt_hip.h): against bloom_cases.model(), a float64 restatement
of rt_bloom.h's header comment; the exact properties; the argument errors; the command line's --bloom."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import bloom_cases as bc
import noise_cases as nc
import rt_amd
import scenes
from bloom_cases import bloom, inputs, params
from rt_amd import cli, ptr

f32 = np.float32


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("levels", bc.LEVELS)
@pytest.mark.parametrize("w,h", bc.SHAPES)
def test_hostsim_matches_float64_model(w, h, levels):
    """The largest error over the 15 cases is 4.82e-7 (263x41, levels 8); every pixel is compared."""
    rgba = inputs(w, h)
    p = params(levels=levels)
    got = bloom(rgba, p)
    want = bc.model(rgba, p)
    e_out, e_layer = bc.model_error(got[0], want[0]), bc.model_error(got[1], want[1])
    print(f"bloom model {w}x{h} levels {levels}: rgba_out {e_out:.3e} layer_out {e_layer:.3e}")
    assert e_out <= bc.MODEL_TOL and e_layer <= bc.MODEL_TOL
    if w >= 37:
        lum = bc.luminance(rgba[..., :3])
        dim = np.isfinite(lum) & (lum < 1.0)
        assert (got[0][..., :3][dim] > rgba[..., :3][dim]).any(), "a pixel below the threshold got brighter"


# ------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("levels", bc.LEVELS)
@pytest.mark.parametrize("w,h", bc.SHAPES)
def test_nothing_above_the_threshold_or_intensity_zero_returns_the_input(w, h, levels):
    rgba = inputs(w, h)
    keep = rgba.copy()
    # the gradient stays below 1.0 in luminance: a threshold of 1e39 is not a float, so take one above every planted pixel
    quiet = np.where(np.isfinite(rgba) & (np.abs(rgba) < 10), rgba, f32(0.25)).astype(f32)
    quiet[..., :3] = np.minimum(quiet[..., :3], f32(0.45))  # luminance <= 0.45 < threshold - knee = 0.5
    for frame, p in ((quiet, params(levels=levels)), (rgba, params(intensity=0.0, levels=levels))):
        before = frame.copy()
        out, layer = bloom(frame, p)
        fin = ~bc.bad_pixels(frame)
        assert np.array_equal(out[..., :3][fin], frame[..., :3][fin]), "the input as values"
        nc.assert_bits(out[~fin], frame[~fin], "a bad centre is copied bit for bit")
        nc.assert_bits(out[..., 3], frame[..., 3], "alpha comes back bit for bit")
        assert np.all(layer == 0.0), "nothing was added"
        nc.assert_bits(frame, before, "the input changed")
    nc.assert_bits(rgba, keep, "the input changed")


@pytest.mark.parametrize("levels", bc.LEVELS)
@pytest.mark.parametrize("w,h", [(5, 3), (37, 29), (130, 67)])
def test_uniform_frame_gives_a_uniform_layer(w, h, levels):
    """The weights of the reduce sum to 1 at every level and so do the expand's: a uniform b stays b on every level,
    u_1 is levels * b and the layer is scale * levels * b."""
    rgba = np.empty((h, w, 4), f32)
    rgba[...] = (3.0, 2.0, 1.5, 0.25)
    p = params(levels=levels)
    out, layer = bloom(rgba, p)
    b = bc.bright_pass(rgba[:1, :1], p)[0, 0]
    want = float(f32(p.intensity) / f32(levels)) * levels * b
    assert b.min() > 0.5
    err = np.abs(layer[..., :3].astype(np.float64) - want) / np.maximum(1.0, want)
    assert err.max() <= bc.MODEL_TOL, err.max()
    assert np.all(layer[..., 3] == 0.0)
    assert np.ptp(layer[..., 0]) <= bc.MODEL_TOL * want[0], "uniform"


@pytest.mark.parametrize("w,h", [(5, 3), (37, 29)])
def test_a_bad_colour_stays_where_it_is(w, h):
    rgba = inputs(w, h)
    clean = rgba.copy()
    bad = bc.bad_pixels(rgba)
    assert bad.any()
    clean[bad] = (0.3, 0.3, 0.3, 1.0)  # (below threshold - knee: b = 0, as a bad pixel's)
    p = params(levels=3)
    out, layer = bloom(rgba, p)
    ref, ref_layer = bloom(clean, p)
    nc.assert_bits(out[bad], rgba[bad], "a bad centre is copied bit for bit")
    assert np.isfinite(out[~bad]).all() and np.isfinite(layer).all(), "no other pixel's finiteness changed"
    nc.assert_bits(out[~bad], ref[~bad], "the others are what they are without the bad colours")
    nc.assert_bits(layer, ref_layer, "the layer does not see the bad colours")


@pytest.mark.parametrize("levels", bc.LEVELS)
@pytest.mark.parametrize("w,h", bc.SHAPES)
def test_layer_is_what_was_added(w, h, levels):
    rgba = inputs(w, h)
    out, layer = bc.host_result(w, h, levels)
    fin = ~bc.bad_pixels(rgba)
    with np.errstate(all="ignore"):  # (the bad centres: left out below)
        diff = out[..., :3].astype(np.float64) - rgba[..., :3].astype(np.float64)
    scale = np.maximum(1.0, np.abs(out[..., :3].astype(np.float64)))
    # (rgba_out is the rounded sum: half an ulp of it, well inside the model's tolerance)
    assert (np.abs(diff - layer[..., :3])[fin] / scale[fin]).max() <= bc.MODEL_TOL
    assert np.all(layer[..., 3] == 0.0), "the layer's alpha is 0"
    no_layer = bloom(rgba, params(levels=levels), layer=False)
    assert no_layer[1] is None
    nc.assert_bits(no_layer[0], out, "layer_out NULL: rgba_out")


def test_null_params_are_the_defaults():
    rgba = inputs(37, 29)
    d = rt_amd.bloom_default_params(hostsim=True)
    assert (d.threshold, d.knee, d.intensity, d.levels) == (1.0, 0.5, f32(0.2), 5)
    for a, b in zip(bloom(rgba, None), bloom(rgba, d)):
        nc.assert_bits(a, b, "params NULL: the defaults")


def test_argument_errors():
    rgba = inputs(5, 3)
    L, h = bc.ctx(True)
    ARG = rt_amd.RT_ERR_ARG

    def rc(p=None, **over):
        r = bloom(rgba, p if p is not None else params(), code=True, **over)
        assert r == 0 or L.rt_last_error(h).startswith(b"rt_bloom:"), L.rt_last_error(h)
        return r

    assert rc() == 0
    for v in (0, 9, -1):
        assert rc(params(levels=v)) == ARG and b"levels" in L.rt_last_error(h)
    assert rc(params(levels=1)) == 0 and rc(params(levels=8)) == 0
    for name in ("threshold", "knee", "intensity"):
        for v in (-0.5, np.nan, np.inf, -np.inf):
            assert rc(params(**{name: v})) == ARG and name.encode() in L.rt_last_error(h), (name, v)
    assert rc(params(threshold=0.5, knee=0.75)) == ARG and b"knee is above threshold" in L.rt_last_error(h)
    assert rc(params(threshold=0.5, knee=0.5)) == 0 and rc(params(threshold=0.0, knee=0.0)) == 0 and rc(params(knee=0.0)) == 0
    for kw in (dict(w=0), dict(h=0), dict(w=-3)):
        assert rc(**kw) == ARG and b"at least 1" in L.rt_last_error(h)
    assert rc(rgba_in=None) == ARG and b"NULL" in L.rt_last_error(h)
    assert rc(out=None) == ARG and b"NULL" in L.rt_last_error(h)
    # an output that aliases the input or the other output, by pointer and by overlap
    assert rc(out=rgba) == ARG and b"overlaps an input" in L.rt_last_error(h)
    assert rc(layer_out=rgba) == ARG and b"overlaps an input" in L.rt_last_error(h)
    big = np.zeros(16 * 15 + 16, np.uint8)
    assert rc(rgba_in=big[:240].view(f32).reshape(3, 5, 4), out=big[16:256].view(f32).reshape(3, 5, 4)) == ARG
    both = np.zeros((3, 5, 4), f32)
    assert rc(out=both, layer_out=both) == ARG and b"two outputs overlap" in L.rt_last_error(h)
    assert rc(out=big[:240].view(f32).reshape(3, 5, 4), layer_out=big[16:256].view(f32).reshape(3, 5, 4)) == ARG
    assert b"two outputs overlap" in L.rt_last_error(h)
    # rt_denoise's frame-size limits
    tall = np.zeros((262141, 1, 4), f32)
    p = params()
    assert L.rt_bloom(h, 1, 262141, ptr(tall), ctypes.byref(p), ptr(tall.copy()), None) == ARG
    assert b"262140" in L.rt_last_error(h)
    assert L.rt_bloom(h, 1 << 14, 1 << 13, ptr(tall), ctypes.byref(p), ptr(tall.copy()), None) == ARG
    assert b"rt_bloom: too many pixels" in L.rt_last_error(h)
    # the device form's alignment rule
    odd = np.zeros(16 * 15 + 16, np.uint8)[4:]
    o4, l4 = np.zeros((3, 5, 4), f32), np.zeros((3, 5, 4), f32)

    def dev(i=rgba, o=o4, lo=l4):
        return L.rt_bloom_device(h, 5, 3, ptr(i), ctypes.byref(p), ptr(o), ptr(lo), None)

    assert dev() == 0, L.rt_last_error(h)
    for kw in (dict(i=odd), dict(o=odd), dict(lo=odd)):
        assert dev(**kw) == ARG and b"aligned" in L.rt_last_error(h), kw
        assert L.rt_last_error(h).startswith(b"rt_bloom_device:")
    assert L.rt_bloom(None, 5, 3, ptr(rgba), None, ptr(o4), None) == ARG
    for v in (2.0, 7.0, -3.0, 0.0):  # (clamped to 0..2, as ff_variant is)
        assert L.rt_test_schedule(h, b"bloom_variant", v) == 0


def _small_kernel(sky):
    """Cornell 12-tri at 16 x 12 on the hostsim build, 4 samples, 2 bounces, under the Cornell camera."""
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    fb = rt_amd.Image(16, 12)
    rk = rt_amd.RenderKernel(16, 12, 4, 2, fb, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices, None,
                             rt_amd.BVH(P.triangles), sky, rt_amd.compute_env_map_cdf(sky), hostsim=True)
    rk.set_camera(rt_amd.Camera.preset("cornell"))
    return rk, fb


def test_python_layer():
    rgba = inputs(37, 29)
    rk, _ = _small_kernel(rt_amd.Image.from_rgb(scenes.make_sky("S")))  # (the stage takes a frame of any size)
    img = rt_amd.Image(37, 29, pixels=rgba)
    out, layer = rk.bloom(img, levels=3, return_layer=True)
    want = bc.host_result(37, 29, 3)
    nc.assert_bits(out.pixels, want[0], "RenderKernel.bloom: the frame")
    nc.assert_bits(layer, want[1], "RenderKernel.bloom: the layer")
    nc.assert_bits(rk.bloom(img, threshold=1.0, knee=0.5, intensity=0.2, levels=3).pixels, want[0], "every keyword")
    assert not np.array_equal(rk.bloom(img, intensity=0.4, levels=3).pixels, want[0])
    with pytest.raises(rt_amd.RtError):
        rk.bloom(img, knee=2.0)


# ------------------------------------------------------------------ the command line
def _cli(tmp_path, out, *flags):
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    return cli.main([scenes.scene_path("cornell12"), f"--sky={hdr}", "--w=16", "--h=12", "--samples=4", "--bounces=2",
                     "--hostsim", "--camera=cornell", f"--out={out}", *flags])


PNGS = ("RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png")


def test_cli_bloom(tmp_path, capsys):
    for bad in ("--bloom=-1", "--bloom=inf", "--bloom=nan"):
        assert _cli(tmp_path, tmp_path / "bad", bad) == 2
        assert "--bloom=INTENSITY" in capsys.readouterr().err
    # without the flag: the tone-mapped render's path, and the display stage's path at the reference's parameters,
    # which bloom's path shares; they write the same bytes, and neither prints the line
    assert _cli(tmp_path, tmp_path / "plain") == 0
    assert "bloom:" not in capsys.readouterr().out
    assert _cli(tmp_path, tmp_path / "linear", "--exposure=1.5", "--gamma=2.2") == 0
    assert "bloom:" not in capsys.readouterr().out
    for name in PNGS:
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "linear" / name).read_bytes(), name
    # the frame the run renders
    rk, fb = _small_kernel(rt_amd.read_image_float(str(tmp_path / "sky.hdr")))
    rk.render_linear()
    c = fb.pixels
    above = int(((f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2] > f32(1.0)).sum())
    assert 0 < above < 16 * 12, "the small Cornell frame shows its light"
    for flag, kw in (("--bloom", {}), ("--bloom=0.6", dict(intensity=0.6))):
        out = tmp_path / flag.strip("-").replace("=", "_")
        assert _cli(tmp_path, out, flag, f"--hdr-out={out}.hdr") == 0
        assert f"bloom: 5 levels, {above} of 192 pixels above threshold" in capsys.readouterr().out
        rt_amd.write_image_png(rk.display(rk.bloom(fb, **kw), exposure=1.5, gamma=2.2), str(tmp_path / "want.png"))
        assert (out / "RT_output.png").read_bytes() == (tmp_path / "want.png").read_bytes()
        assert (out / "RT_output.png").read_bytes() != (tmp_path / "plain" / "RT_output.png").read_bytes()
        rt_amd.write_image_hdr(fb, str(tmp_path / "want.hdr"))
        assert open(f"{out}.hdr", "rb").read() == (tmp_path / "want.hdr").read_bytes(), "--hdr-out stays the frame before bloom"
    # an intensity of 0 adds nothing: the bytes of a run without the flag
    assert _cli(tmp_path, tmp_path / "zero", "--bloom=0") == 0
    assert "bloom: 5 levels" in capsys.readouterr().out
    for name in PNGS:
        assert (tmp_path / "zero" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    # the exposure is metered on the frame before bloom
    assert _cli(tmp_path, tmp_path / "auto", "--bloom", "--auto-exposure") == 0
    text = capsys.readouterr().out
    e = rk.auto_exposure(fb)
    assert f"auto-exposure: {e:.9g}" in text and text.index("auto-exposure:") < text.index("bloom:")
    rt_amd.write_image_png(rk.display(rk.bloom(fb), exposure=e, gamma=2.2), str(tmp_path / "want.png"))
    assert (tmp_path / "auto" / "RT_output.png").read_bytes() == (tmp_path / "want.png").read_bytes()
