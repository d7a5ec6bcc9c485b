"""The depth-of-field stage on the hostsim build (rt_dof; include/rt_hip.h): against dof_cases.model(), a restatement
of rt_dof.h's header comment with float64 sums; the exact properties; the argument errors; rt_amd.focus_at; the command
line's --dof."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import dof_cases as dc
import noise_cases as nc
import rt_amd
import scenes
from dof_cases import dof, inputs, params
from rt_amd import cli, ptr

f32 = np.float32


def _flat(w, h, colour=(0.4, 0.3, 0.2, 0.7), t=dc.FOCUS):
    rgba = np.empty((h, w, 4), f32)
    rgba[...] = colour
    nd = np.zeros((h, w, 4), f32)
    nd[..., 3] = t
    return rgba, nd


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("max_radius", dc.RADII)
@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_hostsim_matches_float64_model(w, h, max_radius):
    """The largest error over the 15 cases is 1.526e-6 (130x67, max_radius 12); every pixel is compared."""
    rgba, nd = inputs(w, h)
    keep = rgba.copy(), nd.copy()
    p = params(max_radius=max_radius)
    out, coc = dof(rgba, nd, p)
    want, r = dc.model(rgba, nd, p)
    e = dc.model_error(out, want)
    print(f"dof model {w}x{h} max_radius {max_radius}: rgba_out {e:.3e}")
    nc.assert_bits(coc, r, "coc_out is the float32 radius")
    nc.assert_bits(out[..., 3], rgba[..., 3], "alpha comes back bit for bit")
    bad = dc.bad_pixels(rgba)
    nc.assert_bits(out[bad], rgba[bad], "a bad centre is copied bit for bit")
    nc.assert_bits(rgba, keep[0], "the input changed")
    nc.assert_bits(nd, keep[1], "the guide changed")
    assert e <= dc.MODEL_TOL
    nc.assert_bits(dof(rgba, nd, p, coc=False)[0], out, "coc_out NULL: rgba_out")


# ------------------------------------------------------------------ properties
@pytest.mark.parametrize("max_radius", dc.RADII)
@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_no_lens_or_everything_in_focus_returns_the_input(w, h, max_radius):
    rgba, nd = inputs(w, h)
    focused = nd.copy()
    focused[..., 3] = dc.FOCUS
    for guide, p in ((nd, params(coc_inf=0.0, max_radius=max_radius)), (focused, params(max_radius=max_radius))):
        out, coc = dof(rgba, guide, p)
        fin = ~dc.bad_pixels(rgba)
        assert np.array_equal(out[..., :3][fin], rgba[..., :3][fin]), "the input as values: one tap of weight 2, 2c / 2"
        nc.assert_bits(out[~fin], rgba[~fin], "a bad centre is copied bit for bit")
        nc.assert_bits(out[..., 3], rgba[..., 3], "alpha comes back bit for bit")
        assert np.all(coc == 0.0)


@pytest.mark.parametrize("max_radius", dc.RADII)
def test_uniform_colour_over_any_depth_stays_uniform(max_radius):
    rgba, nd = inputs(37, 29)
    rgba[...] = (3.0, 2.0, 1.5, 0.25)
    out, _ = dof(rgba, nd, params(max_radius=max_radius))
    err = np.abs(out.astype(np.float64) - rgba) / np.maximum(1.0, rgba)
    assert err.max() <= dc.MODEL_TOL, err.max()


def test_one_bright_pixel_becomes_a_disc():
    """Uniform r = 4 (t = 2 focus, coc_inf 4): a is 1 for D <= 3.5 and 0 for D >= 4.5, k is the same for every tap and
    so is W for every pixel whose window is inside the image: a flat interior, nothing beyond."""
    rgba, nd = _flat(41, 41, colour=(0.0, 0.0, 0.0, 1.0), t=2 * dc.FOCUS)
    rgba[20, 20, :3] = (100.0, 50.0, 25.0)
    out, coc = dof(rgba, nd, params(coc_inf=8.0, max_radius=8))  # r = 8 * |4 - 2| / 4
    assert np.all(coc == 4.0)
    yy, xx = np.mgrid[0:41, 0:41]
    D = np.sqrt((xx - 20.0) ** 2 + (yy - 20.0) ** 2)
    inner, outer = D <= 3.5, D >= 4.5
    assert np.all(out[..., :3][outer] == 0.0), "nothing beyond D >= 4.5"
    assert np.ptp(out[..., 0][inner]) <= dc.MODEL_TOL * out[20, 20, 0] and out[20, 20, 0] > 0, "a flat interior"
    ring = ~inner & ~outer
    assert np.all(out[..., 0][ring] < out[20, 20, 0]) and np.all(out[..., 0][ring] > 0), "one pixel of soft edge"


def test_sharp_foreground_stays_sharp_and_blurred_foreground_bleeds():
    rgba, nd = inputs(37, 29)
    rgba[...] = np.where(np.isfinite(rgba), rgba, f32(0.5))
    # an in-focus foreground pixel, every neighbour farther and blurred
    nd[..., 3] = 4 * dc.FOCUS
    nd[14, 18, 3] = dc.FOCUS
    out, coc = dof(rgba, nd, params(max_radius=8))
    assert coc[14, 18] == 0.0 and coc[14, 19] == f32(7.5)
    assert np.array_equal(out[14, 18], rgba[14, 18]), "an in-focus foreground pixel comes back exactly"
    assert not np.array_equal(out[14, 19, :3], rgba[14, 19, :3])
    # a defocused foreground block over an in-focus background
    rgba[..., :3] = 0.0
    rgba[10:20, 10:20, :3] = 5.0
    nd[..., 3] = dc.FOCUS
    nd[10:20, 10:20, 3] = dc.FOCUS / 2  # r = min(10 * 1 / 1, 8) = 8
    out, coc = dof(rgba, nd, params(max_radius=8))
    assert coc[15, 25] == 0.0 and coc[15, 15] == 8.0
    assert np.all(out[15, 20:27, 0] > 0), "the foreground bleeds onto in-focus background within its radius"
    assert np.all(out[15, 29:, 0] == 0) and np.all(out[:, :1, 0] == 0), "and no further"


@pytest.mark.parametrize("w,h", [(5, 3), (37, 29)])
def test_a_bad_colour_stays_where_it_is(w, h):
    rgba, nd = inputs(w, h)
    bad = dc.bad_pixels(rgba)
    assert bad.any()
    p = params(max_radius=4)
    out, coc = dof(rgba, nd, p)
    nc.assert_bits(out[bad], rgba[bad], "a bad centre is copied bit for bit")
    assert np.isfinite(out[~bad]).all(), "no other pixel's finiteness changed"
    # what the others are with the bad pixel cut out of every window: the model says so, and so does a second call
    # whose bad pixel has another (bad) colour
    other = rgba.copy()
    other[bad] = (np.inf, 1.0, -np.inf, 0.5)
    out2, coc2 = dof(other, nd, p)
    nc.assert_bits(out2[~bad], out[~bad], "the others do not see the bad colour")
    nc.assert_bits(coc2, coc, "nor does the radius")


def test_null_params_are_the_defaults():
    rgba, nd = inputs(37, 29)
    d = rt_amd.dof_default_params(hostsim=True)
    assert (d.focus, d.coc_inf, d.max_radius) == (1.0, 4.0, 8)
    for a, b in zip(dof(rgba, nd, None), dof(rgba, nd, d)):
        nc.assert_bits(a, b, "params NULL: the defaults")


def test_argument_errors():
    rgba, nd = inputs(5, 3)
    L, h = dc.ctx(True)
    ARG = rt_amd.RT_ERR_ARG

    def rc(p=None, **over):
        r = dof(rgba, nd, p if p is not None else params(), code=True, **over)
        assert r == 0 or L.rt_last_error(h).startswith(b"rt_dof:"), L.rt_last_error(h)
        return r

    assert rc() == 0
    for v in (0, 13, -1):
        assert rc(params(max_radius=v)) == ARG and b"max_radius" in L.rt_last_error(h)
    assert rc(params(max_radius=1)) == 0 and rc(params(max_radius=12)) == 0
    for v in (0.0, -0.5, np.nan, np.inf, -np.inf):
        assert rc(params(focus=v)) == ARG and b"focus" in L.rt_last_error(h), v
    for v in (-0.5, np.nan, np.inf, -np.inf):
        assert rc(params(coc_inf=v)) == ARG and b"coc_inf" in L.rt_last_error(h), v
    assert rc(params(coc_inf=0.0)) == 0
    for kw in (dict(w=0), dict(h=0), dict(w=-3)):
        assert rc(**kw) == ARG and b"at least 1" in L.rt_last_error(h)
    for name in ("rgba_in", "nd_in", "out"):
        assert rc(**{name: None}) == ARG and b"NULL" in L.rt_last_error(h)
    assert rc(coc_out=None) == 0
    # an output that aliases an input or the other output, by pointer and by overlap
    assert rc(out=rgba) == ARG and b"overlaps an input" in L.rt_last_error(h)
    assert rc(out=nd) == ARG and b"overlaps an input" in L.rt_last_error(h)
    assert rc(coc_out=nd.reshape(-1)[:15].reshape(3, 5)) == ARG and b"overlaps an input" in L.rt_last_error(h)
    big = np.zeros(16 * 15 + 16, np.uint8)
    assert rc(rgba_in=big[:240].view(f32).reshape(3, 5, 4), out=big[16:256].view(f32).reshape(3, 5, 4)) == ARG
    both = np.zeros((3, 5, 4), f32)
    assert rc(out=both, coc_out=both.reshape(-1)[4:19].reshape(3, 5)) == ARG and b"two outputs overlap" in L.rt_last_error(h)
    # rt_denoise's frame-size limits
    tall = np.zeros((262141, 1, 4), f32)
    p = params()
    assert L.rt_dof(h, 1, 262141, ptr(tall), ptr(tall.copy()), ctypes.byref(p), ptr(tall.copy()), None) == ARG
    assert b"262140" in L.rt_last_error(h)
    assert L.rt_dof(h, 1 << 14, 1 << 13, ptr(tall), ptr(tall), ctypes.byref(p), ptr(tall.copy()), None) == ARG
    assert b"rt_dof: too many pixels" in L.rt_last_error(h)
    # the device form's alignment rule
    odd = np.zeros(16 * 15 + 16, np.uint8)[4:]
    odd1 = np.zeros(4 * 15 + 16, np.uint8)[1:]
    o4, c1 = np.zeros((3, 5, 4), f32), np.zeros((3, 5), f32)

    def dev(i=rgba, g=nd, o=o4, co=c1):
        return L.rt_dof_device(h, 5, 3, ptr(i), ptr(g), ctypes.byref(p), ptr(o), ptr(co), None)

    assert dev() == 0, L.rt_last_error(h)
    assert dev(co=odd) == 0, "coc_out needs 4-byte alignment only"
    for kw in (dict(i=odd), dict(g=odd), dict(o=odd), dict(co=odd1)):
        assert dev(**kw) == ARG and b"aligned" in L.rt_last_error(h), kw
        assert L.rt_last_error(h).startswith(b"rt_dof_device:")
    assert L.rt_dof(None, 5, 3, ptr(rgba), ptr(nd), None, ptr(o4), None) == ARG
    for v in (2.0, 7.0, -3.0, 0.0):  # (clamped to 0..2, as ff_variant is)
        assert L.rt_test_schedule(h, b"dof_variant", v) == 0
    assert L.rt_version() == 10002


def test_focus_at():
    _, nd = inputs(37, 29)
    assert rt_amd.focus_at(nd, 5, 20) == float(nd[20, 5, 3]), "a hit: its own t"
    # (3, h - 2) is a lone miss: the nearest hit of the 3 x 3 window about it
    win = nd[26:29, 2:5, 3]
    assert rt_amd.focus_at(nd, 3, 27) == float(win[win > 0].min())
    # inside the block of misses the window grows until it holds a hit
    t = rt_amd.focus_at(nd, 37 // 2 + 4, 2)
    assert t > 0 and t in nd[..., 3]
    nd[12, 28, 3] = np.nan
    assert rt_amd.focus_at(nd, 28, 12) > 0, "a NaN t is a miss"
    nd[..., 3] = -1.0
    with pytest.raises(ValueError):
        rt_amd.focus_at(nd, 3, 3)
    with pytest.raises(ValueError):
        rt_amd.focus_at(nd, 37, 3)


def _small_kernel(sky):
    """Cornell 12-tri at 16 x 12 on the hostsim build, 4 samples, 2 bounces, under the Cornell camera."""
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    fb = rt_amd.Image(16, 12)
    rk = rt_amd.RenderKernel(16, 12, 4, 2, fb, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices, None,
                             rt_amd.BVH(P.triangles), sky, rt_amd.compute_env_map_cdf(sky), hostsim=True)
    rk.set_camera(rt_amd.Camera.preset("cornell"))
    return rk, fb


def test_python_layer():
    rgba, nd = inputs(37, 29)
    rk, _ = _small_kernel(rt_amd.Image.from_rgb(scenes.make_sky("S")))  # (the stage takes a frame of any size)
    img = rt_amd.Image(37, 29, pixels=rgba)
    want = dc.host_result(37, 29, 4)
    out, coc = rk.dof(img, nd, params(max_radius=4), coc=True)
    nc.assert_bits(out.pixels, want[0], "RenderKernel.dof: the frame")
    nc.assert_bits(coc, want[1], "RenderKernel.dof: the radius")
    nc.assert_bits(rk.dof(img, nd, dict(focus=dc.FOCUS, coc_inf=dc.COC_INF, max_radius=4)).pixels, want[0], "a dict of fields")
    assert not np.array_equal(rk.dof(img, nd).pixels, want[0])
    with pytest.raises(rt_amd.RtError):
        rk.dof(img, nd, dict(max_radius=13))
    with pytest.raises(ValueError):
        rk.dof(img, nd[:5])


# ------------------------------------------------------------------ the command line
def _cli(tmp_path, out, *flags):
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    return cli.main([scenes.scene_path("cornell12"), f"--sky={hdr}", "--w=16", "--h=12", "--samples=4", "--bounces=2",
                     "--hostsim", "--camera=cornell", f"--out={out}", *flags])


PNGS = ("RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png")


def test_cli_dof(tmp_path, capsys):
    for bad, word in (("--dof=-1", "--dof=COC_INF"), ("--dof=inf", "--dof=COC_INF"), ("--focus=2", "need --dof"),
                      ("--focus-at=3,3", "need --dof")):
        assert _cli(tmp_path, tmp_path / "bad", bad) == 2
        assert word in capsys.readouterr().err
    for extra, word in (("--focus=0", "--focus=T"), ("--focus-at=16,3", "--focus-at=X,Y"), ("--focus-at=a,b", "--focus-at=X,Y"),
                        ("--focus-at=3", "--focus-at=X,Y"), ("--focus-at=1.5,2", "--focus-at=X,Y"), ("--focus-at=", "--focus-at=X,Y")):
        assert _cli(tmp_path, tmp_path / "bad", "--dof", extra) == 2
        assert word in capsys.readouterr().err
    assert _cli(tmp_path, tmp_path / "bad", "--dof", "--focus=2", "--focus-at=3,3") == 2
    assert "do not go together" in capsys.readouterr().err
    assert _cli(tmp_path, tmp_path / "plain") == 0
    assert "dof:" not in capsys.readouterr().out
    # a radius of 0 blurs nothing: the bytes of a run without the flag
    assert _cli(tmp_path, tmp_path / "zero", "--dof=0") == 0
    assert "dof: focus" in capsys.readouterr().out
    for name in PNGS:
        assert (tmp_path / "zero" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    # the frame the run renders, its guides and the three ways to focus
    rk, fb = _small_kernel(rt_amd.read_image_float(str(tmp_path / "sky.hdr")))
    rk.render_linear()
    nd = rk.features()[1]
    for flags, kw in ((("--dof",), dict(focus=rt_amd.focus_at(nd, 8, 6))),
                      (("--dof=6", "--focus-at=2,9"), dict(focus=rt_amd.focus_at(nd, 2, 9), coc_inf=6.0)),
                      (("--dof=6", "--focus=1.5"), dict(focus=1.5, coc_inf=6.0))):
        out = tmp_path / "_".join(flags).strip("-").replace("=", "_").replace(",", "_")
        assert _cli(tmp_path, out, *flags, f"--hdr-out={out}.hdr") == 0
        assert f"dof: focus {kw['focus']:.9g}, coc_inf {kw.get('coc_inf', 4.0):.9g}, max_radius 8" in capsys.readouterr().out
        rt_amd.write_image_png(rk.display(rk.dof(fb, nd, kw), exposure=1.5, gamma=2.2), str(tmp_path / "want.png"))
        assert (out / "RT_output.png").read_bytes() == (tmp_path / "want.png").read_bytes()
        assert (out / "RT_output.png").read_bytes() != (tmp_path / "plain" / "RT_output.png").read_bytes()
        rt_amd.write_image_hdr(fb, str(tmp_path / "want.hdr"))
        assert open(f"{out}.hdr", "rb").read() == (tmp_path / "want.hdr").read_bytes(), "--hdr-out stays the sharp frame"
    # the lens, then the meter, then the glow, then the display
    assert _cli(tmp_path, tmp_path / "all", "--dof", "--bloom", "--auto-exposure") == 0
    text = capsys.readouterr().out
    blurred = rk.dof(fb, nd, dict(focus=rt_amd.focus_at(nd, 8, 6)))
    e = rk.auto_exposure(blurred)
    assert f"auto-exposure: {e:.9g}" in text and text.index("dof:") < text.index("auto-exposure:") < text.index("bloom:")
    rt_amd.write_image_png(rk.display(rk.bloom(blurred), exposure=e, gamma=2.2), str(tmp_path / "want.png"))
    assert (tmp_path / "all" / "RT_output.png").read_bytes() == (tmp_path / "want.png").read_bytes()
