"""The motion stages on the hostsim build (rt_motion_vectors, rt_motion_blur; include/rt_hip.h): the vectors against
motion_cases.vectors_model(), bit for bit; the blur against motion_cases.model(), a restatement of rt_motion.h's header
comment with float64 sums; the exact properties; the argument errors; the Python layer; the command line's --motion-blur."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import motion_cases as mc
import noise_cases as nc
import rt_amd
import scenes
import temporal_cases as tc
from motion_cases import blur, clean, field, inputs, params, vectors
from rt_amd import cli, ptr

f32 = np.float32


def _flat(w, h, colour=(0.4, 0.3, 0.2, 0.7), t=2.0):
    rgba = np.empty((h, w, 4), f32)
    rgba[...] = colour
    nd = np.zeros((h, w, 4), f32)
    nd[..., 3] = t
    return rgba, nd


# ------------------------------------------------------------------ vectors
@pytest.mark.parametrize("w,h", tc.SHAPES)
def test_vectors_of_the_same_camera_are_zero(w, h):
    cur, prev = tc.cameras("same", w, h)
    m = vectors(cur, prev, tc.normal_depth(cur, w, h))
    assert np.abs(m).max() < 1e-3


@pytest.mark.parametrize("kind", ["turn", "shift"])
@pytest.mark.parametrize("w,h", tc.SHAPES)
def test_vectors_equal_the_float32_model(w, h, kind):
    cur, prev = tc.cameras(kind, w, h)
    nd = tc.normal_depth(cur, w, h)
    keep = nd.copy()
    got = vectors(cur, prev, nd)
    nc.assert_bits(got, mc.vectors_model(cur, prev, nd), f"{kind} {w}x{h}: the vectors")
    nc.assert_bits(nd, keep, "the guide changed")
    if (w, h) != (1, 1):
        assert np.abs(got).max() > 0.3, "the camera moved"


def test_vectors_of_a_nan_guide_and_of_a_point_behind_the_previous_camera_are_zero():
    w, h = 37, 29
    cur, prev = tc.cameras("turn", w, h)
    nd = tc.normal_depth(cur, w, h)
    for k in range(4):
        nd[3 + k, 5, k] = np.nan
    got = vectors(cur, prev, nd)
    assert np.all(got[3:7, 5] == 0.0) and np.any(got[8, 5] != 0.0)
    cur, away = tc.cameras("away", w, h)
    assert np.all(vectors(cur, away, tc.normal_depth(cur, w, h)) == 0.0), "everything in view is behind a camera turned by 180 degrees"


def test_vectors_of_a_miss_move_by_rotation_only():
    w, h = 37, 29
    cur, _ = tc.cameras("same", w, h)
    nd = np.zeros((h, w, 4), f32)
    nd[..., 3] = -1.0
    assert np.abs(vectors(cur, tc._cam((5.0, -3.0, 2.0), 0.0), nd)).max() < 1e-3, "a translation does not move the sky"
    turned = vectors(cur, tc._cam((0.0, 0.1, 1.0), 5.0), nd)
    # (P = o_prev + d is rounded at |o_prev| = 6: a few float32 ulps of 6 times the 37 pixels per unit)
    assert np.abs(turned - vectors(cur, tc._cam((5.0, -3.0, 2.0), 5.0), nd)).max() < 1e-3, "nor on top of a rotation"
    assert np.abs(turned[..., 0]).min() > 1.0, "a yaw does"
    nc.assert_bits(turned, mc.vectors_model(cur, tc._cam((0.0, 0.1, 1.0), 5.0), nd), "the model's miss")


def test_vectors_argument_errors():
    w, h = 5, 3
    cur, prev = tc.cameras("turn", w, h)
    nd = tc.normal_depth(cur, w, h)
    L, hnd = tc.ctx(True, cur)
    ARG = rt_amd.RT_ERR_ARG

    def rc(**over):
        r = vectors(cur, prev, nd, code=True, **over)
        assert r == 0 or L.rt_last_error(hnd).startswith(b"rt_motion_vectors:"), L.rt_last_error(hnd)
        return r

    assert rc() == 0
    for kw in (dict(w=0), dict(h=-1), dict(nd_in=None), dict(out=None), dict(prev_view=None)):
        assert rc(**kw) == ARG, kw
    for v in (0.0, np.nan, np.inf):
        assert rc(prev_fov=v) == ARG and b"prev_fov_dist" in L.rt_last_error(hnd)
    sing = prev.view_matrix.copy()
    sing[2] = 0
    assert rc(prev_view=sing) == ARG and b"singular" in L.rt_last_error(hnd)
    bad = prev.view_matrix.copy()
    bad[1, 1] = np.nan
    assert rc(prev_view=bad) == ARG
    assert rc(out=nd.reshape(-1)[:30].reshape(3, 5, 2)) == ARG and b"overlaps an input" in L.rt_last_error(hnd)
    tall = np.zeros((262141, 1, 4), f32)
    assert L.rt_motion_vectors(hnd, 1, 262141, ptr(tall), ptr(prev.view_matrix), ctypes.c_float(prev.fov_dist), ptr(tall.copy())) == ARG
    assert b"262140" in L.rt_last_error(hnd)
    # the device form's alignment rule: 16 bytes for the guides, 8 for the vectors
    odd8 = np.zeros(16 * 15 + 16, np.uint8)[8:]
    odd4 = np.zeros(8 * 15 + 16, np.uint8)[4:]
    out = np.zeros((3, 5, 2), f32)

    def dev(g=nd, o=out):
        return L.rt_motion_vectors_device(hnd, 5, 3, ptr(g), ptr(prev.view_matrix), ctypes.c_float(prev.fov_dist), ptr(o), None)

    assert dev() == 0, L.rt_last_error(hnd)
    assert dev(o=odd8) == 0, "motion_out needs 8-byte alignment only"
    for kw in (dict(g=odd8), dict(o=odd4)):
        assert dev(**kw) == ARG and b"aligned" in L.rt_last_error(hnd), kw
        assert L.rt_last_error(hnd).startswith(b"rt_motion_vectors_device:")
    bare, h2 = mc.ctx(True)
    assert bare.rt_motion_vectors(h2, 5, 3, ptr(nd), ptr(prev.view_matrix), ctypes.c_float(prev.fov_dist), ptr(out)) == rt_amd.RT_ERR_STATE


# ------------------------------------------------------------------ the blur against the model
@pytest.mark.parametrize("kind", mc.FIELDS)
@pytest.mark.parametrize("max_radius", mc.RADII)
@pytest.mark.parametrize("w,h", mc.SHAPES)
def test_hostsim_matches_float64_model(w, h, max_radius, kind):
    """The largest error over the 60 cases is 4.942e-7 (130x67, max_radius 16, random); every pixel is compared."""
    rgba, nd = inputs(w, h)
    m = field(kind, w, h, max_radius)
    keep = rgba.copy(), nd.copy(), m.copy()
    p = params(max_radius=max_radius)
    out, reach = (a.copy() for a in mc.host_result(w, h, max_radius, kind))
    want, l = mc.model(rgba, nd, m, p)
    e = mc.model_error(out, want)
    print(f"motion model {w}x{h} max_radius {max_radius} {kind}: rgba_out {e:.3e}")
    nc.assert_bits(reach, l, "reach_out is the float32 l")
    nc.assert_bits(out[..., 3], rgba[..., 3], "alpha comes back bit for bit")
    bad = mc.bad_pixels(rgba)
    nc.assert_bits(out[bad], rgba[bad], "a bad centre is copied bit for bit")
    for a, b, name in zip((rgba, nd, m), keep, ("the input", "the guide", "the motion")):
        nc.assert_bits(a, b, name + " changed")
    assert e <= mc.MODEL_TOL
    nc.assert_bits(blur(rgba, nd, m, p, want_reach=False)[0], out, "reach_out NULL: rgba_out")


# ------------------------------------------------------------------ properties
@pytest.mark.parametrize("w,h", mc.SHAPES)
def test_closed_shutter_or_no_motion_returns_the_inputs_bits(w, h):
    rgba, nd = inputs(w, h)
    rgba[0, 0, 2] = -0.0
    for m, p in ((field("random", w, h, 16), params(shutter=0.0, max_radius=16)), (np.zeros((h, w, 2), f32), params(max_radius=16))):
        out, reach = blur(rgba, nd, m, p)
        nc.assert_bits(out, rgba, "the input's bits")
        assert np.all(reach == 0.0)


@pytest.mark.parametrize("kind", mc.FIELDS)
def test_uniform_colour_under_any_motion_stays_uniform(kind):
    rgba, nd = inputs(37, 29)
    rgba[...] = (3.0, 2.0, 1.5, 0.25)
    out, _ = blur(rgba, nd, field(kind, 37, 29, 8), params(max_radius=8))
    err = np.abs(out.astype(np.float64) - rgba) / np.maximum(1.0, rgba)
    assert err.max() <= mc.MODEL_TOL, err.max()


def test_one_bright_pixel_becomes_a_streak_in_its_own_row():
    rgba, nd = _flat(41, 21, colour=(0.0, 0.0, 0.0, 1.0))
    rgba[10, 20, :3] = (100.0, 50.0, 25.0)
    m = np.zeros((21, 41, 2), f32)
    m[...] = (8.0, 0.0)  # h = (4, 0) at shutter 1
    out, reach = blur(rgba, nd, m, params(max_radius=8))
    assert np.all(reach == 4.0)
    assert np.all(out[10, 16:25, 0] > 0), "non-zero within 4 px"
    assert np.all(out[10, :15, :3] == 0) and np.all(out[10, 26:, :3] == 0), "exactly zero beyond 5 px"
    rows = np.arange(21) != 10
    assert np.all(out[rows][..., :3] == 0), "and in every other row"


def test_still_near_pixel_among_moving_far_pixels_comes_back_exactly():
    rgba, nd = clean(37, 29)
    nd[..., 3] = 4.0
    nd[14, 18, 3] = 2.0  # (4 - 2) / (0.05 * 2) is far beyond the fade
    m = np.zeros((29, 37, 2), f32)
    m[...] = (10.0, 6.0)
    m[14, 18] = 0.0
    out, reach = blur(rgba, nd, m, params(max_radius=8))
    assert reach[14, 18] == 0.0 and reach[14, 19] > 5.0
    assert np.array_equal(out[14, 18], rgba[14, 18]), "(2 c) / 2"
    assert not np.array_equal(out[14, 19, :3], rgba[14, 19, :3])


def test_moving_near_pixels_bleed_onto_still_far_neighbours_within_their_reach():
    rgba, nd = _flat(48, 20, colour=(0.0, 0.0, 0.0, 1.0), t=4.0)
    rgba[:, 10:16, :3] = 5.0
    nd[:, 10:16, 3] = 2.0
    m = np.zeros((20, 48, 2), f32)
    m[:, 10:16] = (12.0, 0.0)  # h = (6, 0)
    out, reach = blur(rgba, nd, m, params(max_radius=8))
    assert reach[9, 20] == 0.0 and reach[9, 12] == 6.0
    assert np.all(out[9, 16:21, 0] > 0) and np.all(out[9, 5:10, 0] > 0), "the block bleeds over the still background within its reach"
    assert np.all(out[9, 22:, 0] == 0) and np.all(out[9, :4, 0] == 0), "and no further"


def test_first_of_two_equal_reaches_sets_the_tiles_direction():
    rgba, nd, m, p = mc.tie_case()
    out, reach = blur(rgba, nd, m, p)
    assert reach[2, 3] == 6.0 and reach[9, 10] == 6.0
    want, _ = mc.model(rgba, nd, m, p)
    assert mc.model_error(out, want) <= mc.MODEL_TOL
    # (3, 2) moves along x: its colour spreads along its row; with (10, 9)'s direction it would spread along the column
    probe = rgba.copy()
    probe[..., :3] = 0.0
    probe[2, 3, :3] = 9.0
    streak, _ = blur(probe, nd, m, p)
    assert np.all(streak[2, 1:9, 0] > 0) and np.all(streak[np.arange(29) != 2][..., 0] == 0)
    swapped = m.copy()
    swapped[2, 3], swapped[9, 10] = m[9, 10], m[2, 3]  # now the first in raster order moves along y
    streak, _ = blur(probe, nd, swapped, p)
    assert np.all(streak[0:8, 3, 0] > 0) and np.all(streak[:, np.arange(37) != 3, 0] == 0)


def test_moving_tile_blurs_the_border_of_the_still_tile_beside_it():
    rgba, nd, m, p = mc.border_case()
    out, reach = blur(rgba, nd, m, p)
    assert np.all(reach[:, 32:] == 0.0) and np.all(reach[:, 16:32] == 12.0)
    assert not np.array_equal(out[:, 32:44, :3], rgba[:, 32:44, :3]), "a per-tile maximum alone would copy the still tile"
    assert not np.array_equal(out[:, 4:16, :3], rgba[:, 4:16, :3])
    nc.assert_bits(out[:, 64:], rgba[:, 64:], "tiles beyond the neighbours are copied")
    want, _ = mc.model(rgba, nd, m, p)
    assert mc.model_error(out, want) <= mc.MODEL_TOL


@pytest.mark.parametrize("w,h", [(5, 3), (37, 29)])
def test_a_bad_colour_stays_where_it_is(w, h):
    rgba, nd = inputs(w, h)
    bad = mc.bad_pixels(rgba)
    assert bad.any()
    p = params(max_radius=4)
    m = field("diagonal", w, h, 4)
    out, reach = blur(rgba, nd, m, p)
    nc.assert_bits(out[bad], rgba[bad], "a bad centre is copied bit for bit")
    assert np.isfinite(out[~bad]).all(), "no other pixel's finiteness changed"
    other = rgba.copy()
    other[bad] = (np.inf, 1.0, -np.inf, 0.5)
    out2, reach2 = blur(other, nd, m, p)
    nc.assert_bits(out2[~bad], out[~bad], "the others do not see the bad colour")
    nc.assert_bits(reach2, reach, "nor does the reach")


def test_null_params_are_the_defaults():
    rgba, nd = inputs(37, 29)
    m = field("diagonal", 37, 29, 8)
    d = rt_amd.motion_default_params(hostsim=True)
    assert (d.shutter, d.depth_soft, d.max_radius) == (0.5, f32(0.05), 8)
    for a, b in zip(blur(rgba, nd, m, None), blur(rgba, nd, m, d)):
        nc.assert_bits(a, b, "params NULL: the defaults")


def test_argument_errors():
    rgba, nd = inputs(5, 3)
    m = field("diagonal", 5, 3, 4)
    L, h = mc.ctx(True)
    ARG = rt_amd.RT_ERR_ARG

    def rc(p=None, **over):
        r = blur(rgba, nd, m, p if p is not None else params(), code=True, **over)
        assert r == 0 or L.rt_last_error(h).startswith(b"rt_motion_blur:"), L.rt_last_error(h)
        return r

    assert rc() == 0
    for v in (0, 17, -1):
        assert rc(params(max_radius=v)) == ARG and b"max_radius" in L.rt_last_error(h)
    assert rc(params(max_radius=1)) == 0 and rc(params(max_radius=16)) == 0
    for v in (-0.01, 1.01, np.nan, np.inf, -np.inf):
        assert rc(params(shutter=v)) == ARG and b"shutter" in L.rt_last_error(h), v
    assert rc(params(shutter=0.0)) == 0 and rc(params(shutter=1.0)) == 0
    for v in (0.0, -0.5, np.nan, np.inf, -np.inf):
        assert rc(params(depth_soft=v)) == ARG and b"depth_soft" in L.rt_last_error(h), v
    for kw in (dict(w=0), dict(h=0), dict(w=-3)):
        assert rc(**kw) == ARG and b"at least 1" in L.rt_last_error(h)
    for name in ("rgba_in", "nd_in", "motion_in", "out"):
        assert rc(**{name: None}) == ARG and b"NULL" in L.rt_last_error(h)
    assert rc(reach_out=None) == 0
    # an output that aliases an input or the other output, by pointer and by overlap
    assert rc(out=rgba) == ARG and b"overlaps an input" in L.rt_last_error(h)
    assert rc(out=nd) == ARG and b"overlaps an input" in L.rt_last_error(h)
    assert rc(reach_out=m.reshape(-1)[:15].reshape(3, 5)) == ARG and b"overlaps an input" in L.rt_last_error(h)
    both = np.zeros((3, 5, 4), f32)
    assert rc(out=both, reach_out=both.reshape(-1)[4:19].reshape(3, 5)) == ARG and b"two outputs overlap" in L.rt_last_error(h)
    # rt_denoise's frame-size limits
    tall = np.zeros((262141, 1, 4), f32)
    p = params()
    assert L.rt_motion_blur(h, 1, 262141, ptr(tall), ptr(tall.copy()), ptr(tall.copy()), ctypes.byref(p), ptr(tall.copy()), None) == ARG
    assert b"262140" in L.rt_last_error(h)
    assert L.rt_motion_blur(h, 1 << 14, 1 << 13, ptr(tall), ptr(tall), ptr(tall), ctypes.byref(p), ptr(tall.copy()), None) == ARG
    assert b"rt_motion_blur: too many pixels" in L.rt_last_error(h)
    # the device form's alignment rule
    odd = np.zeros(16 * 15 + 16, np.uint8)
    o4, r1 = np.zeros((3, 5, 4), f32), np.zeros((3, 5), f32)

    def dev(i=rgba, g=nd, mv=m, o=o4, ro=r1):
        return L.rt_motion_blur_device(h, 5, 3, ptr(i), ptr(g), ptr(mv), ctypes.byref(p), ptr(o), ptr(ro), None)

    assert dev() == 0, L.rt_last_error(h)
    assert dev(ro=odd[4:]) == 0 and dev(mv=odd[8:]) == 0, "reach_out needs 4-byte alignment only, motion 8"
    for kw in (dict(i=odd[8:]), dict(g=odd[4:]), dict(o=odd[8:]), dict(mv=odd[4:]), dict(ro=odd[1:])):
        assert dev(**kw) == ARG and b"aligned" in L.rt_last_error(h), kw
        assert L.rt_last_error(h).startswith(b"rt_motion_blur_device:")
    assert L.rt_motion_blur(None, 5, 3, ptr(rgba), ptr(nd), ptr(m), None, ptr(o4), None) == ARG
    for v in (2.0, 7.0, -3.0, 0.0):  # (clamped to 0..2, as dof_variant is)
        assert L.rt_test_schedule(h, b"motion_variant", v) == 0
    assert L.rt_version() == 10002


# ------------------------------------------------------------------ the Python layer
def _small_kernel(sky, camera="cornell"):
    """Cornell 12-tri at 16 x 12 on the hostsim build, 4 samples, 2 bounces."""
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    fb = rt_amd.Image(16, 12)
    rk = rt_amd.RenderKernel(16, 12, 4, 2, fb, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices, None,
                             rt_amd.BVH(P.triangles), sky, rt_amd.compute_env_map_cdf(sky), hostsim=True)
    rk.set_camera(rt_amd.Camera.preset(camera))
    return rk, fb


def test_python_layer():
    rgba, nd = inputs(37, 29)
    rk, _ = _small_kernel(rt_amd.Image.from_rgb(scenes.make_sky("S")))  # (the stages take a frame of any size)
    img = rt_amd.Image(37, 29, pixels=rgba)
    m = field("diagonal", 37, 29, 4)
    want = mc.host_result(37, 29, 4, "diagonal")
    out, reach = rk.motion_blur(img, nd, m, params(max_radius=4), reach=True)
    nc.assert_bits(out.pixels, want[0], "RenderKernel.motion_blur: the frame")
    nc.assert_bits(reach, want[1], "RenderKernel.motion_blur: the reach")
    nc.assert_bits(rk.motion_blur(img, nd, m, dict(shutter=mc.SHUTTER, depth_soft=mc.DEPTH_SOFT, max_radius=4)).pixels, want[0],
                   "a dict of fields")
    assert not np.array_equal(rk.motion_blur(img, nd, m).pixels, want[0])
    with pytest.raises(rt_amd.RtError):
        rk.motion_blur(img, nd, m, dict(max_radius=17))
    with pytest.raises(ValueError):
        rk.motion_blur(img, nd[:5], m)
    with pytest.raises(ValueError):
        rk.motion_blur(img, nd, m[:5])
    # the vectors under the kernel's camera, and TemporalHistory's convenience
    cur, prev = tc.cameras("turn", 37, 29)
    rk.set_camera(cur)
    guide = tc.normal_depth(cur, 37, 29)
    mv = rk.motion_vectors(guide, prev)
    nc.assert_bits(mv, mc.vectors_model(cur, prev, guide), "RenderKernel.motion_vectors")
    nc.assert_bits(rk.motion_vectors(guide, (prev.view_matrix, prev.fov_dist)), mv, "a (view, fov) pair")
    hist = rt_amd.TemporalHistory()
    assert np.abs(hist.motion_vectors(rk, guide)).max() < 1e-3, "before the first push: the kernel's own camera"
    hist.camera = prev
    nc.assert_bits(hist.motion_vectors(rk, guide), mv, "TemporalHistory.motion_vectors passes the previous camera")


# ------------------------------------------------------------------ the command line
def _cli(tmp_path, out, *flags):
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    return cli.main([scenes.scene_path("cornell12"), f"--sky={hdr}", "--w=16", "--h=12", "--samples=4", "--bounces=2",
                     "--hostsim", "--camera=cornell", f"--out={out}", *flags])


PNGS = ("RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png")


def test_cli_motion_blur(tmp_path, capsys):
    for bad, word in (("--motion-blur=-1", "--motion-blur=SHUTTER"), ("--motion-blur=2", "--motion-blur=SHUTTER"),
                      ("--prev-camera=dragon", "needs --motion-blur")):
        assert _cli(tmp_path, tmp_path / "bad", bad) == 2
        assert word in capsys.readouterr().err
    assert _cli(tmp_path, tmp_path / "bad", "--motion-blur") == 2
    assert "--prev-camera=PRESET" in capsys.readouterr().err
    assert _cli(tmp_path, tmp_path / "plain") == 0
    assert "motion blur:" not in capsys.readouterr().out
    # a closed shutter blurs nothing: the bytes of a run without the flag
    assert _cli(tmp_path, tmp_path / "zero", "--motion-blur=0", "--prev-camera=dragon") == 0
    assert "motion blur: shutter 0" in capsys.readouterr().out
    for name in PNGS:
        assert (tmp_path / "zero" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    # the frame the run renders, its guides and its vectors against the previous camera
    rk, fb = _small_kernel(rt_amd.read_image_float(str(tmp_path / "sky.hdr")))
    rk.render_linear()
    nd = rk.features()[1]
    mv = rk.motion_vectors(nd, rt_amd.Camera.preset("dragon"))
    out = tmp_path / "mb"
    assert _cli(tmp_path, out, "--motion-blur", "--prev-camera=dragon", f"--hdr-out={out}.hdr") == 0
    blurred, reach = rk.motion_blur(fb, nd, mv, None, reach=True)
    assert f"motion blur: shutter 0.5, max_radius 8, longest reach {reach.max():.9g}" in capsys.readouterr().out
    rt_amd.write_image_png(rk.display(blurred, exposure=1.5, gamma=2.2), str(tmp_path / "want.png"))
    assert (out / "RT_output.png").read_bytes() == (tmp_path / "want.png").read_bytes()
    assert (out / "RT_output.png").read_bytes() != (tmp_path / "plain" / "RT_output.png").read_bytes()
    rt_amd.write_image_hdr(fb, str(tmp_path / "want.hdr"))
    assert open(f"{out}.hdr", "rb").read() == (tmp_path / "want.hdr").read_bytes(), "--hdr-out stays the sharp frame"
    # the lens, then the shutter, then the meter, then the glow, then the display
    assert _cli(tmp_path, tmp_path / "all", "--dof", "--motion-blur", "--prev-camera=dragon", "--bloom", "--auto-exposure") == 0
    text = capsys.readouterr().out
    lens = rk.dof(fb, nd, dict(focus=rt_amd.focus_at(nd, 8, 6)))
    shut = rk.motion_blur(lens, nd, mv)
    e = rk.auto_exposure(shut)
    assert f"auto-exposure: {e:.9g}" in text
    assert text.index("dof:") < text.index("motion blur:") < text.index("auto-exposure:") < text.index("bloom:")
    rt_amd.write_image_png(rk.display(rk.bloom(shut), exposure=e, gamma=2.2), str(tmp_path / "want.png"))
    assert (tmp_path / "all" / "RT_output.png").read_bytes() == (tmp_path / "want.png").read_bytes()
