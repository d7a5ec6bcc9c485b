"""Exposure metering on the hostsim build (rt_meter, rt_meter_solve; include/rt_hip.h): the histogram against
meter_cases.model(), word for word; its invariants and argument errors; the solve against meter_cases.solve_model()
and on hand-built histograms; ExposureAdapter and the command line's --auto-exposure."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import dnv_cases as dv
import meter_cases as mc
import noise_cases as nc
import rt_amd
import scenes
from meter_cases import frame, hist_of, meter, solve, solve_model
from rt_amd import cli, ptr

f32, u32 = np.float32, np.uint32


def close(got, want, what=""):
    assert abs(got - want) <= mc.SOLVE_RTOL * abs(want), f"{what}: got {got!r}, want {want!r}"


def close_result(got, want, what=""):
    for k in ("exposure", "target", "log2_mean"):
        close(got[k], want[k], f"{what} {k}")
    assert got["valid"] == want["valid"], what


# ------------------------------------------------------------------ the histogram
def test_edge_pixels_are_found():
    """Every bin's lower edge and the float below it, as a luminance: the search finds all 256 edges (at least 250
    are asked for). Grey alone reaches 192 of them, six of the eight mantissa steps of every octave, because the
    float weights do not sum to 1; the other 64 take an (r, g, g) triple."""
    rgb, grey_hits = mc.edge_pixels()
    bits = mc.luminance32(rgb).view(u32)
    want = (np.arange(256, dtype=np.int64) + mc.K0) << 20
    found = int((bits[0::2] == want).sum())
    print(f"meter edges: {found} of 256 found, {grey_hits} of them grey")
    assert found >= 250 and found == 256
    assert (bits[1::2] == want - 1).all()
    hist = mc.model(np.concatenate([rgb, np.ones((512, 1), f32)], 1).reshape(1, 512, 4))
    # bin b holds its own lower edge and the float below bin b + 1's; the float below bin 0's edge is `under`
    assert hist[0] == 3 and (hist[1:255] == 2).all() and hist[255] == 1
    assert hist[mc.UNDER] == 1 and hist[mc.OVER] == 0 and hist[mc.COUNTED] == 512


@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("w,h", mc.SHAPES)
def test_hostsim_equals_the_model_word_for_word(w, h, kind):
    rgba = frame(kind, w, h)
    keep = rgba.copy()
    got = meter(rgba)
    mc.assert_words(got, mc.model(rgba), f"{kind} {w}x{h}")
    assert int(got[:256].sum()) == int(got[mc.COUNTED])
    assert int(got[mc.COUNTED]) + int(got[mc.NONPOSITIVE]) + int(got[mc.NONFINITE]) == w * h
    assert got[mc.RESERVED] == 0
    nc.assert_bits(rgba, keep, "the input changed")
    if kind == "noise" and w * h > 1000:
        assert got[mc.UNDER] > 0 and got[mc.OVER] > 0
        assert w * h < 8000 or (got[:256] > 0).all(), "8710 pixels over 304 eighth-octaves reach every bin"
    if kind == "specials" and w * h > 1000:
        assert got[mc.NONFINITE] > 0 and got[mc.NONPOSITIVE] > 0 and got[mc.UNDER] > 0 and got[mc.OVER] > 0
        assert got[mc.MIN_BITS] == 1, "the smallest denormal"
    if kind == "constant":
        assert got[:256].max() == w * h and got[mc.MAX_BITS] == got[mc.MIN_BITS]
    if kind == "black":
        assert got[mc.COUNTED] == 0 and got[mc.NONPOSITIVE] == w * h
        assert got[mc.MAX_BITS] == 0 and got[mc.MIN_BITS] == 0xFFFFFFFF


def test_argument_errors():
    rgba = frame("noise", 5, 3)
    L, h = mc.ctx(True)
    ARG = rt_amd.RT_ERR_ARG

    def rc(**over):
        r = meter(rgba, code=True, **over)
        assert r == 0 or L.rt_last_error(h)
        return r

    assert rc() == 0
    for kw in (dict(w=0), dict(h=0), dict(w=-3)):
        assert rc(**kw) == ARG and b"at least 1" in L.rt_last_error(h)
    assert rc(src=None) == ARG and rc(out=None) == ARG and b"NULL" in L.rt_last_error(h)
    assert rc(w=1 << 14, h=1 << 13) == ARG and b"too many pixels" in L.rt_last_error(h)
    out = np.zeros(mc.WORDS, u32)
    assert L.rt_meter(None, 5, 3, ptr(rgba), ptr(out)) == ARG
    # the device form's alignment rules
    odd4 = np.zeros(16 * 15 + 16, np.uint8)[4:]
    odd1 = np.zeros(4 * mc.WORDS + 8, np.uint8)[1:]
    assert L.rt_meter_device(h, 5, 3, ptr(rgba), ptr(out), None) == 0, L.rt_last_error(h)
    mc.assert_words(out, mc.model(rgba), "the device form on the hostsim build")
    assert L.rt_meter_device(h, 5, 3, ptr(odd4), ptr(out), None) == ARG and b"aligned" in L.rt_last_error(h)
    assert L.rt_meter_device(h, 5, 3, ptr(rgba), ptr(odd1), None) == ARG and b"aligned" in L.rt_last_error(h)
    assert L.rt_meter(h, 5, 3, ptr(odd4), ptr(out)) == 0, "the host form takes any alignment"
    for key in (b"mt_variant", b"mt_blocks"):
        assert L.rt_test_schedule(h, key, 2.0) == 0 and L.rt_test_schedule(h, key, 0.0) == 0


def test_multi_device_context_runs_the_stage():
    m = nc.Session(True, name="meter-multi", devices=[0, 1])
    rgba = frame("specials", 37, 29)
    out = np.zeros(mc.WORDS, u32)
    m.ok(m.L.rt_meter(m.ctx, 37, 29, ptr(rgba), ptr(out)), "rt_meter")
    mc.assert_words(out, mc.host_result("specials", 37, 29), "multi-device context")
    m.close()


# ------------------------------------------------------------------ the solve
@pytest.mark.parametrize("kind", ["noise", "specials", "constant"])
@pytest.mark.parametrize("w,h", [(37, 29), (130, 67)])
def test_solve_agrees_with_the_float64_model(w, h, kind):
    hist = mc.host_result(kind, w, h)
    for kw in ({}, dict(low=0.0, high=1.0), dict(low=0.3, high=0.6, key=0.5), dict(key=0.05, min_exposure=0.5),
               dict(tau_up=0.7, tau_down=0.2)):
        for prev, dt in ((0.0, 0.0), (1.5, 0.1), (3000.0, 0.4), (1e-3, 2.0)):
            got, want = solve(hist, prev, dt, **kw), solve_model(hist, prev, dt, **kw)
            close_result(got, want, f"{kind} {w}x{h} {kw} prev {prev} dt {dt}")
            assert got["valid"]


def test_trim_is_exact_on_hand_built_histograms():
    key_term = -np.log1p(-float(f32(0.18)))
    # all mass in one bin: the trim removes from it and the mean stays the bin's middle
    r = solve(hist_of({100: 1000}))
    close(r["log2_mean"], (2 * 100 - 319) / 16.0, "one bin")
    close(r["target"], key_term / 2.0 ** ((2 * 100 - 319) / 16.0), "one bin")
    # two spikes: low = 0.25 removes the whole dark one, high = 1 keeps the bright one whole
    two = hist_of({40: 250, 200: 750})
    close(solve(two, low=0.25, high=1.0)["log2_mean"], (2 * 200 - 319) / 16.0, "the dark spike is cut away")
    close(solve(two, low=0.0, high=0.25)["log2_mean"], (2 * 40 - 319) / 16.0, "the bright spike is cut away")
    # one sample short of the spike: one dark sample stays in the mean
    short = solve(two, low=0.2495, high=1.0)  # (floor(249.5) = 249)
    close(short["log2_mean"], (1 * (2 * 40 - 319) + 750 * (2 * 200 - 319)) / (16.0 * 751), "249 of 250 removed")
    close(solve(two, low=0.0, high=1.0)["log2_mean"], (250 * (2 * 40 - 319) + 750 * (2 * 200 - 319)) / 16000.0, "no trim")
    # lo + hi >= n: nothing is trimmed (low = high = 0.5 asks for all 1000)
    close(solve(two, low=0.5, high=0.5)["log2_mean"], (250 * (2 * 40 - 319) + 750 * (2 * 200 - 319)) / 16000.0, "lo + hi = n")
    one = hist_of({7: 1})
    assert solve(one)["valid"] and solve(one)["log2_mean"] == (2 * 7 - 319) / 16.0
    # the trim crosses bins from both ends
    ramp = hist_of({b: 10 for b in range(100, 110)})
    close(solve(ramp, low=0.25, high=0.75)["log2_mean"],
          (5 * (2 * 102 - 319) + sum(10 * (2 * b - 319) for b in range(103, 107)) + 5 * (2 * 107 - 319)) / (16.0 * 50), "ramp")
    for h in (two, ramp, hist_of({0: 3, 255: 5})):
        for kw in (dict(), dict(low=0.3, high=0.7), dict(low=0.0, high=0.5)):
            close_result(solve(h, **kw), solve_model(h, **kw), f"hand-built {kw}")


def test_clamping_to_both_bounds():
    dark, bright = hist_of({0: 100}), hist_of({255: 100})
    assert solve(dark)["target"] == 4096.0 and solve(dark)["exposure"] == 4096.0
    assert solve(bright)["target"] == 2.0 ** -8
    assert solve(dark, max_exposure=8.0)["exposure"] == 8.0 and solve(bright, min_exposure=0.5)["exposure"] == 0.5
    mid = hist_of({160: 100})  # (log2 luminance 1/16: inside the bounds)
    t = solve(mid)["target"]
    assert 2.0 ** -8 < t < 4096.0
    assert solve(mid, min_exposure=t, max_exposure=t)["exposure"] == t


def test_adaptation():
    h = hist_of({150: 400, 170: 600})
    target = solve(h)["target"]
    up, down = target / 8.0, target * 8.0
    taus = dict(tau_up=2.0, tau_down=0.5)
    close(solve(h, up, 0.0, **taus)["exposure"], float(f32(up)), "dt = 0 keeps prev")
    close(solve(h, down, 0.0, **taus)["exposure"], float(f32(down)), "dt = 0 keeps prev")
    close(solve(h, up, 1e30, **taus)["exposure"], target, "dt -> inf reaches the target")
    close(solve(h, down, np.inf, **taus)["exposure"], target, "dt = inf reaches the target")
    # the direction picks the time constant: after dt = tau the exposure has gone 1 - 1/e of the way, in log2
    for prev, tau_dt, other in ((up, 2.0, 0.5), (down, 0.5, 2.0)):
        want = 2.0 ** (np.log2(float(f32(prev))) + (np.log2(target) - np.log2(float(f32(prev)))) * (1 - np.exp(-1.0)))
        close(solve(h, prev, tau_dt, **taus)["exposure"], want, "dt = tau")
        assert abs(solve(h, prev, other, **taus)["exposure"] - want) > 1e-3 * want
    assert solve(h, up, 1.0, tau_up=0.0, tau_down=3.0)["exposure"] == target, "tau_up = 0: at once"
    assert solve(h, down, 1.0, tau_up=3.0, tau_down=0.0)["exposure"] == target
    for prev in (0.0, -1.0, np.nan):
        assert solve(h, prev, 0.1, **taus)["exposure"] == target, "no previous exposure: jump"
    assert solve(h, up, -1.0, **taus)["exposure"] == target, "a negative dt: jump"
    for prev, dt in ((up, 0.3), (down, 0.3), (target, 1.0)):
        close_result(solve(h, prev, dt, **taus), solve_model(h, prev, dt, **taus), f"prev {prev} dt {dt}")
    assert solve(h, up, 0.3, **taus)["target"] == target, "target is the exposure before the adaptation"


def test_empty_histogram():
    for h in (hist_of({}), mc.host_result("black", 37, 29)):
        for prev, want in ((0.0, 1.5), (-2.0, 1.5), (0.75, 0.75)):
            r = solve(h, prev, 0.1, tau_up=1.0, tau_down=1.0)
            assert r == dict(exposure=want, target=want, log2_mean=0.0, valid=False)


def test_solve_argument_errors():
    h = hist_of({100: 10})
    L = rt_amd.lib(True)
    ARG = rt_amd.RT_ERR_ARG
    assert solve(h, code=True) == 0
    for kw in (dict(low=-0.1), dict(low=1.5), dict(high=1.1), dict(high=-0.2), dict(low=0.6, high=0.4), dict(low=np.nan)):
        assert solve(h, code=True, **kw) == ARG and b"low" in L.rt_last_error(None), kw
    assert solve(h, code=True, low=0.0, high=0.0) == 0 and solve(h, code=True, low=1.0, high=1.0) == 0
    for kw in (dict(key=0.0), dict(key=1.0), dict(key=-0.5), dict(key=np.nan)):
        assert solve(h, code=True, **kw) == ARG and b"key" in L.rt_last_error(None), kw
    for kw in (dict(min_exposure=0.0), dict(min_exposure=-1.0), dict(max_exposure=np.inf), dict(min_exposure=np.nan),
               dict(min_exposure=8.0, max_exposure=4.0)):
        assert solve(h, code=True, **kw) == ARG and b"bounds" in L.rt_last_error(None), kw
    for kw in (dict(tau_up=-1.0), dict(tau_down=-0.1), dict(tau_up=np.nan)):
        assert solve(h, code=True, **kw) == ARG and b"tau" in L.rt_last_error(None), kw
    r = rt_amd.MeterResult()
    assert L.rt_meter_solve(None, None, 0.0, 0.0, ctypes.byref(r)) == ARG
    assert L.rt_meter_solve(ptr(h), None, 0.0, 0.0, None) == ARG
    assert L.rt_meter_solve(ptr(h), None, 0.0, 0.0, ctypes.byref(r)) == 0 and r.exposure == solve(h)["exposure"]
    d = rt_amd.meter_default_params(hostsim=True)
    assert (d.low, d.high, d.key, d.min_exposure, d.max_exposure, d.tau_up, d.tau_down) == \
        (f32(0.10), f32(0.95), f32(0.18), 2.0 ** -8, 4096.0, 0.0, 0.0)


# ------------------------------------------------------------------ the Python bindings
def test_python_meter_and_auto_exposure(cameras, manifest):
    rk, _ = dv.cornell_kernel(cameras, manifest, True, 24, 20, 4, 3)
    rgba = frame("noise", 37, 29)  # (the stage takes any frame size, not only the kernel's)
    want = mc.host_result("noise", 37, 29)
    for linear in (rt_amd.Image(37, 29, pixels=rgba), rgba):
        mc.assert_words(rk.meter(linear), want, "RenderKernel.meter")
    s = rt_amd.meter_stats(want)
    assert s["counted"] == int(want[mc.COUNTED]) and s["min_bits"] == int(want[mc.MIN_BITS]) and s["bins"].shape == (256,)
    assert rt_amd.meter_solve(want, hostsim=True) == solve(want)
    assert rt_amd.meter_solve(want, 2.0, 0.5, hostsim=True, tau_down=1.0, key=0.3) == solve(want, 2.0, 0.5, tau_down=1.0, key=0.3)
    p = rt_amd.meter_default_params(hostsim=True)
    p.key = 0.3
    assert rt_amd.meter_solve(want, hostsim=True, params=p) == solve(want, key=0.3)
    assert rk.auto_exposure(rgba) == solve(want)["exposure"]
    full = rk.auto_exposure(rgba, prev=2.0, dt=0.5, full=True, tau_down=1.0)
    assert {k: full[k] for k in ("exposure", "target", "log2_mean", "valid")} == solve(want, 2.0, 0.5, tau_down=1.0)
    mc.assert_words(full["hist"], want, "auto_exposure(full=True) hands the histogram on")
    rk.render_linear()
    assert rk.auto_exposure() == solve(meter(rk.frame_buffer.pixels))["exposure"], "the bound Image by default"
    with pytest.raises(TypeError):
        rk.auto_exposure(rgba, kee=0.2)
    with pytest.raises(rt_amd.RtError):
        rk.auto_exposure(rgba, key=1.5)


def test_exposure_adapter_over_three_frames(cameras, manifest):
    rk, _ = dv.cornell_kernel(cameras, manifest, True, 24, 20, 4, 3)
    frames = [np.full((20, 24, 4), v, f32) for v in (0.18, 1.5, 0.02)]  # (mid, brighter: exposure falls, darker: rises)
    ad = rt_amd.ExposureAdapter(tau_up=2.0, tau_down=0.5, kernel=rk, key=0.25)
    prev, got = 0.0, []
    for fr, dt in zip(frames, (0.0, 0.25, 0.25)):
        want = solve(meter(fr), prev, dt, tau_up=2.0, tau_down=0.5, key=0.25)
        e = ad.update(fr, dt)
        assert e == want["exposure"] and ad.exposure == e and ad.last["target"] == want["target"]
        got.append((e, want["target"]))
        prev = e
    assert got[0][0] == got[0][1], "the first frame jumps to its target"
    assert got[1][1] < got[1][0] < got[0][0], "the second moves down towards its target and does not reach it"
    assert got[1][0] < got[2][0] < got[2][1], "the third moves up"
    ad.reset()
    assert ad.update(frames[2], 0.25) == got[2][1], "after reset() the next frame jumps"
    bare = rt_amd.ExposureAdapter(2.0, 0.5)
    with pytest.raises(ValueError):
        bare.update(frames[0], 0.1)
    assert bare.update(frames[0], 0.1, kernel=rk) == solve(meter(frames[0]))["exposure"]


# ------------------------------------------------------------------ the command line
def _cli(tmp_path, out, *flags):
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    return cli.main([scenes.scene_path("cornell12"), f"--sky={hdr}", "--w=16", "--h=12", "--samples=4", "--bounces=2",
                     "--hostsim", "--camera=cornell", f"--out={out}", *flags])


def _exposures(text):
    return [(s.split(":")[0], float(s.split(":")[1])) for s in text.splitlines() if s.startswith("auto-exposure")]


def test_cli_auto_exposure(tmp_path, capsys):
    for flags in (("--auto-exposure", "--exposure=2"), ("--exposure=1.5", "--auto-exposure=0.18")):
        assert _cli(tmp_path, tmp_path / "bad", *flags) == 2
        assert "does not go with --exposure=" in capsys.readouterr().err
    assert _cli(tmp_path, tmp_path / "bad", "--auto-exposure=1.5") == 2
    assert "KEY" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "bad")
    # the frame the run renders, and what auto_exposure gives for it
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    hdr = rt_amd.read_image_float(str(tmp_path / "sky.hdr"))
    fb = rt_amd.Image(16, 12)
    rk = rt_amd.RenderKernel(16, 12, 4, 2, fb, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices, None,
                             rt_amd.BVH(P.triangles), hdr, rt_amd.compute_env_map_cdf(hdr), hostsim=True)
    rk.set_camera(rt_amd.Camera.preset("cornell"))
    rk.render_linear()
    for flag, kw in (("--auto-exposure=0.18", dict(key=0.18)), ("--auto-exposure", {}), ("--auto-exposure=0.4", dict(key=0.4))):
        out = tmp_path / flag.strip("-").replace("=", "_")
        assert _cli(tmp_path, out, flag) == 0
        lines = _exposures(capsys.readouterr().out)
        want = rk.auto_exposure(fb, **kw)
        assert len(lines) == 1 and lines[0][0] == "auto-exposure"
        assert f32(lines[0][1]) == f32(want), "the printed exposure is auto_exposure of render_linear's frame"
        rt_amd.write_image_png(rk.display(fb, exposure=want, gamma=2.2), str(tmp_path / "want.png"))
        assert (out / "RT_output.png").read_bytes() == (tmp_path / "want.png").read_bytes()
    assert rk.auto_exposure(fb, key=0.4) > rk.auto_exposure(fb)
    # previews are metered one by one, then the final frame
    assert _cli(tmp_path, tmp_path / "prev", "--auto-exposure", "--preview-every=2") == 0
    lines = _exposures(capsys.readouterr().out)
    assert [n for n, _ in lines] == ["auto-exposure (preview 2)", "auto-exposure (preview 4)", "auto-exposure"]
    assert f32(lines[2][1]) == f32(rk.auto_exposure(fb)) and lines[1][1] == lines[2][1] and lines[0][1] != lines[1][1]
    # a run without the flag prints no such line
    assert _cli(tmp_path, tmp_path / "plain", "--gamma=2.2") == 0
    assert "auto-exposure" not in capsys.readouterr().out
