"""The bindings of the firefly rejection stage against the C calls, on the hostsim build: RenderKernel.firefly_clamp
and TemporalHistory.push(firefly=...) of rt_amd, and the command line's --firefly. (The C++ drop-in's
RenderKernel::firefly_clamp is a row of tests/test_shims.py.)"""
from __future__ import annotations

import numpy as np
import pytest

import dnv_cases as dv
import firefly_cases as fc
import noise_cases as nc
import rt_amd
import scenes
import temporal_cases as tc
from rt_amd import cli


def test_python_firefly_clamp_equals_the_c_abi(cameras, manifest):
    rk, _ = dv.cornell_kernel(cameras, manifest, True, 24, 20, 4, 3)
    rgba, sigma = fc.inputs(37, 29)  # (the stage takes any frame size, not only the kernel's)
    img = rt_amd.Image(37, 29, pixels=rgba)
    want = fc.clamp(rgba, sigma, None)
    out, s_out = rk.firefly_clamp(img, sigma)
    nc.assert_bits(out.pixels, want[0], "firefly_clamp at the defaults: colour")
    nc.assert_bits(s_out, want[1], "firefly_clamp at the defaults: sigma")
    want = fc.clamp(rgba, sigma, fc.params(2, 3, 1.5, 0.01))
    for params in ({"radius": 2, "rank": 3, "gain": 1.5, "floor": 0.01}, rt_amd.FireflyParams(2, 3, 1.5, 0.01)):
        got = rk.firefly_clamp(img, sigma, params, return_scale=True)
        for g, w, name in zip((got[0].pixels, got[1], got[2]), want, ("colour", "sigma", "scale")):
            nc.assert_bits(g, w, f"firefly_clamp with {type(params).__name__}: {name}")
    bare = rk.firefly_clamp(img, None, {"radius": 2, "rank": 3, "gain": 1.5, "floor": 0.01})
    assert bare[1] is None
    nc.assert_bits(bare[0].pixels, want[0], "firefly_clamp without a sigma")
    d = rt_amd.firefly_default_params(hostsim=True)
    assert (d.radius, d.rank, d.gain, d.floor) == (1, 2, 2.0, 0.0)
    with pytest.raises(TypeError):
        rk.firefly_clamp(img, sigma, {"radious": 2})
    with pytest.raises(rt_amd.RtError):
        rk.firefly_clamp(img, sigma, {"rank": 9})


def test_temporal_history_push_with_and_without_firefly(cameras, manifest):
    rk, _ = dv.cornell_kernel(cameras, manifest, True, 24, 20, 4, 3)
    frames = []
    for k in range(2):
        rk.set_camera(tc.moved_camera(k, 0.05))
        frames.append(tc.recipe_frame(rk, k, 8, 4, 24, 20))
    plain, none, clamped, by_hand = (rt_amd.TemporalHistory() for _ in range(4))
    p = {"gain": 1.0}  # (gain 1: this small frame has clamped pixels)
    for k, (lin, sigma) in enumerate(frames):
        rk.set_camera(tc.moved_camera(k, 0.05))
        a = plain.push(rk, lin, sigma)
        b = none.push(rk, lin, sigma, firefly=None)
        c = clamped.push(rk, lin, sigma, firefly=p)
        ff, ff_sigma, scale = rk.firefly_clamp(lin, sigma, p, return_scale=True)
        d = by_hand.push(rk, ff, ff_sigma)
        assert (scale < 1).any()
        for x, y, z, w, name in zip(a, b, c, d, ("colour", "sigma", "length")):
            px = lambda v: getattr(v, "pixels", v)  # noqa: E731
            nc.assert_bits(px(y), px(x), f"frame {k}: push(firefly=None) is push(): {name}")
            nc.assert_bits(px(z), px(w), f"frame {k}: push(firefly=p) is firefly_clamp, then push(): {name}")
        assert (a[0].pixels != c[0].pixels).any()


def _cli(tmp_path, out, *flags):
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    return cli.main([scenes.scene_path("cornell12"), f"--sky={hdr}", "--w=16", "--h=12", "--samples=4", "--bounces=2",
                     "--hostsim", "--camera=cornell", f"--out={out}", *flags])


NAMES = ("RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png")


def test_cli_firefly(tmp_path, capsys):
    prog = ("--preview-every=1", "--noise-threshold=0")
    for flags in (("--firefly",), ("--firefly=2",) + prog, ("--firefly", "--denoise=atrous") + prog):
        assert _cli(tmp_path, tmp_path / "bad", *flags) == 2
        assert "--firefly needs --denoise=var" in capsys.readouterr().err
    assert _cli(tmp_path, tmp_path / "bad", "--firefly=-1", "--denoise=var", *prog) == 2
    var, same, on = tmp_path / "var", tmp_path / "same", tmp_path / "on"
    assert _cli(tmp_path, var, "--denoise=var", *prog) == 0
    assert "firefly:" not in capsys.readouterr().out
    # an infinite gain is the identity: the files of the run without the flag
    assert _cli(tmp_path, same, "--denoise=var", "--firefly=inf", *prog) == 0
    assert "firefly: clamped 0 of 192 pixels" in capsys.readouterr().out
    for n in NAMES:
        assert (var / n).read_bytes() == (same / n).read_bytes(), n
    assert _cli(tmp_path, on, "--denoise=var", "--firefly=1", *prog) == 0
    line = [s for s in capsys.readouterr().out.splitlines() if s.startswith("firefly: clamped")]
    assert line and int(line[0].split()[2]) > 0
    assert (var / NAMES[0]).read_bytes() == (on / NAMES[0]).read_bytes(), "the render itself is not clamped"
    assert (var / NAMES[1]).read_bytes() != (on / NAMES[1]).read_bytes(), "the filter took the clamped frame"
    # the run without the flag is the chain it was: resolve, noise figure, filter, display
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    hdr = rt_amd.read_image_float(str(tmp_path / "sky.hdr"))
    fb = rt_amd.Image(16, 12)
    rk = rt_amd.RenderKernel(16, 12, 4, 2, fb, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices, None,
                             rt_amd.BVH(P.triangles), hdr, rt_amd.compute_env_map_cdf(hdr), hostsim=True)
    rk.set_camera(rt_amd.Camera.preset("cornell"))
    rk.progress_begin()
    rk.progress_track_noise()
    for _ in range(4):
        rk.progress_advance(1)
        if _ and rk.progress_noise(0.0)["tiles_over"] == 0:
            break
    rk.progress_resolve_linear(fb)
    with np.errstate(all="ignore"):
        shown = rk.display(rk.denoise_var(fb, None, 1.0), exposure=1.5, gamma=2.2)
        rt_amd.write_image_png(cli.blend(shown, rk.display(fb, exposure=1.5, gamma=2.2), 1.0), str(tmp_path / "chain.png"))
    assert (var / NAMES[1]).read_bytes() == (tmp_path / "chain.png").read_bytes()
