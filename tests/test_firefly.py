"""Firefly rejection on the hostsim build (rt_firefly; include/rt_hip.h): against firefly_cases.model(), a float64
restatement of the header comment; the exact properties and argument errors; the sweep and the quality figures of
DESIGN.md §16."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import dnv_cases as dv
import firefly_cases as fc
import noise_cases as nc
import rt_amd
from firefly_cases import clamp, inputs, params
from rt_amd import ptr

f32 = np.float32


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("floor", [0.0, 0.1])
@pytest.mark.parametrize("gain", [1.0, 2.0])
@pytest.mark.parametrize("rank", [1, 2, 3, 8])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_hostsim_matches_float64_model(w, h, radius, rank, gain, floor):
    """The largest errors over all 128 cases: colour 2.31e-7, sigma_out 9.09e-8, scale_out 2.62e-7. A
    pixel within 1e-5 (relative) of its limit is left out: with the seed of firefly_cases.py 11 of the 313568 pixel-cases
    are, in 6 of the 128 cases, at most 0.093 % of a case's pixels. At gain 1 a third of a noisy frame's pixels sit above
    their limit, so over this many pixel-cases no seed leaves none out: seeds 1..5 leave 6 to 16."""
    rgba, sigma = inputs(w, h)
    p = params(radius, rank, gain, floor)
    got = clamp(rgba, sigma, p)
    want = fc.model(rgba, sigma, p)
    near = want[3]
    ec, es, ef = fc.model_errors(got, want)
    print(f"firefly model {w}x{h} R {radius} rank {rank} gain {gain} floor {floor}: left out {int(near.sum())} "
          f"({near.mean():.4f}) colour {ec:.3e} sigma_out {es:.3e} scale_out {ef:.3e} clamped {(got[2] < 1).mean():.3f}")
    assert near.mean() <= fc.NEAR_CAP
    assert ec <= fc.COLOR_TOL and es <= fc.SIGMA_TOL and ef <= fc.SCALE_TOL
    keep = ~near
    assert np.array_equal((got[2] < 1)[keep], (want[2] < 1)[keep]), "the same pixels are clamped"
    if (w, h) == (1, 1):
        assert got[2][0, 0] == 1.0, "no neighbour: untouched"
    elif w >= 37:
        assert (got[2] < 1).any() and (got[2] == 1).any(), "the case has clamped and untouched pixels"


# ------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_untouched_pixels_keep_their_bits_and_scales_are_in_range(w, h, radius):
    rgba, sigma = inputs(w, h)
    keep = (rgba.copy(), sigma.copy())
    out, s_out, scale = clamp(rgba, sigma, params(radius, 2, 1.0, 0.0))
    same = scale == 1.0
    nc.assert_bits(out[same], rgba[same], "colour where scale_out == 1")
    nc.assert_bits(s_out[same], sigma[same], "sigma where scale_out == 1")
    nc.assert_bits(out[..., 3], rgba[..., 3], "alpha is copied")
    finite = np.isfinite(rgba[..., :3]).all(-1)
    assert np.all(scale[finite] > 0) and np.all(scale[finite] <= 1)
    assert np.all(scale[~finite] == 1.0), "a centre that is not finite is kept with scale 1"
    nc.assert_bits(rgba, keep[0], "rgba_in changed")
    nc.assert_bits(sigma, keep[1], "sigma_in changed")
    # a clamped pixel with a NaN or infinite sigma keeps that sigma's bits
    bad = ~same & ~np.isfinite(sigma)
    nc.assert_bits(s_out[bad], sigma[bad], "a non-finite sigma is copied")
    if w >= 37:
        assert not same[8, 10] and not same[4, 5] and bad.sum() >= 2, "the planted NaN and +inf sigmas of clamped pixels"


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_infinite_gain_is_the_identity(w, h, radius):
    rgba, sigma = inputs(w, h)
    out, s_out, scale = clamp(rgba, sigma, params(radius, 2, np.inf, 0.0))
    nc.assert_bits(out, rgba, "gain +inf: colour")
    nc.assert_bits(s_out, sigma, "gain +inf: sigma")
    assert np.all(scale == 1.0)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("w,h", [(37, 29), (130, 67)])
def test_planted_patterns_at_rank_2(w, h, radius):
    """gain 2: a bright pixel is BRIGHT * (1 .. 1.05), so two bright neighbours put the limit at 2 * BRIGHT at least."""
    scale = clamp(*inputs(w, h), params(radius, 2, 2.0, 0.0))[2]
    at = lambda px: np.array([scale[y, x] for (x, y) in px])  # noqa: E731
    assert np.all(at(fc.BAR) == 1.0), "the two-pixel-thick bar is untouched"
    assert np.all(at(fc.LINE[2:-2]) == 1.0), "the interior of the one-pixel-wide line survives"
    assert np.all(at([fc.LONE, *fc.PAIR_H, *fc.PAIR_D]) < 0.1), "the lone spike and both pairs are clamped"
    w1, h1 = w - 1, h - 1
    assert np.all(at([(18, 0), (18, h1), (0, 14), (w1, 14), (0, 0), (w1, 0), (0, h1), (w1, h1)]) < 0.1), "edges and corners"
    assert np.all(at([(27, 11), (31, 10)]) < 0.1), "spikes beside NaN, +inf and negative neighbours"
    assert np.all(at(fc.CLUSTER) == 1.0), "a 2x2 cluster has three bright neighbours per pixel"
    if radius == 1:
        assert np.all(at([fc.LINE[0], fc.LINE[-1]]) < 0.1), "radius 1: a line's end has one bright neighbour"
        assert np.all(clamp(*inputs(w, h), params(1, 4, 2.0, 0.0))[2][4:6, 22:24] < 0.1), "rank 4 clamps the cluster"


def test_optional_buffers():
    rgba, sigma = inputs(37, 29)
    p = params(2, 3, 1.0, 0.01)
    full = clamp(rgba, sigma, p)
    no_sigma = clamp(rgba, None, p)
    assert no_sigma[1] is None
    nc.assert_bits(no_sigma[0], full[0], "sigma_in NULL: colour")
    nc.assert_bits(no_sigma[2], full[2], "sigma_in NULL: scale_out")
    no_scale = clamp(rgba, sigma, p, scale_out=None)
    nc.assert_bits(no_scale[0], full[0], "scale_out NULL: colour")
    nc.assert_bits(no_scale[1], full[1], "scale_out NULL: sigma_out")
    only = clamp(rgba, sigma, p, sigma_out=None, scale_out=None)
    nc.assert_bits(only[0], full[0], "sigma_out and scale_out NULL: colour")
    nc.assert_bits(clamp(rgba, sigma, None)[0], clamp(rgba, sigma, rt_amd.firefly_default_params(hostsim=True))[0],
                   "params NULL: the defaults")


def test_argument_errors():
    rgba, sigma = inputs(5, 3)
    L, h = fc.ctx(True)
    ARG = rt_amd.RT_ERR_ARG

    def rc(p=None, **over):
        r = clamp(rgba, sigma, p if p is not None else params(), code=True, **over)
        assert r == 0 or L.rt_last_error(h)
        return r

    assert rc() == 0
    for v in (0, 3, -1):
        assert rc(params(radius=v)) == ARG and b"radius" in L.rt_last_error(h)
    for v in (0, 9, -2):
        assert rc(params(rank=v)) == ARG and b"rank" in L.rt_last_error(h)
    assert rc(params(1, 8)) == 0 and rc(params(2, 8)) == 0 and rc(params(2, 1)) == 0
    for v in (np.nan, -0.5, -np.inf):
        assert rc(params(gain=v)) == ARG and b"gain" in L.rt_last_error(h)
    assert rc(params(gain=0.0)) == 0 and rc(params(gain=np.inf)) == 0
    assert rc(params(floor=np.nan)) == ARG and b"floor" in L.rt_last_error(h)
    assert rc(params(floor=-1.0)) == 0 and rc(params(floor=np.inf)) == 0 and rc(params(floor=-np.inf)) == 0
    for kw in (dict(w=0), dict(h=0), dict(w=-3)):
        assert rc(**kw) == ARG and b"at least 1" in L.rt_last_error(h)
    assert rc(rgba_in=None) == ARG and rc(out=None) == ARG and b"NULL" in L.rt_last_error(h)
    assert rc(sigma_in=None, sigma_out=np.zeros((3, 5), f32)) == ARG and b"sigma_out" in L.rt_last_error(h)
    # an output that aliases an input or another output, by pointer and by overlap
    assert rc(out=rgba) == ARG and b"overlaps" in L.rt_last_error(h)
    assert rc(sigma_out=sigma) == ARG and rc(scale_out=sigma) == ARG
    assert rc(scale_out=rgba.reshape(-1)[8:23].reshape(3, 5)) == ARG
    both = np.zeros((2, 3, 5), f32)
    assert rc(sigma_out=both[0], scale_out=both[0]) == ARG and b"outputs" in L.rt_last_error(h)
    assert rc(sigma_out=both[0], scale_out=both[1]) == 0
    big = np.zeros(16 * 15 + 8, np.uint8)
    assert rc(rgba_in=big[:240].view(f32).reshape(3, 5, 4), out=big[8:248].view(f32).reshape(3, 5, 4)) == ARG
    flat = np.zeros(15 + 14, f32)
    assert rc(sigma_out=flat[:15].reshape(3, 5), scale_out=flat[14:].reshape(3, 5)) == ARG
    # rt_denoise's frame-size limits
    tall4, tall1 = np.zeros((262141, 1, 4), f32), np.zeros((262141, 1), f32)
    p = params()
    assert L.rt_firefly(h, 1, 262141, ptr(tall4), ptr(tall1), ctypes.byref(p), ptr(tall4.copy()), None, None) == ARG
    assert b"262140" in L.rt_last_error(h)
    assert L.rt_firefly(h, 1 << 14, 1 << 13, ptr(tall4), None, ctypes.byref(p), ptr(tall4.copy()), None, None) == ARG
    assert b"too many pixels" in L.rt_last_error(h)
    # the device form's alignment rules
    odd4 = np.zeros(16 * 15 + 16, np.uint8)[4:]
    odd1 = np.zeros(4 * 15 + 8, np.uint8)[1:]
    o4, o1, o2 = np.zeros((3, 5, 4), f32), np.zeros((3, 5), f32), np.zeros((3, 5), f32)

    def dev(i=rgba, s=sigma, o=o4, so=o1, fo=o2):
        return L.rt_firefly_device(h, 5, 3, ptr(i), ptr(s), ctypes.byref(p), ptr(o), ptr(so), ptr(fo), None)

    assert dev() == 0, L.rt_last_error(h)
    for kw in (dict(i=odd4), dict(s=odd1), dict(o=odd4), dict(so=odd1), dict(fo=odd1)):
        assert dev(**kw) == ARG and b"aligned" in L.rt_last_error(h), kw
    assert L.rt_firefly(None, 5, 3, ptr(rgba), ptr(sigma), None, ptr(o4), ptr(o1), ptr(o2)) == ARG
    d = rt_amd.firefly_default_params(hostsim=True)
    assert (d.radius, d.rank, d.gain, d.floor) == (1, 2, 2.0, 0.0)
    assert L.rt_test_schedule(h, b"ff_variant", 2.0) == 0 and L.rt_test_schedule(h, b"ff_variant", 0.0) == 0


def test_multi_device_context_runs_the_stage():
    m = nc.Session(True, name="firefly-multi", devices=[0, 1])
    rgba, sigma = inputs(37, 29)
    out, s, f = (np.empty((29, 37, 4), f32), np.empty((29, 37), f32), np.empty((29, 37), f32))
    p = params(2, 2, 1.0, 0.01)
    m.ok(m.L.rt_firefly(m.ctx, 37, 29, ptr(rgba), ptr(sigma), ctypes.byref(p), ptr(out), ptr(s), ptr(f)), "rt_firefly")
    for g, w, name in zip((out, s, f), fc.host_result(37, 29, 2, 2), ("colour", "sigma_out", "scale_out")):
        nc.assert_bits(g, w, f"multi-device context: {name}")
    m.close()


# ------------------------------------------------------------------ quality
def test_quality_sweep_and_defaults(cameras, manifest):
    """Cornell 64x64, the cornell32 camera, 8 bounces: the 4-sample frame of a tracked [2, 2] progression and its
    noise_sigma, against a 256-sample linear render, RMSE over rgb. The sweep of DESIGN.md §16 is printed (pytest -s);
    the two inequalities are asserted at the default parameters. Measured on the hostsim build at the defaults (radius
    1, rank 2, gain 2, floor 0): raw 2.094, clamped 1.578; rt_denoise_var of the raw frame 1.552, of the clamped one
    1.537. What is left sits on the light's edge, whose pixels are as bright as a firefly and have bright neighbours.
    On the 256-sample frame itself the defaults clamp 0.88 % of the pixels and change the mean luminance by -0.80 %.
    One scene at one size."""
    rk, lin, sigma, ref = fc.quality_frames(cameras, manifest)
    with np.errstate(all="ignore"):
        raw, raw_dn = dv.rmse(lin.pixels, ref), dv.rmse(rk.denoise_var(lin, sigma).pixels, ref)
        print(f"firefly quality: raw {raw:.5f} denoise_var(raw) {raw_dn:.5f}")
        for radius in (1, 2):
            for rank in (1, 2, 3):
                for gain in (1.0, 1.5, 2.0, 4.0):
                    c, s, f = rk.firefly_clamp(lin, sigma, params(radius, rank, gain, 0.0), return_scale=True)
                    print(f"firefly sweep R {radius} rank {rank} gain {gain}: clamped {dv.rmse(c.pixels, ref):.5f} "
                          f"denoise_var(clamped) {dv.rmse(rk.denoise_var(c, s).pixels, ref):.5f} share {(f < 1).mean():.4f}")
        c, s = rk.firefly_clamp(lin, sigma)
        r_c, r_dn = dv.rmse(c.pixels, ref), dv.rmse(rk.denoise_var(c, s).pixels, ref)
    # the bias of the defaults on the converged frame: recorded, not asserted
    conv = rt_amd.Image(64, 64, pixels=np.concatenate([ref, np.ones((64, 64, 1))], -1))
    cc, _, cf = rk.firefly_clamp(conv, None, return_scale=True)
    l0, l1 = fc.luminance(conv.pixels[..., :3]).mean(), fc.luminance(cc.pixels[..., :3]).mean()
    print(f"firefly defaults: clamped {r_c:.5f} denoise_var(clamped) {r_dn:.5f}; on the 256-sample frame "
          f"{(cf < 1).mean() * 100:.2f} % of the pixels clamped, mean luminance {100 * (l1 - l0) / l0:+.2f} %")
    assert r_c < raw
    assert r_dn < raw_dn
