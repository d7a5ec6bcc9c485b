"""The guided upscale stage on the hostsim build (rt_upscale; include/rt_hip.h): against upscale_cases.model(), a
float64 restatement of the header comment; the identity, the tiers' coverage, the argument errors, the Python front
end, the quality figure of DESIGN.md §18 and the command line's --upscale=F."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import dnv_cases as dv
import noise_cases as nc
import rt_amd
import scenes
import upscale_cases as uc
from rt_amd import cli, ptr
from upscale_cases import inputs, params, upscale

f32 = np.float32


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("sigma", [True, False])
@pytest.mark.parametrize("pair", uc.PAIRS)
def test_hostsim_matches_float64_model(pair, sigma):
    """The bound is uc.tolerance(), per pixel, from the operation count. Measured on the hostsim build
    with the seed of upscale_cases.py, largest over the 14 cases: colour 5.28e-6 ((37, 29) -> (130, 67)), at most 0.050
    of the pixel's bound ((33, 1) -> (257, 1)); sigma_out 2.7e-7 where the weights are normal floats and 0.227 at the
    tier-2 pixels whose weights lie below 1e-19, where sum wgt (wgt v) is denormal (rt_upscale.h) and the bound
    carries sqrt(32 * 2^-149) / S. 0 of the 52,908 pixel-cases lie near a threshold and are left out."""
    case = inputs(*pair)
    p = params()
    got = upscale(case, p, sigma)
    want = uc.model(case, p, sigma)
    ec, es, worst, left = uc.model_errors(got[0], got[1], want)
    tiers = [int((want["tier"] == k).sum()) for k in range(4)]
    print(f"upscale model {pair} sigma {sigma}: left out {left} ({want['near'].mean():.4f}) colour {ec:.3e} sigma_out {es:.3e} "
          f"error / bound {worst:.3e} tiers empty/1/2/3 {tiers}")
    assert want["near"].mean() <= uc.NEAR_CAP
    assert worst <= 1.0
    assert np.all(got[0][..., 3] == 1.0), "alpha is 1"
    assert (got[1] is None) == (not sigma)


def test_every_tier_and_the_empty_case_occur():
    count = np.zeros(4, int)
    for pair in uc.PAIRS:
        for sigma in (True, False):
            tier = uc.model(inputs(*pair), params(), sigma)["tier"]
            count += np.bincount(tier.reshape(-1), minlength=4)
    print("upscale tiers over the cases (empty, 1, 2, 3):", count.tolist())
    assert np.all(count >= 1), count
    # the empty case as the library reports it: black, alpha 1, an infinite sigma
    pair = (37, 29, 130, 67)
    tier = uc.model(inputs(*pair), params(), True)["tier"]
    out, s_out = uc.host_result(pair)
    assert (tier == 0).any()
    assert np.all(out[tier == 0] == (0.0, 0.0, 0.0, 1.0)) and np.all(np.isposinf(s_out[tier == 0]))


# ------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("sigma", [True, False])
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (130, 67)])
def test_identity_is_bit_exact(size, sigma):
    """w_lo == w, h_lo == h and the same guides: rgb and sigma pass through bit for bit on the finite pixels."""
    w, h = size
    case = dict(inputs(w, h, w, h))
    case["alb_hi"], case["nd_hi"] = case["alb_lo"], case["nd_lo"]
    out, s_out = upscale(case, None, sigma)
    ok = np.isfinite(case["rgba"][..., :3]).all(-1)
    if sigma:
        ok &= np.isfinite(case["sigma"])
    # (a NaN normal sends the pixel to tier 3, which is the pixel itself: it passes through as well)
    nc.assert_bits(out[ok][:, :3], case["rgba"][ok][:, :3], f"{size}: colour")
    if sigma:
        nc.assert_bits(s_out[ok], case["sigma"][ok], f"{size}: sigma")
    assert ok.sum() >= 0.8 * ok.size and np.all(out[..., 3] == 1.0)
    assert np.isfinite(out[~ok][:, :3]).all() or size == (1, 1), "a pixel that is not finite is rebuilt from its neighbours"


def test_inputs_are_left_alone_and_sigma_is_optional():
    pair = (37, 29, 130, 67)
    case = {k: v.copy() for k, v in inputs(*pair).items()}
    with_sigma = upscale(case, None, True)
    for k, v in inputs(*pair).items():
        nc.assert_bits(case[k], v, f"{k} changed")
    nc.assert_bits(with_sigma[0], uc.host_result(pair)[0], "a second call gives the same frame")
    # without a sigma the taps whose sigma is not finite count again: only elsewhere are the frames equal
    without = upscale(case, None, False)
    assert without[1] is None
    fin = np.isfinite(case["sigma"])
    assert not np.array_equal(without[0], with_sigma[0]) and fin.sum() < fin.size
    nc.assert_bits(upscale(case, rt_amd.upscale_default_params(hostsim=True), True)[0], with_sigma[0], "params NULL: the defaults")


def test_argument_errors():
    case = inputs(5, 3, 10, 6)
    L, h = uc.ctx(True)
    ARG = rt_amd.RT_ERR_ARG

    def rc(p=None, use_sigma=True, **over):
        r = upscale(case, p, use_sigma, code=True, **over)
        assert r == 0 or L.rt_last_error(h)
        return r

    assert rc() == 0 and rc(use_sigma=False) == 0 and rc(params()) == 0
    for k in ("rgba", "alb_lo", "nd_lo", "alb_hi", "nd_hi", "out"):
        assert rc(**{k: None}) == ARG and b"NULL" in L.rt_last_error(h), k
    assert rc(use_sigma=False, sigma_out=np.zeros((6, 10), f32)) == ARG and b"sigma_out without" in L.rt_last_error(h)
    assert rc(sigma_out=None) == ARG and b"sigma_lo without" in L.rt_last_error(h)
    for kw in (dict(w_lo=0), dict(h_lo=0), dict(w=0), dict(h=0), dict(w_lo=-2), dict(h=-1)):
        assert rc(**kw) == ARG and b"at least 1" in L.rt_last_error(h), kw
    assert rc(w_lo=11) == ARG and b"larger" in L.rt_last_error(h)
    assert rc(h_lo=7) == ARG and b"larger" in L.rt_last_error(h)
    for field in ("sigma_normal", "sigma_albedo", "sigma_depth"):
        for v in (0.0, -0.1, np.nan, np.inf):
            assert rc(params(**{field: v})) == ARG and b"positive and finite" in L.rt_last_error(h), (field, v)
    for v in (-0.1, 1.0, 1.5, np.nan):
        assert rc(params(min_weight=v)) == ARG and b"min_weight" in L.rt_last_error(h), v
    assert rc(params(min_weight=0.0)) == 0 and rc(params(min_weight=0.999)) == 0
    # an output that overlaps an input or the other output, by pointer and by range
    big = np.zeros((6, 10, 4), f32)
    assert rc(out=big, nd_hi=big) == ARG and b"overlaps" in L.rt_last_error(h)
    assert rc(out=big, alb_hi=big) == ARG and rc(out=big, alb_hi=big[::-1].copy()) == 0
    lo = np.zeros((6, 10, 4), f32)
    for k in ("rgba", "alb_lo", "nd_lo"):
        assert rc(out=lo, **{k: lo.reshape(-1)[60:120].reshape(3, 5, 4)}) == ARG and b"overlaps" in L.rt_last_error(h), k
    assert rc(sigma_out=lo.reshape(-1)[:60].reshape(6, 10), sigma=lo.reshape(-1)[56:71].reshape(3, 5)) == ARG
    assert rc(out=big, sigma_out=big.reshape(-1)[180:240].reshape(6, 10)) == ARG and b"outputs" in L.rt_last_error(h)
    # rt_denoise's frame-size limits, on the output
    one4, one1 = np.zeros((1, 1, 4), f32), np.zeros((1, 1), f32)
    tall = np.zeros((262141, 1, 4), f32)
    assert L.rt_upscale(h, 1, 1, 1, 262141, ptr(one4), None, ptr(one4), ptr(one4), ptr(tall), ptr(tall), None,
                        ptr(tall.copy()), None) == ARG and b"262140" in L.rt_last_error(h)
    assert L.rt_upscale(h, 1, 1, 1 << 14, 1 << 13, ptr(one4), None, ptr(one4), ptr(one4), ptr(tall), ptr(tall), None,
                        ptr(tall.copy()), None) == ARG and b"too many pixels" in L.rt_last_error(h)
    # the device form's alignment rules
    odd4 = lambda n: np.zeros(16 * n + 16, np.uint8)[4:]  # noqa: E731
    odd1 = lambda n: np.zeros(4 * n + 8, np.uint8)[1:]  # noqa: E731
    o4, o1 = np.zeros((6, 10, 4), f32), np.zeros((6, 10), f32)

    def dev(**kw):
        a = dict(case, out=o4, sigma_out=o1)
        a.update(kw)
        return L.rt_upscale_device(h, 5, 3, 10, 6, ptr(a["rgba"]), ptr(a["sigma"]), ptr(a["alb_lo"]), ptr(a["nd_lo"]),
                                   ptr(a["alb_hi"]), ptr(a["nd_hi"]), None, ptr(a["out"]), ptr(a["sigma_out"]), None)

    assert dev() == 0, L.rt_last_error(h)
    for k, n in (("rgba", 15), ("alb_lo", 15), ("nd_lo", 15), ("alb_hi", 60), ("nd_hi", 60), ("out", 60)):
        assert dev(**{k: odd4(n)}) == ARG and b"aligned" in L.rt_last_error(h), k
    assert dev(sigma=odd1(15)) == ARG and dev(sigma_out=odd1(60)) == ARG and b"aligned" in L.rt_last_error(h)
    assert L.rt_upscale(None, 5, 3, 10, 6, ptr(case["rgba"]), None, ptr(case["alb_lo"]), ptr(case["nd_lo"]),
                        ptr(case["alb_hi"]), ptr(case["nd_hi"]), None, ptr(o4), None) == ARG
    d = rt_amd.upscale_default_params(hostsim=True)
    dn = rt_amd.denoise_default_params(hostsim=True)
    assert (d.sigma_normal, d.sigma_albedo, d.sigma_depth) == (dn.sigma_normal, dn.sigma_albedo, dn.sigma_depth)
    assert d.min_weight == f32(0.1)
    assert L.rt_test_schedule(h, b"up_variant", 2.0) == 0 and L.rt_test_schedule(h, b"up_variant", 0.0) == 0


def test_multi_device_context_runs_the_stage():
    pair = (37, 29, 130, 67)
    case = inputs(*pair)
    m = nc.Session(True, name="upscale-multi", devices=[0, 1])
    out, s = np.empty((67, 130, 4), f32), np.empty((67, 130), f32)
    m.ok(m.L.rt_upscale(m.ctx, 37, 29, 130, 67, ptr(case["rgba"]), ptr(case["sigma"]), ptr(case["alb_lo"]), ptr(case["nd_lo"]),
                        ptr(case["alb_hi"]), ptr(case["nd_hi"]), None, ptr(out), ptr(s)), "rt_upscale")
    nc.assert_bits(out, uc.host_result(pair)[0], "multi-device context: colour")
    nc.assert_bits(s, uc.host_result(pair)[1], "multi-device context: sigma_out")
    m.close()


# ------------------------------------------------------------------ the Python front end and the quality figure
_frames = {}


def _cornell(cameras, manifest):
    """Cornell, the cornell32 camera, 8 bounces, on the hostsim build: the 64-sample linear render at 32x32 with its
    guides, the guides at 64x64 and the 256-sample linear render at 64x64 (rgb, float64)."""
    if not _frames:
        lo_k, lo_fb = dv.cornell_kernel(cameras, manifest, True, 32, 32, 64, 8)
        lo_k.render_linear()
        low = rt_amd.Image(32, 32, pixels=lo_fb.pixels.copy())
        hi_k, hi_fb = dv.cornell_kernel(cameras, manifest, True, 64, 64, 256, 8)
        hi_k.render_linear()
        _frames["v"] = (lo_k, low, lo_k.features(), lo_k.features(size=(64, 64)), hi_k.features(),
                        hi_fb.pixels[..., :3].astype(np.float64).copy())
    return _frames["v"]


def test_python_front_end_equals_c_calls(cameras, manifest):
    rk, low, (la, ln), (ha, hn), hi_own, _ = _cornell(cameras, manifest)
    nc.assert_bits(ha, hi_own[0], "features(size=) equals a 64x64 kernel's albedo")
    nc.assert_bits(hn, hi_own[1], "features(size=) equals a 64x64 kernel's normal_depth")
    sigma = (0.01 + 0.1 * np.random.default_rng(3).random((32, 32))).astype(f32)
    p = params(0.25, 0.2, 0.05, 0.2)
    for prm, cp in ((None, None), (p, p), (dict(sigma_normal=0.25, sigma_albedo=0.2, sigma_depth=0.05, min_weight=0.2), p)):
        for sg in (None, sigma):
            got = rk.upscale(low, la, ln, ha, hn, sigma=sg, params=prm)
            out, s_out = np.empty((64, 64, 4), f32), (None if sg is None else np.empty((64, 64), f32))
            rt_amd.check(rk.L, rk.L.rt_upscale(rk.ctx, 32, 32, 64, 64, ptr(low.pixels), ptr(sg), ptr(la), ptr(ln), ptr(ha), ptr(hn),
                                               ctypes.byref(cp) if cp is not None else None, ptr(out), ptr(s_out)), rk.ctx, "rt_upscale")
            if sg is None:
                nc.assert_bits(got.pixels, out, "upscale(): colour")
            else:
                nc.assert_bits(got[0].pixels, out, "upscale(sigma=): colour")
                nc.assert_bits(got[1], s_out, "upscale(sigma=): sigma_out")
    # the device form on the host build takes host pointers
    out = np.full((64, 64, 4), -1.0, f32)
    rk.upscale_device((32, 32), (64, 64), low.pixels.ctypes.data, la.ctypes.data, ln.ctypes.data, ha.ctypes.data, hn.ctypes.data,
                      out.ctypes.data)
    nc.assert_bits(out, rk.upscale(low, la, ln, ha, hn).pixels, "upscale_device")
    with pytest.raises(TypeError):
        rk.upscale(low, la, ln, ha, hn, params=dict(gain=1.0))


def test_quality_guided_beats_bilinear(cameras, manifest):
    """Cornell 64x64 from a 64-sample 32x32 linear render, RMSE over rgb against a 256-sample 64x64 linear render, on
    the hostsim build: rt_upscale at the defaults 1.69405; tier 3 forced everywhere (plain bilinear, upscale_cases'
    float64 model with force3) 2.81837 (the light's pixels carry most of either figure). One scene at one size; only
    the ordering is asserted."""
    rk, low, (la, ln), (ha, hn), _, ref = _cornell(cameras, manifest)
    guided = dv.rmse(rk.upscale(low, la, ln, ha, hn).pixels, ref)
    case = dict(rgba=low.pixels, sigma=None, alb_lo=la, nd_lo=ln, alb_hi=ha, nd_hi=hn)
    plain = uc.model(case, params(), sigma=False, force3=True)
    assert set(np.unique(plain["tier"])) <= {0, 3}
    bilinear = dv.rmse(plain["rgb"], ref)
    print(f"upscale quality: guided {guided:.5f} bilinear {bilinear:.5f}")
    assert guided < bilinear


# ------------------------------------------------------------------ the command line
def _cli(tmp_path, out, *flags, w=16, h=12):
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    return cli.main([scenes.scene_path("cornell12"), f"--sky={hdr}", f"--w={w}", f"--h={h}", "--samples=4", "--bounces=2",
                     "--hostsim", "--camera=cornell", f"--out={out}", *flags])


def _kernel(tmp_path, w, h):
    P = rt_amd.parse_obj(scenes.scene_path("cornell12"))
    hdr = rt_amd.read_image_float(str(tmp_path / "sky.hdr"))
    fb = rt_amd.Image(w, h)
    rk = rt_amd.RenderKernel(w, h, 4, 2, fb, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices, None,
                             rt_amd.BVH(P.triangles), hdr, rt_amd.compute_env_map_cdf(hdr), hostsim=True)
    rk.set_camera(rt_amd.Camera.preset("cornell"))
    return rk, fb


def _png(tmp_path, image):
    rt_amd.write_image_png(image, str(tmp_path / "want.png"))
    return (tmp_path / "want.png").read_bytes()


def test_cli_upscale(tmp_path, capsys):
    for bad in ("--upscale=1", "--upscale=4.5", "--upscale=0.5", "--upscale=nan"):
        assert _cli(tmp_path, tmp_path / "bad", bad) == 2
        assert "1 < F <= 4" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "bad")
    # 16 x 12 at F = 1.5: round(10.67) x round(8) = 11 x 8; at F = 2.5 on 15 x 9: round(6) x round(3.6) = 6 x 4
    for (w, h), f, lo in (((16, 12), 1.5, (11, 8)), ((15, 9), 2.5, (6, 4))):
        out = tmp_path / f"up_{f}"
        assert _cli(tmp_path, out, f"--upscale={f}", w=w, h=h) == 0
        assert f"upscale: {lo[0]}x{lo[1]} -> {w}x{h}" in capsys.readouterr().out
        rk, fb = _kernel(tmp_path, *lo)
        rk.render_linear()
        hi = rk.features(size=(w, h))
        full = rk.upscale(fb, *rk.features(), *hi)
        assert (full.width, full.height) == (w, h)
        shown = rk.display(full)
        assert (out / "RT_output.png").read_bytes() == _png(tmp_path, shown), "the frame equals the Python calls"
        with np.errstate(all="ignore"):
            dn = rk.denoise(shown, 1.0, hi)
        assert (out / "RT_output_denoised_1.png").read_bytes() == _png(tmp_path, dn)
    # with --denoise=var the filter runs at the low size and its result is upscaled too; metering at the full size
    out = tmp_path / "var"
    flags = ("--upscale=2", "--denoise=var", "--noise-threshold=0", "--preview-every=2", "--auto-exposure")
    assert _cli(tmp_path, out, *flags) == 0
    text = capsys.readouterr().out
    rk, fb = _kernel(tmp_path, 8, 6)
    rk.progress_begin()
    rk.progress_track_noise()
    rk.progress_advance(2)
    rk.progress_advance(2)
    rk.progress_resolve_linear(fb)
    with np.errstate(all="ignore"):
        filtered = rk.denoise_var(fb, None, 1.0)
    rk.progress_end()
    guides = (*rk.features(), *rk.features(size=(16, 12)))
    full, full_f = rk.upscale(fb, *guides), rk.upscale(filtered, *guides)
    e = rk.auto_exposure(full_f)
    assert f"auto-exposure: {e:.9g}" in text
    assert (out / "RT_output.png").read_bytes() == _png(tmp_path, rk.display(full, exposure=e))
    assert (out / "RT_output_denoised_1.png").read_bytes() == _png(tmp_path, rk.display(full_f, exposure=e))
    # without the flag: the run's bytes are render()'s, and no line is printed
    assert _cli(tmp_path, tmp_path / "plain") == 0
    assert "upscale:" not in capsys.readouterr().out
    rk, fb = _kernel(tmp_path, 16, 12)
    rk.render()
    assert (tmp_path / "plain" / "RT_output.png").read_bytes() == _png(tmp_path, fb)
    with np.errstate(all="ignore"):
        assert (tmp_path / "plain" / "RT_output_denoised_1.png").read_bytes() == _png(tmp_path, rk.denoise(fb, 1.0))
