"""The variance-guided à-trous filter and the absolute noise figure on the hostsim build
(rt_denoise_var, rt_progress_noise_sigma; include/rt_hip.h): the filter against dnv_cases.model(), a
float64 restatement of the header comment; the query against a numpy float32 restatement, bit for
bit; the exact properties and argument errors; the quality figures of DESIGN.md §14; the CLI flag."""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import adapt_cases as ac
import dnv_cases as dv
import noise_cases as nc
import progress_cases as pc
import rt_amd
import scenes
from dnv_cases import HK, SIZES, denoise_var, inputs, params
from rt_amd import ptr


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("guides", [True, False])
@pytest.mark.parametrize("passes", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("w,h", SIZES)
def test_hostsim_matches_float64_model(w, h, passes, guides):
    rgba, sigma, alb, nd = inputs(w, h)
    got = dv.host_result(w, h, passes, guides)
    want = dv.model(rgba, sigma, alb if guides else None, nd if guides else None, params(passes), 1.0)
    ec, es = dv.model_errors(got, want)
    print(f"denoise_var model {w}x{h} passes {passes} guides {guides}: colour {ec:.3e} sigma_out {es:.3e}")
    assert dv.COLOR_TOL <= 1e-4
    assert ec <= dv.COLOR_TOL
    assert es <= dv.SIGMA_TOL
    assert np.all(got[0][..., 3] == 1.0)


def test_sigma_out_is_optional_and_changes_nothing():
    rgba, sigma, alb, nd = inputs(37, 29)
    out, _ = denoise_var(rgba, sigma, alb, nd, params(3), 1.0, sigma_out=False)
    nc.assert_bits(out, dv.host_result(37, 29, 3, True)[0], "rgba_out without sigma_out")


# ------------------------------------------------------------------ the sigma query
@pytest.mark.parametrize("which", ["ordinary", "edge"])
@pytest.mark.parametrize("halves", nc.HALVES)
@pytest.mark.parametrize("shape", nc.SHAPES)
def test_noise_sigma_on_injected_states(shape, halves, which):
    """noise_cases' injected states as version-2 checkpoints: s against the restatement, bit for bit, both
    forms; pixel_err == s / sqrt(0.01 + sum m) wherever both are finite."""
    w, h = shape
    n_a, n_b = halves
    s = pc.session(True, "cornell")
    base, state, half = nc.ordinary(w, h, n_a, n_b) if which == "ordinary" else nc.edges(w, h, n_a, n_b)
    blob = nc.pack_v2(base, state, half, total=n_a + n_b + 2, done=n_a + n_b, passes=2, n_a=n_a)
    assert pc.load_rc(s, blob) == 0, s.error()
    th, tw = (h + 7) // 8, (w + 7) // 8
    want, root = dv.sigma_restate(state, half, np.full((th, tw), n_a + n_b), np.full((th, tw), n_a))
    got = dv.noise_sigma(s)
    nc.assert_bits(got, want, f"{w}x{h} {halves} {which}")
    nc.assert_bits(dv.noise_sigma(s, device=True), want, f"{w}x{h} {halves} {which} device form")
    px = nc.noise(s)[0]
    both = np.isfinite(px) & np.isfinite(got)
    with np.errstate(all="ignore"):
        nc.assert_bits(px[both], (got / root)[both], "pixel_err == s / sqrt(0.01 + sum m)")
    assert pc.save(s) == blob, "the query changed the state"
    s.close()


def test_noise_sigma_with_unequal_tile_counts():
    dv.case_sigma_uneven(True)


def test_noise_sigma_errors():
    s = pc.session(True, "cornell")
    out = np.zeros((pc.H, pc.W), np.float32)
    L = s.L
    assert L.rt_progress_noise_sigma(None, ptr(out)) == rt_amd.RT_ERR_ARG
    assert L.rt_progress_noise_sigma(s.ctx, ptr(out)) == rt_amd.RT_ERR_STATE, "no progression"
    pc.begin(s)
    pc.advance(s, 1)
    assert L.rt_progress_noise_sigma(s.ctx, ptr(out)) == rt_amd.RT_ERR_STATE and "tracked" in s.error()
    pc.begin(s)
    nc.track(s)
    pc.advance(s, 2)
    assert L.rt_progress_noise_sigma(s.ctx, ptr(out)) == rt_amd.RT_ERR_STATE and "both halves" in s.error()
    assert L.rt_progress_noise_sigma_device(s.ctx, ptr(out), None) == rt_amd.RT_ERR_STATE
    pc.advance(s, 1)
    assert L.rt_progress_noise_sigma(s.ctx, ptr(out)) == 0, s.error()
    assert L.rt_progress_noise_sigma(s.ctx, None) == rt_amd.RT_ERR_ARG and "NULL" in s.error()
    assert L.rt_progress_noise_sigma_device(s.ctx, None, None) == rt_amd.RT_ERR_ARG
    odd = np.zeros(4 * pc.W * pc.H + 8, np.uint8)[1:]
    assert L.rt_progress_noise_sigma_device(s.ctx, ptr(odd), None) == rt_amd.RT_ERR_ARG and "aligned" in s.error()
    s.close()
    m = nc.Session(True, name="dnv-multi", devices=[0, 1])
    pc.bind(m, "cornell")
    assert m.L.rt_progress_noise_sigma(m.ctx, ptr(out)) == rt_amd.RT_ERR_STATE, "a multi-device context has no progression"
    m.close()


# ------------------------------------------------------------------ exact properties
def test_blend_zero_returns_input_bitwise():
    rgba, sigma, alb, nd = inputs(37, 29)
    out, _ = denoise_var(rgba, sigma, alb, nd, params(3), 0.0)
    np.testing.assert_array_equal(out[..., :3].view(np.uint32), rgba[..., :3].view(np.uint32))
    assert np.all(out[..., 3] == 1.0)


def test_huge_sigma_color_is_the_b3_spline_blur_with_squared_weights():
    """Guides off and sigma_color 1e18: every e is 0 (or rounds to it), so a pass is the B3-spline blur over
    the taps inside the image and sigma_out follows v' = sum k^2 v / (sum k)^2."""
    rgba, sigma, _, _ = inputs(37, 29)
    sigma = np.where(np.isfinite(sigma), sigma, np.float32(0.25)).astype(np.float32)
    out, left = denoise_var(rgba, sigma, None, None, params(1, 1e18), 1.0)
    c, v = rgba[..., :3].astype(np.float64), sigma.astype(np.float64) ** 2
    h, w = v.shape
    num, den, numv = np.zeros_like(c), np.zeros((h, w)), np.zeros((h, w))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            k = HK[dy + 2] * HK[dx + 2]
            for y in range(max(0, -dy), min(h, h - dy)):
                xs = np.arange(max(0, -dx), min(w, w - dx))
                num[y, xs] += k * c[y + dy, xs + dx]
                numv[y, xs] += k * k * v[y + dy, xs + dx]
                den[y, xs] += k
    assert np.abs(out[..., :3] - num / den[..., None]).max() <= dv.COLOR_TOL
    assert np.abs(left - np.sqrt(numv / den ** 2)).max() <= dv.SIGMA_TOL


@pytest.mark.parametrize("guides", [True, False])
def test_constant_image_comes_back_constant(guides):
    """Every colour distance is 0, so whatever the sigma map (its NaN and +inf included) the output is a
    weighted mean of one value. The weights do not sum to 1 in float32, so the quotient may be an ulp off."""
    rgba, sigma, alb, nd = inputs(37, 29)
    rgba[..., :3] = (0.25, 0.5, 0.75)  # (exact in float32, as are their products with the kernel's weights)
    out, left = denoise_var(rgba, sigma, alb if guides else None, nd if guides else None, params(5), 1.0)
    assert np.abs(out[..., :3] - np.asarray([0.25, 0.5, 0.75], np.float32)).max() <= 2 ** -22
    assert np.isfinite(left).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_pixel_stays_alone(bad):
    rgba, sigma, alb, nd = inputs(37, 29)
    rgba[10, 12, 1] = bad
    out, left = denoise_var(rgba, sigma, alb, nd, params(5), 1.0)
    nf = ~np.isfinite(out[..., :3]).all(-1)
    assert nf.sum() == 1 and nf[10, 12]
    assert np.isfinite(left).all()
    v = np.float32(sigma[10, 12]) * np.float32(sigma[10, 12])
    assert left[10, 12] == np.sqrt(v), "a centre that is not finite keeps its record, v included"


def test_nan_guide_gets_no_weight():
    rgba, sigma, alb, nd = inputs(37, 29)
    clean, _ = denoise_var(rgba, sigma, alb, nd, params(2), 1.0)
    nd2 = nd.copy()
    nd2[10, 12, 0] = np.nan
    out, left = denoise_var(rgba, sigma, alb, nd2, params(2), 1.0)
    assert np.isfinite(out).all() and np.isfinite(left).all()
    np.testing.assert_array_equal(out[10, 12, :3].view(np.uint32), rgba[10, 12, :3].view(np.uint32))
    far = np.ones((29, 37), bool)
    far[max(0, 10 - 6):10 + 7, max(0, 12 - 6):12 + 7] = False  # reach of 2 passes: 2 * (1 + 2)
    np.testing.assert_array_equal(out[far].view(np.uint32), clean[far].view(np.uint32))
    assert (out != clean).any()


def test_finite_input_never_gives_nan():
    """Colours up to 1e19 (distances that overflow float32) beside a +inf sigma (r_p = 0 once the floor is added
    to the largest float): 0 x inf is a NaN e, which is a skipped tap, never a NaN colour."""
    rgba, sigma, alb, nd = inputs(37, 29)
    rgba[::3, ::2, :3] *= np.float32(1e19)
    sigma[5:9, 5:9] = np.inf
    out, left = denoise_var(rgba, sigma, alb, nd, params(5, floor=3e38), 1.0)
    assert not np.isnan(out).any() and np.isfinite(left).all()


def test_argument_errors():
    rgba, sigma, alb, nd = inputs(5, 3)
    L, h = dv.ctx(True)

    def rc(p=None, blend=1.0, a=alb, n=nd, s=sigma):
        r = denoise_var(rgba, s, a, n, p if p is not None else params(), blend, code=True)
        assert r == 0 or L.rt_last_error(h)
        return r

    assert rc() == 0
    assert L.rt_denoise_var(h, 5, 3, ptr(rgba), ptr(sigma), None, None, None, ctypes.c_float(1.0),
                            ptr(np.zeros_like(rgba)), None) == 0, "params NULL, guides NULL, sigma_out NULL"
    for passes in (0, 11, -1):
        assert rc(params(passes)) == rt_amd.RT_ERR_ARG
    for bad in (0.0, -1.0, np.nan, np.inf):
        for k in range(5):
            s = [2.0, 0.3, 0.1, 0.1, 1e-4]
            s[k] = bad
            assert rc(params(3, *s)) == rt_amd.RT_ERR_ARG, (bad, k)
    assert b"var_floor" in L.rt_last_error(h)
    for blend in (np.nan, np.inf, -np.inf):
        assert rc(blend=blend) == rt_amd.RT_ERR_ARG
    assert rc(a=None) == rt_amd.RT_ERR_ARG
    assert rc(n=None) == rt_amd.RT_ERR_ARG
    assert rc(s=None) == rt_amd.RT_ERR_ARG and b"sigma is NULL" in L.rt_last_error(h)
    assert L.rt_denoise_var(h, 5, 3, ptr(rgba), ptr(sigma), None, None, None, ctypes.c_float(1.0), ptr(rgba),
                            None) == rt_amd.RT_ERR_ARG, "rgba_in == rgba_out"
    assert L.rt_denoise_var(None, 5, 3, ptr(rgba), ptr(sigma), None, None, None, ctypes.c_float(1.0),
                            ptr(np.zeros_like(rgba)), None) == rt_amd.RT_ERR_ARG
    tall = np.zeros((262141, 1, 4), np.float32)
    assert L.rt_denoise_var(h, 1, 262141, ptr(tall), ptr(np.zeros((262141, 1), np.float32)), None, None, None,
                            ctypes.c_float(1.0), ptr(np.zeros_like(tall)), None) == rt_amd.RT_ERR_ARG
    assert b"262140" in L.rt_last_error(h)
    odd = np.zeros(4 * 15 + 8, np.uint8)[1:]
    p = params()
    assert L.rt_denoise_var_device(h, 5, 3, ptr(rgba), ptr(odd), None, None, ctypes.byref(p), ctypes.c_float(1.0),
                                   ptr(np.zeros_like(rgba)), None, None) == rt_amd.RT_ERR_ARG
    assert b"aligned" in L.rt_last_error(h)
    d = rt_amd.denoise_var_default_params(hostsim=True)
    assert 1 <= d.passes <= 10 and min(d.sigma_color, d.sigma_normal, d.sigma_albedo, d.sigma_depth, d.var_floor) > 0


# ------------------------------------------------------------------ quality
def test_quality_filtered_is_closer_to_converged(cameras, manifest):
    """Cornell 64x64, 8 bounces, linear frames against 512 spp: frame U (uniform, [8, 8]) and frame A (adaptive,
    64 in passes of 8, threshold = the median tile error after the second pass), filtered at the defaults with
    each frame's own noise figure. Measured on the hostsim build (DESIGN.md §14 has the sweep):
    """
    rk, fb = dv.cornell_kernel(cameras, manifest, True, 64, 64, 512, 8)
    rk.render_linear()
    ref = fb.pixels[..., :3].astype(np.float64)
    for name, frame in (("U", dv.frame_uniform), ("A", dv.frame_adaptive)):
        k, lin, sigma, tile_n = frame(cameras, manifest)
        if name == "A":
            assert tile_n.min() < tile_n.max(), "the adaptive frame's tile counts differ"
        with np.errstate(all="ignore"):
            var = k.denoise_var(lin, sigma)
            fixed = k.denoise(lin)
        r_in, r_var, r_fixed = dv.rmse(lin.pixels, ref), dv.rmse(var.pixels, ref), dv.rmse(fixed.pixels, ref)
        print(f"frame {name}: tile_n {tile_n.min()}..{tile_n.max()} rmse input {r_in:.5f} denoise_var {r_var:.5f} "
              f"rt_denoise {r_fixed:.5f}")
        assert r_var < r_in
        k.progress_end()


def test_python_denoise_var_takes_the_live_progressions_sigma(cameras, manifest):
    k, lin, sigma, _ = dv.frame_uniform(cameras, manifest, W=24, H=20, bounces=3, split=(2, 2))
    alb, nd = k.features()
    want, left = denoise_var(lin.pixels, sigma, alb, nd, None, 0.75)
    got, got_left = k.denoise_var(lin, blend_factor=0.75, return_sigma=True)
    nc.assert_bits(got.pixels, want, "RenderKernel.denoise_var(sigma=None) vs the C ABI")
    nc.assert_bits(got_left, left, "sigma_out")
    nc.assert_bits(k.denoise_var(lin, sigma, 0.75, guides=(alb, nd), params={"passes": 3}).pixels, want, "explicit arguments")
    with pytest.raises(TypeError):
        k.denoise_var(lin, sigma, params={"sigma": 1.0})
    k.progress_end()
    with pytest.raises(rt_amd.RtError):
        k.denoise_var(lin)


# ------------------------------------------------------------------ CLI
def _cli(tmp_path, out, *flags):
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(rt_amd.__file__)))
    return subprocess.run([sys.executable, "-m", "rt_amd.cli", scenes.scene_path("cornell12"), f"--sky={hdr}", "--w=16",
                           "--h=12", "--samples=4", "--bounces=2", "--hostsim", "--camera=cornell", f"--out={out}", *flags],
                          capture_output=True, text=True, env=env)


def test_cli_denoise_var(tmp_path):
    r = _cli(tmp_path, tmp_path / "bad", "--denoise=var")
    assert r.returncode == 2 and "--noise-threshold" in r.stderr
    prog = ("--preview-every=1", "--noise-threshold=0")
    plain, var = tmp_path / "plain", tmp_path / "var"
    for out, flags in ((plain, prog), (var, prog + ("--denoise=var",))):
        r = _cli(tmp_path, out, *flags)
        assert r.returncode == 0, r.stdout + r.stderr
    # the render is the same image; the denoised ones come from the other filter
    assert (plain / "RT_output.png").read_bytes() == (var / "RT_output.png").read_bytes()
    assert (plain / "RT_output_denoised_1.png").read_bytes() != (var / "RT_output_denoised_1.png").read_bytes()
    for n in ("RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png"):
        assert (var / n).exists()
