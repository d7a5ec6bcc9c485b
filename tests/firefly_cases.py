"""Firefly rejection (rt_firefly; include/rt_hip.h). The reference is model(): the header comment restated in
numpy float64, never calling the library.

Inputs are synthetic, so no scene is bound: a smooth gradient (0.2 .. 0.8 per channel) plus white noise of
amplitude 0.1 in the colour, a sigma of 0.05 .. 0.5, and planted patterns at fixed positions. A bright pixel is
BRIGHT * (1 + 0.05 u), u the pixel's own uniform draw, so that no two bright pixels tie. Frames of at least
37 x 29 pixels (x, y; w1 = w - 1, h1 = h - 1):
  lone spikes        interior (10, 8); edges (18, 0), (18, h1), (0, 14), (w1, 14); corners (0, 0), (w1, 0),
                     (0, h1), (w1, h1)
  pairs              horizontal (5, 4) (6, 4); diagonal (14, 4) (15, 5)
  2x2 cluster        (22, 4) .. (23, 5)
  line               one pixel wide, y = 12, x = 4 .. 16
  bar                two pixels thick, y = 17 and 18, x = 4 .. 16
  bad colours        NaN at (26, 10), +inf at (28, 10), negative at (30, 10); the spike (27, 11) has the first
                     two among its neighbours and the spike (31, 10) the third
  bad sigmas         NaN at (10, 8) and +inf at (5, 4), both clamped pixels; NaN at (2, 21) and +inf at (3, 21), untouched ones
5 x 3: spikes at (2, 1) and (0, 0), a NaN colour at (4, 2), a negative colour at (4, 0), a +inf sigma at (2, 1) and a NaN
sigma at (1, 2). 1 x 1: one spike, no neighbour.

Shared by tests/test_firefly.py (hostsim), tests/test_firefly_gpu.py (gfx950) and tests/test_firefly_shim.py.
Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import rt_amd
from rt_amd import FireflyParams, ptr

f32 = np.float32
FMAX = float(np.finfo(np.float32).max)
SHAPES = [(1, 1), (5, 3), (37, 29), (130, 67)]
BRIGHT = 50.0
SEED = 7
NEAR = 1e-5      # a pixel whose model luminance is within this relative distance of its limit is left out ...
NEAR_CAP = 0.02  # ... and at most this share of a case's pixels may be
W709 = tuple(float(f32(v)) for v in (0.2126, 0.7152, 0.0722))  # the header's float constants

# |hostsim - float64 model| over SHAPES x radius {1, 2} x rank {1, 2, 3, 8} x gain {1, 2} x floor {0, 0.1}, largest over
# the compared pixels, as |got - want| / max(1, want) for colour, sigma_out and scale_out. Measured on the hostsim build;
# the bound is 4x the measurement. The figure is float32 rounding: L(c) has three rounded products and two rounded sums,
# limit two more operations, f the division and the output one product: some 8 roundings of up to 2^-24 = 6e-8 each,
# about half of which the measured figures show.
COLOR_MEASURED = 2.31e-7  # 130x67, radius 2, rank 8, gain 1, floor 0
SIGMA_MEASURED = 9.10e-8  # 130x67, radius 1, rank 3, gain 1, floor 0
SCALE_MEASURED = 2.63e-7  # 130x67, radius 2, rank 8, gain 1, floor 0
COLOR_TOL = 4 * COLOR_MEASURED
SIGMA_TOL = 4 * SIGMA_MEASURED
SCALE_TOL = 4 * SCALE_MEASURED

LONE, PAIR_H, PAIR_D = (10, 8), ((5, 4), (6, 4)), ((14, 4), (15, 5))
CLUSTER = tuple((x, y) for y in (4, 5) for x in (22, 23))
LINE = tuple((x, 12) for x in range(4, 17))
BAR = tuple((x, y) for y in (17, 18) for x in range(4, 17))


def params(radius=1, rank=2, gain=2.0, floor=0.0):
    return FireflyParams(radius, rank, gain, floor)


def inputs(w, h, seed=SEED):
    """(rgba [h, w, 4], sigma [h, w]) float32 of one case."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w) / max(w - 1, 1), np.arange(h) / max(h - 1, 1))
    rgba = np.empty((h, w, 4), f32)
    rgba[..., 0] = 0.2 + 0.6 * x
    rgba[..., 1] = 0.2 + 0.6 * y
    rgba[..., 2] = 0.8 - 0.3 * (x + y)
    rgba[..., :3] += (0.1 * rng.random((h, w, 3))).astype(f32)
    rgba[..., 3] = rng.random((h, w)).astype(f32)  # (alpha is copied, whatever it holds)
    sigma = (0.05 + 0.45 * rng.random((h, w))).astype(f32)
    u = rng.random((h, w))

    def bright(px):
        for (bx, by) in px:
            rgba[by, bx, :3] = f32(BRIGHT * (1 + 0.05 * u[by, bx]))

    if w >= 37 and h >= 29:
        w1, h1 = w - 1, h - 1
        bright([LONE, (18, 0), (18, h1), (0, 14), (w1, 14), (0, 0), (w1, 0), (0, h1), (w1, h1), *PAIR_H, *PAIR_D, *CLUSTER,
                *LINE, *BAR, (27, 11), (31, 10)])
        rgba[10, 26, 1] = np.nan
        rgba[10, 28, 2] = np.inf
        rgba[10, 30, :3] = (-0.5, -0.4, -0.6)
        sigma[8, 10], sigma[4, 5], sigma[21, 2], sigma[21, 3] = np.nan, np.inf, np.nan, np.inf
    elif (w, h) == (5, 3):
        bright([(2, 1), (0, 0)])
        rgba[2, 4, 0] = np.nan
        rgba[0, 4, :3] = (-0.5, -0.4, -0.6)
        sigma[1, 2], sigma[2, 1] = np.inf, np.nan
    else:
        bright([(0, 0)])
    return rgba, sigma


# ------------------------------------------------------------------ the reference (numpy float64)
def luminance(rgb):
    c = rgb.astype(np.float64)
    with np.errstate(all="ignore"):
        return (W709[0] * c[..., 0] + W709[1] * c[..., 1]) + W709[2] * c[..., 2]


def model(rgba, sigma, p):
    """(rgba_out [h, w, 4], sigma_out [h, w] or None, scale_out [h, w], near [h, w] bool) in float64: near marks the
    pixels whose luminance is within NEAR (relative) of their limit, or whose limit is within 1e-7 of zero."""
    h, w = rgba.shape[:2]
    R, rank, gain, floor = p.radius, p.rank, float(f32(p.gain)), float(f32(p.floor))
    c = rgba[..., :3].astype(np.float64)
    fin = np.isfinite(c).all(-1)
    L = luminance(c)
    val = np.where(fin, np.maximum(np.where(fin, L, 0.0), -FMAX), -np.inf)
    pad = np.full((h + 2 * R, w + 2 * R), -np.inf)
    pad[R:R + h, R:R + w] = val
    taps = [pad[R + dy:R + dy + h, R + dx:R + dx + w] for dy in range(-R, R + 1) for dx in range(-R, R + 1)
            if (dx, dy) != (0, 0)]
    ranked = -np.sort(-np.stack(taps, -1), axis=-1)
    M = ranked[..., rank - 1] if rank <= len(taps) else np.full((h, w), -np.inf)
    have = M > -np.inf
    with np.errstate(all="ignore"):
        limit = gain * np.where(have, M, 0.0) + floor
        clamp = have & fin & (limit > 0) & (L > limit)
        near = have & fin & ((np.abs(L - limit) <= NEAR * np.abs(limit)) | (np.abs(limit) < 1e-7))
        f = np.where(clamp, limit / np.where(clamp, L, 1.0), 1.0)
        out = rgba.astype(np.float64)
        out[..., :3] = np.where(clamp[..., None], f[..., None] * c, c)
        s_out = None
        if sigma is not None:
            s = sigma.astype(np.float64)
            s_out = np.where(clamp & np.isfinite(s), f * s, s)
    return out, s_out, f, near


def model_errors(got, want):
    """(colour, sigma_out, scale_out) errors over the pixels not in `near`, as the *_TOL measure them; NaN and
    infinite values must match exactly and are left out of the figure."""
    keep = ~want[3]
    errs = []
    for g, x in zip(got, want[:3]):
        if g is None:
            errs.append(0.0)
            continue
        k = keep if g.ndim == 2 else keep[..., None] & np.ones(g.shape, bool)
        fin = np.isfinite(x)
        assert np.array_equal(np.isnan(g[k]), np.isnan(x[k])) and np.array_equal(np.isinf(g[k]), np.isinf(x[k]))
        xs = np.where(fin, x, 0.0)
        e = np.where(fin, np.abs(np.where(fin, g, 0.0).astype(np.float64) - xs) / np.maximum(1.0, xs), 0.0)
        errs.append(float(e[k].max(initial=0.0)))
    return tuple(errs)


# ------------------------------------------------------------------ the calls
_ctx = {}


def ctx(hostsim=True):
    """One bare context per library: the stage needs neither a scene nor a camera."""
    if hostsim not in _ctx:
        L = rt_amd.lib(hostsim)
        hnd = ctypes.c_void_p()
        rt_amd.check(L, L.rt_create(0, ctypes.byref(hnd)), None, "rt_create")
        _ctx[hostsim] = (L, hnd)
    return _ctx[hostsim]


def clamp(rgba, sigma, p=None, hostsim=True, code=False, **over):
    """(rgba_out, sigma_out, scale_out) of rt_firefly, or its return code. over: replacements for the call's
    arguments by name (rgba_in, sigma_in, out, sigma_out, scale_out, w, h); sigma_out follows sigma unless replaced."""
    L, hnd = ctx(hostsim)
    H, W = rgba.shape[:2]
    a = dict(rgba_in=rgba, sigma_in=sigma, w=W, h=H, out=np.full((H, W, 4), -5.0, f32),
             sigma_out=None if sigma is None else np.full((H, W), -5.0, f32), scale_out=np.full((H, W), -5.0, f32))
    a.update(over)
    rc = L.rt_firefly(hnd, a["w"], a["h"], ptr(a["rgba_in"]), ptr(a["sigma_in"]), ctypes.byref(p) if p is not None else None,
                      ptr(a["out"]), ptr(a["sigma_out"]), ptr(a["scale_out"]))
    if code:
        return rc
    rt_amd.check(L, rc, hnd, "rt_firefly")
    return a["out"], a["sigma_out"], a["scale_out"]


_host_cache = {}


def host_result(w, h, radius, rank, gain=1.0, floor=0.01):
    """hostsim's three outputs for a synthetic case, computed once and shared (read-only)."""
    key = (w, h, radius, rank, gain, floor)
    if key not in _host_cache:
        got = clamp(*inputs(w, h), params(radius, rank, gain, floor))
        for a in got:
            a.setflags(write=False)
        _host_cache[key] = got
    return _host_cache[key]


# ------------------------------------------------------------------ the 4-sample Cornell frame of DESIGN.md §16
_quality = {}


def quality_frames(cameras, manifest):
    """Cornell 64x64, the cornell32 camera, 8 bounces, on the hostsim build: (kernel, 4-sample linear Image of a tracked
    [2, 2] progression declared at 64 samples, its noise_sigma, the 256-sample linear render's rgb in float64)."""
    if not _quality:
        import dnv_cases as dv
        import temporal_cases as tc
        rk, fb = dv.cornell_kernel(cameras, manifest, True, 64, 64, 256, 8)
        lin, sigma = tc.recipe_frame(rk, 0, 64, 4, 64, 64)
        rk.render_linear()
        _quality["v"] = (rk, lin, sigma, fb.pixels[..., :3].astype(np.float64).copy())
    return _quality["v"]
