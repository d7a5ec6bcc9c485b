"""The bloom stage (rt_bloom; include/rt_hip.h). The reference is model(): the header comment of rt_bloom.h restated
in numpy float64, never calling the library.

Inputs are synthetic, so no scene is bound: a smooth gradient (0.2 .. 0.8 per channel) plus white noise of amplitude
0.1 in the colour, a random alpha, and planted pixels at fixed positions. A bright pixel is BRIGHT * (1 + 0.05 u), u the
pixel's own uniform draw. Frames of at least 37 x 29 pixels (x, y; w1 = w - 1, h1 = h - 1):
  bright pixels      alone (10, 8); a 2x2 cluster (22, 4) .. (23, 5); corners (0, 0), (w1, 0), (0, h1), (w1, h1);
                     edges (18, 0), (18, h1), (0, 14), (w1, 14)
  bad colours        NaN at (26, 10), +inf at (28, 10), negative at (30, 10); the bright pixel (27, 11) has the first two
                     among its neighbours and the bright pixel (31, 10) the third
  a huge pixel       3e38 per channel at (12, 20). The Rec. 709 weights sum to 1, so its luminance is 3e38 and does not
                     overflow: e / L rounds to 1 and the pixel hands its whole colour to the pyramid, whose sums stay
                     below the largest float (a lone texel's share of a level is at most (6 / 16)^2).
5 x 3: bright pixels at (2, 1) and (0, 0), a NaN colour at (4, 2), a +inf colour at (3, 2), a negative colour at (4, 0).
1 x 1: one bright pixel. The two small frames carry no 3e38: their upper levels are single texels, each the frame's
mean, and eight of them would add up past the largest float.

Shared by tests/test_bloom.py (hostsim) and tests/test_bloom_gpu.py (gfx950). Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import rt_amd
from rt_amd import BloomParams, ptr

f32 = np.float32
FMAX = float(np.finfo(np.float32).max)
SHAPES = [(1, 1), (5, 3), (37, 29), (130, 67), (263, 41)]
LEVELS = [1, 3, 8]
BRIGHT = 50.0
HUGE = 3e38
SEED = 11
W709 = tuple(float(f32(v)) for v in (0.2126, 0.7152, 0.0722))  # rt_firefly.h's float constants
TAPS = tuple(float(v) for v in (0.0625, 0.25, 0.375, 0.25, 0.0625))

# |hostsim - float64 model| / max(1, |model|) over SHAPES x LEVELS at the default threshold, knee and intensity, largest
# over every pixel and channel of both outputs (no pixel is left out: the bright pass is continuous in L). Measured on the
# hostsim build; the bound is 4x the measurement, firefly_cases.py's margin. The figure is float32 rounding: a texel of
# level k is 6 k weighted sums of 5 terms, the glow a sum of `levels` such values through 2 mixes each, some 60 roundings
# of up to 2^-24 = 6e-8 between a bright pixel and the output, of which most cancel.
MODEL_MEASURED = 4.82e-7  # 263x41, levels 8, both outputs (the smallest: 1.5e-8 at 1x1, levels 1)
MODEL_TOL = 4 * MODEL_MEASURED


def params(threshold=1.0, knee=0.5, intensity=0.2, levels=5):
    return BloomParams(threshold, knee, intensity, levels)


def inputs(w, h, seed=SEED):
    """rgba [h, w, 4] float32 of one case."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w) / max(w - 1, 1), np.arange(h) / max(h - 1, 1))
    rgba = np.empty((h, w, 4), f32)
    rgba[..., 0] = 0.2 + 0.6 * x
    rgba[..., 1] = 0.2 + 0.6 * y
    rgba[..., 2] = 0.8 - 0.3 * (x + y)
    rgba[..., :3] += (0.1 * rng.random((h, w, 3))).astype(f32)
    rgba[..., 3] = rng.random((h, w)).astype(f32)  # (alpha is copied, whatever it holds)
    u = rng.random((h, w))

    def bright(px):
        for (bx, by) in px:
            rgba[by, bx, :3] = f32(BRIGHT * (1 + 0.05 * u[by, bx]))

    if w >= 37 and h >= 29:
        w1, h1 = w - 1, h - 1
        bright([(10, 8), (22, 4), (23, 4), (22, 5), (23, 5), (0, 0), (w1, 0), (0, h1), (w1, h1), (18, 0), (18, h1), (0, 14),
                (w1, 14), (27, 11), (31, 10)])
        rgba[10, 26, 1] = np.nan
        rgba[10, 28, 2] = np.inf
        rgba[10, 30, :3] = (-0.5, -0.4, -0.6)
        rgba[20, 12, :3] = HUGE
    elif (w, h) == (5, 3):
        bright([(2, 1), (0, 0)])
        rgba[2, 4, 0] = np.nan
        rgba[2, 3, 1] = np.inf
        rgba[0, 4, :3] = (-0.5, -0.4, -0.6)
    else:
        bright([(0, 0)])
    return rgba


def bad_pixels(rgba):
    return ~np.isfinite(rgba[..., :3]).all(-1)


# ------------------------------------------------------------------ the reference (numpy float64)
def luminance(rgb):
    c = rgb.astype(np.float64)
    with np.errstate(all="ignore"):
        return (W709[0] * c[..., 0] + W709[1] * c[..., 1]) + W709[2] * c[..., 2]


def bright_pass(rgba, p):
    """Step 1: b [h, w, 3] float64."""
    T, K = float(f32(p.threshold)), float(f32(p.knee))
    c = rgba[..., :3].astype(np.float64)
    with np.errstate(all="ignore"):
        L = luminance(c)
        ok = np.isfinite(c).all(-1) & (np.abs(L) <= FMAX)  # (a float32 L beyond the largest float is an infinity)
        Ls = np.where(ok, L, 0.0)
        d = Ls - T
        s = np.minimum(np.maximum(d + K, 0.0), 2 * K)
        q = s * s / (4 * K) if K > 0 else np.zeros_like(s)
        e = np.maximum(q, d)
        on = ok & (e > 0)
        f = np.where(on, e / np.where(on, Ls, 1.0), 0.0)
        return np.where(on[..., None], np.where(on[..., None], c, 0.0) * f[..., None], 0.0)


def reduce_level(g):
    """Step 2: the next level of g [h, w, 3]."""
    h, w = g.shape[:2]
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    xs = [np.clip(2 * np.arange(w2) + m, 0, w - 1) for m in range(-2, 3)]
    ys = [np.clip(2 * np.arange(h2) + n, 0, h - 1) for n in range(-2, 3)]
    rows = sum(TAPS[m] * g[:, xs[m]] for m in range(5))  # [h, w2, 3]: the row sums of every source row
    return sum(TAPS[n] * rows[ys[n]] for n in range(5))


def expand_level(u, w, h):
    """Step 3's expand of u [h', w', 3] to w x h."""
    h1, w1 = u.shape[:2]
    x, y = np.arange(w), np.arange(h)
    xs, ys = x >> 1, y >> 1
    xn = np.clip(xs + np.where(x & 1, 1, -1), 0, w1 - 1)
    yn = np.clip(ys + np.where(y & 1, 1, -1), 0, h1 - 1)
    row = lambda yy: 0.75 * u[yy][:, xs] + 0.25 * u[yy][:, xn]  # noqa: E731
    return 0.75 * row(ys) + 0.25 * row(yn)


def model(rgba, p):
    """(rgba_out [h, w, 4], layer [h, w, 4]) in float64; a bad centre is the input's own record."""
    h, w = rgba.shape[:2]
    g = [bright_pass(rgba, p)]
    for _ in range(p.levels):
        g.append(reduce_level(g[-1]))
    u = g[p.levels]
    for k in range(p.levels - 1, 0, -1):
        u = g[k] + expand_level(u, g[k].shape[1], g[k].shape[0])
    scale = float(f32(p.intensity) / f32(p.levels))  # (the host's one float division)
    add = scale * expand_level(u, w, h) if scale > 0 else np.zeros((h, w, 3))
    out = rgba.astype(np.float64)
    keep = bad_pixels(rgba)
    with np.errstate(all="ignore"):
        out[..., :3] = np.where(keep[..., None], out[..., :3], out[..., :3] + add)
    layer = np.zeros((h, w, 4))
    layer[..., :3] = add
    return out, layer


def model_error(got, want):
    """The largest |got - want| / max(1, |want|) over an output; NaN and infinity positions must match exactly."""
    g = got.astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(want)), "NaN positions"
    assert np.array_equal(np.isinf(g), np.isinf(want)) and np.array_equal(g[np.isinf(g)], want[np.isinf(want)]), "infinities"
    fin = np.isfinite(want)
    e = np.abs(np.where(fin, g, 0.0) - np.where(fin, want, 0.0)) / np.maximum(1.0, np.abs(np.where(fin, want, 0.0)))
    return float(e.max(initial=0.0))


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


def bloom(rgba, p=None, hostsim=True, code=False, layer=True, **over):
    """(rgba_out, layer_out) of rt_bloom, or its return code. over: replacements for the call's arguments by name
    (rgba_in, out, layer_out, w, h)."""
    L, hnd = ctx(hostsim)
    H, W = rgba.shape[:2]
    a = dict(rgba_in=rgba, w=W, h=H, out=np.full((H, W, 4), -5.0, f32), layer_out=np.full((H, W, 4), -5.0, f32) if layer else None)
    a.update(over)
    rc = L.rt_bloom(hnd, a["w"], a["h"], ptr(a["rgba_in"]), ctypes.byref(p) if p is not None else None, ptr(a["out"]),
                    ptr(a["layer_out"]))
    if code:
        return rc
    rt_amd.check(L, rc, hnd, "rt_bloom")
    return a["out"], a["layer_out"]


_host_cache = {}


def host_result(w, h, levels):
    """hostsim's two outputs for a synthetic case at the default threshold, knee and intensity, computed once and shared
    (read-only)."""
    key = (w, h, levels)
    if key not in _host_cache:
        got = bloom(inputs(w, h), params(levels=levels))
        for a in got:
            a.setflags(write=False)
        _host_cache[key] = got
    return _host_cache[key]
