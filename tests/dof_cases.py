"""The depth-of-field stage (rt_dof; include/rt_hip.h). The reference is model(): the header comment of rt_dof.h
restated in numpy, never calling the library. The radius r, k(r), the table D, re, a and the weight wq are float32
(numpy's float32 is IEEE, and its sqrt is correctly rounded), so the model shares every exact comparison with the code
and no pixel needs to be left out near a threshold; only the products wq * c, the sums and the final division run in
float64.

Inputs are synthetic, so no scene is bound: the colour is a smooth gradient (0.2 .. 0.8 per channel) plus white noise of
amplitude 0.1 and a random alpha. The distance t comes in four vertical bands of base 2, 8, 1.2 and 2 (x in quarters of
the width), each pixel's t its base times (1 + 0.1 u), u the pixel's own uniform draw; FOCUS is 2 and COC_INF 10. So
band 1 | 2 is a nearly in-focus near surface over a far blurred one, and band 3 | 4 a defocused near surface (r about
6.7) over a nearly in-focus farther one. Frames of at least 37 x 29 pixels (x, y) also carry
  misses             t = -1 over the block x in [w / 2, w / 2 + 9), y in [0, 6) and the single pixel (3, h - 2)
  a NaN colour       at (26, 10);  a NaN t at (28, 12)
  a pixel 1000 times its surroundings at (12, 20)
  exact focus        t = FOCUS over the block x in [4, 9), y in [14, 19): r = 0 there
5 x 3: bands by column (2, 8, 1.2, 2, 2), a miss at (0, 0), a NaN t at (3, 0), a NaN colour at (4, 2), the bright pixel
at (2, 1). 1 x 1: one pixel of band 1.

Shared by tests/test_dof.py (hostsim) and tests/test_dof_gpu.py (gfx950). Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import rt_amd
from rt_amd import DofParams, ptr

f32 = np.float32
SHAPES = [(1, 1), (5, 3), (37, 29), (130, 67), (70, 45)]
RADII = [1, 4, 12]
FOCUS, COC_INF = 2.0, 10.0
SEED = 17
TAB = 13

# |hostsim - model| / max(1, |model|) over SHAPES x RADII at FOCUS and COC_INF, the largest over every pixel and channel
# of rgba_out. Measured on the hostsim build; the bound is 4x the measurement: the margin covers the summation order of up
# to 625 float32 terms on other inputs. The figure is float32 rounding of the products and of the running sums S and W.
MODEL_MEASURED = 1.526e-6  # 130x67, max_radius 12 (37x29: 1.490e-6; at max_radius 4 at most 6.4e-7, at 1 1.9e-7; 1x1: 0)
MODEL_TOL = 4 * MODEL_MEASURED


def params(focus=FOCUS, coc_inf=COC_INF, max_radius=8):
    return DofParams(focus, coc_inf, max_radius)


def inputs(w, h, seed=SEED):
    """(rgba, normal_depth), each [h, w, 4] float32, of one case."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w) / max(w - 1, 1), np.arange(h) / max(h - 1, 1))
    rgba = np.empty((h, w, 4), f32)
    rgba[..., 0] = 0.2 + 0.6 * x
    rgba[..., 1] = 0.2 + 0.6 * y
    rgba[..., 2] = 0.8 - 0.3 * (x + y)
    rgba[..., :3] += (0.1 * rng.random((h, w, 3))).astype(f32)
    rgba[..., 3] = rng.random((h, w)).astype(f32)  # (alpha is copied, whatever it holds)
    u = rng.random((h, w))
    base = np.array([2.0, 8.0, 1.2, 2.0, 2.0])[np.minimum(np.arange(w) * 4 // max(w, 4), 4) if w != 5 else np.arange(5)]
    nd = np.zeros((h, w, 4), f32)
    nd[..., :3] = rng.random((h, w, 3)).astype(f32)  # (the normal is not read)
    nd[..., 3] = (base[None, :] * (1 + 0.1 * u)).astype(f32)
    if w >= 37 and h >= 29:
        nd[0:6, w // 2:w // 2 + 9, 3] = -1.0
        nd[h - 2, 3, 3] = -1.0
        rgba[10, 26, 1] = np.nan
        nd[12, 28, 3] = np.nan
        rgba[20, 12, :3] *= f32(1000.0)
        nd[14:19, 4:9, 3] = FOCUS
    elif (w, h) == (5, 3):
        nd[0, 0, 3] = -1.0
        nd[0, 3, 3] = np.nan
        rgba[2, 4, 0] = np.nan
        rgba[1, 2, :3] *= f32(1000.0)
    return rgba, nd


def bad_pixels(rgba):
    return ~np.isfinite(rgba[..., :3]).all(-1)


# ------------------------------------------------------------------ the reference
def table():
    """D[|dy|][|dx|]: the float nearest sqrt(dx^2 + dy^2)."""
    i = np.arange(TAB, dtype=f32)
    return np.sqrt(i[:, None] * i[:, None] + i[None, :] * i[None, :]).astype(f32)


def far(t):
    with np.errstate(all="ignore"):
        return ~np.isfinite(t) | ~(t > 0)


def radius(t, p):
    """Rule 1 in float32: r [h, w]."""
    t = t.astype(f32)
    R, focus, coc = f32(p.max_radius), f32(p.focus), f32(p.coc_inf)
    with np.errstate(all="ignore"):
        x = coc * (np.abs(t - focus) / t)
        near = np.where(R < x, R, x)  # rt_min(x, R)
    flat = R if R < coc else coc
    return np.where(far(t) | (coc == 0), flat, near).astype(f32)


def k_of(r):
    m = np.where(r < f32(0.5), f32(0.5), r).astype(f32)
    return (f32(1.0) / (m * m)).astype(f32)


def model(rgba, nd, p):
    """(rgba_out [h, w, 4] float64, coc [h, w] float32); a bad centre is the input's own record."""
    h, w = rgba.shape[:2]
    R = p.max_radius
    t = nd[..., 3].astype(f32)
    r = radius(t, p)
    k = k_of(r)
    order = np.where(far(t), f32(np.inf), t).astype(f32)
    ok = ~bad_pixels(rgba)
    c = np.where(ok[..., None], rgba[..., :3], 0).astype(np.float64)
    D = table()
    S, W = np.zeros((h, w, 3)), np.zeros((h, w))

    def pad(a, fill):
        return np.pad(a, [(R, R), (R, R)] + [(0, 0)] * (a.ndim - 2), constant_values=fill)

    rq_, kq_, tq_, ok_, c_ = pad(r, 0), pad(k, 0), pad(order, np.inf), pad(ok, False), pad(c, 0)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sl = (slice(R + dy, R + dy + h), slice(R + dx, R + dx + w))
            rq, kq, tq = rq_[sl], kq_[sl], tq_[sl]
            own = (tq > order) & (r < rq)
            re = np.where(own, r, rq).astype(f32)
            a = ((re + f32(0.5)) - D[abs(dy), abs(dx)]).astype(f32)
            a = np.where(f32(1.0) < a, f32(1.0), a)
            wq = (a * np.where(own, k, kq)).astype(f32)
            wq = np.where(ok_[sl] & (a > 0), wq, f32(0)).astype(np.float64)
            S += wq[..., None] * c_[sl]
            W += wq
    out = rgba.astype(np.float64)
    with np.errstate(all="ignore"):
        out[..., :3] = np.where(ok[..., None], S / W[..., None], out[..., :3])
    return out, r


def model_error(got, want):
    """The largest |got - want| / max(1, |want|); NaN positions must match exactly."""
    g = got.astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(want)), "NaN positions"
    fin = np.isfinite(want)
    assert np.isfinite(g[fin]).all(), "an infinity the model does not have"
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


def dof(rgba, nd, p=None, hostsim=True, code=False, coc=True, **over):
    """(rgba_out, coc_out) of rt_dof, or its return code. over: replacements for the call's arguments by name
    (rgba_in, nd_in, out, coc_out, w, h)."""
    L, hnd = ctx(hostsim)
    H, W = rgba.shape[:2]
    a = dict(rgba_in=rgba, nd_in=nd, w=W, h=H, out=np.full((H, W, 4), -5.0, f32), coc_out=np.full((H, W), -5.0, f32) if coc else None)
    a.update(over)
    rc = L.rt_dof(hnd, a["w"], a["h"], ptr(a["rgba_in"]), ptr(a["nd_in"]), ctypes.byref(p) if p is not None else None,
                  ptr(a["out"]), ptr(a["coc_out"]))
    if code:
        return rc
    rt_amd.check(L, rc, hnd, "rt_dof")
    return a["out"], a["coc_out"]


_host_cache = {}


def host_result(w, h, max_radius):
    """hostsim's two outputs for a synthetic case at FOCUS and COC_INF, computed once and shared (read-only)."""
    key = (w, h, max_radius)
    if key not in _host_cache:
        got = dof(*inputs(w, h), params(max_radius=max_radius))
        for a in got:
            a.setflags(write=False)
        _host_cache[key] = got
    return _host_cache[key]


def tile_case():
    """70 x 45: the 32 x 16 tile at x in [32, 64), y in [16, 32) wholly in focus (t = FOCUS, r = 0) and everything else
    nearer at r = 12 (t = FOCUS / 2 with coc_inf 12: 12 * 1 / 1). (rgba, nd, params)."""
    rgba, nd = inputs(70, 45)
    rgba[...] = np.where(np.isfinite(rgba), rgba, f32(0.5))
    nd[..., 3] = FOCUS / 2
    nd[16:32, 32:64, 3] = FOCUS
    return rgba, nd, params(coc_inf=12.0, max_radius=12)
