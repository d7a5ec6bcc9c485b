"""The guided upscale stage (rt_upscale; include/rt_hip.h). The reference is model(): the header comment restated
in numpy float64, never calling the library.

Inputs are synthetic, so no scene is bound: temporal_cases' wall and nearer box face, seen analytically by its
camera at the low and at the output size, so that the guides of the two sizes belong to one scene (one field of
view where the aspects agree: (5, 3) -> (10, 6) and the identity). The wall's albedo steps at world x = 1.5, where
the depth does not; the box face has an albedo of its own. Colour and sigma (0.05 .. 0.5) are white noise.
Planted faults, by flat index i of the low frame (j of the output guides), in frames of more than 4 pixels:
  colour      NaN at i % 29 == 3, +inf at i % 29 == 17
  sigma       NaN at i % 31 == 5, +inf at i % 31 == 22
  low guides  a NaN normal at i % 37 == 9; a miss {0, 0, 0, -1} with albedo 0 at i % 41 == 11 (misses beside hits)
  out guides  a NaN normal at j % 97 == 13; a miss at j % 101 == 50
and, in low frames of at least 37 x 29, a 4 x 4 block of NaN colours at x 20..23, y 10..13: the output pixels whose
sixteen taps all fall in it are the empty case.

Shared by tests/test_upscale.py (hostsim) and tests/test_upscale_gpu.py (gfx950).
Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import rt_amd
import temporal_cases as tc
from rt_amd import UpscaleParams, ptr

f32 = np.float32
VMAX = float(np.finfo(np.float32).max)
# (w_lo, h_lo, w, h)
PAIRS = [(1, 1, 1, 1), (1, 1, 3, 2), (5, 3, 10, 6), (37, 29, 130, 67), (65, 17, 130, 67), (130, 67, 130, 67), (33, 1, 257, 1)]
SEED = 11
NEAR = 1e-4       # a pixel whose model S is within this (relative) of min_weight ...
NEAR0 = 16 * 2.0 ** -126  # ... or positive and below this: within a relative 1e-4 of 0 is 0 alone, but a sum of up to 16
                  # weights below float32's normal range is what float32 cannot tell from 0 ...
NEAR_CAP = 0.02   # ... is left out, and at most this share of a case's pixels may be
U = 2.0 ** -24    # float32's unit roundoff


def params(sigma_normal=0.3, sigma_albedo=0.1, sigma_depth=0.1, min_weight=0.1):
    return UpscaleParams(sigma_normal, sigma_albedo, sigma_depth, min_weight)


# ------------------------------------------------------------------ inputs
def guides(w, h):
    """(albedo, normal_depth) [h, w, 4] float32 of the wall and the box face at one size."""
    cam = tc.cameras("same", w, h)[0]
    nd = tc.normal_depth(cam, w, h)
    o, d = tc.rays(cam, w, h)
    t = nd[..., 3].astype(np.float64)
    hit = t > 0
    px = o[0] + np.where(hit, t, 0.0) * d[..., 0]
    box = hit & (t < 5.0)  # (the box face lies at z = -3, the wall at z = -6; the camera at z = 1)
    alb = np.zeros((h, w, 4), f32)
    alb[hit] = (0.7, 0.7, 0.7, 0.0)
    alb[hit & ~box & (px > 1.5)] = (0.2, 0.6, 0.3, 0.0)
    alb[box] = (0.7, 0.2, 0.2, 0.0)
    return alb, nd


_inputs = {}


def inputs(w_lo, h_lo, w, h, seed=SEED):
    """dict(rgba, sigma, alb_lo, nd_lo, alb_hi, nd_hi) of one case; float32 arrays, computed once (read-only)."""
    key = (w_lo, h_lo, w, h, seed)
    if key in _inputs:
        return _inputs[key]
    rng = np.random.default_rng(seed)
    rgba = rng.random((h_lo, w_lo, 4)).astype(f32)
    sigma = (0.05 + 0.45 * rng.random((h_lo, w_lo))).astype(f32)
    alb_lo, nd_lo = guides(w_lo, h_lo)
    alb_hi, nd_hi = guides(w, h)
    n_lo, n = w_lo * h_lo, w * h
    if n_lo > 4:
        i = np.arange(n_lo).reshape(h_lo, w_lo)
        rgba[i % 29 == 3, 1] = np.nan
        rgba[i % 29 == 17, 2] = np.inf
        sigma[i % 31 == 5] = np.nan
        sigma[i % 31 == 22] = np.inf
        nd_lo[i % 37 == 9, 0] = np.nan
        nd_lo[i % 41 == 11] = (0, 0, 0, -1)
        alb_lo[i % 41 == 11] = 0
        j = np.arange(n).reshape(h, w)
        nd_hi[j % 97 == 13, 1] = np.nan
        nd_hi[j % 101 == 50] = (0, 0, 0, -1)
        alb_hi[j % 101 == 50] = 0
    if w_lo >= 37 and h_lo >= 29:
        rgba[10:14, 20:24, 0] = np.nan
    case = dict(rgba=rgba, sigma=sigma, alb_lo=alb_lo, nd_lo=nd_lo, alb_hi=alb_hi, nd_hi=nd_hi)
    for a in case.values():
        a.setflags(write=False)
    _inputs[key] = case
    return case


# ------------------------------------------------------------------ the reference (numpy float64)
def _inv_sigma2(s):
    """dn_inv_sigma2: 1 / sigma^2 as the float the library multiplies by."""
    v = 1.0 / (float(f32(s)) ** 2)
    return float(f32(min(max(v, 1.1754943508222875e-38), VMAX)))


def model(case, p, sigma=True, force3=False):
    """dict(rgb [h, w, 3], sigma [h, w] or None, tier [h, w] (0: empty), S [h, w], near [h, w] bool) in float64."""
    rgba, nd_lo, alb_lo = (case[k].astype(np.float64) for k in ("rgba", "nd_lo", "alb_lo"))
    nd_hi, alb_hi = case["nd_hi"].astype(np.float64), case["alb_hi"].astype(np.float64)
    sg = case["sigma"].astype(np.float64) if sigma else None
    h_lo, w_lo = rgba.shape[:2]
    h, w = nd_hi.shape[:2]
    sx, sy = float(f32(w_lo) / f32(w)), float(f32(h_lo) / f32(h))
    inv_n, inv_a, inv_t = _inv_sigma2(p.sigma_normal), _inv_sigma2(p.sigma_albedo), _inv_sigma2(p.sigma_depth)
    mw = float(f32(p.min_weight))
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    fx, fy = X * sx, Y * sy
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    tx, ty = fx - x0, fy - y0
    fin_c = np.isfinite(rgba[..., :3]).all(-1)
    if sg is not None:
        fin_c &= np.isfinite(sg)
    with np.errstate(all="ignore"):
        var = None if sg is None else np.minimum(sg * sg, VMAX)
    hit_p = nd_hi[..., 3] > 0

    def sums(taps, guided):
        """taps: (qx, qy, b) per tap, arrays over the output pixels, in tap order."""
        sc, ss, sv, se = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        for qx, qy, b in taps:
            ok = (b != 0) & (qx >= 0) & (qx < w_lo) & (qy >= 0) & (qy < h_lo)
            cx, cy = np.clip(qx, 0, w_lo - 1), np.clip(qy, 0, h_lo - 1)
            ok &= fin_c[cy, cx]
            g, e = np.ones((h, w)), np.zeros((h, w))
            if guided:
                nq, aq = nd_lo[cy, cx], alb_lo[cy, cx]
                ok &= hit_p == (nq[..., 3] > 0)
                with np.errstate(all="ignore"):
                    e = ((nd_hi[..., :3] - nq[..., :3]) ** 2).sum(-1) * inv_n + ((alb_hi[..., :3] - aq[..., :3]) ** 2).sum(-1) * inv_a
                    r = (nd_hi[..., 3] - nq[..., 3]) / np.maximum(nd_hi[..., 3], nq[..., 3])
                    e = np.where(hit_p, e + r * r * inv_t, e)
                    ok &= e >= 0
                    g = np.exp(-np.where(ok, e, 0.0))
            wgt = np.where(ok, b * g, 0.0)
            sc += wgt[..., None] * np.where(ok[..., None], rgba[cy, cx, :3], 0.0)
            ss += wgt
            if var is not None:
                sv += wgt * wgt * np.where(ok, var[cy, cx], 0.0)
            # the weight's float32 error: e carries some 10 roundings, rt_expf one ulp, a denormal g half a denormal ulp
            se += np.where(ok, b * (g * (10 * U * np.where(ok, e, 0.0) + 2 * U) + 2.0 ** -149), 0.0)
        return sc, ss, sv, se

    bil = [(x0 + dx, y0 + dy, (ty if dy else 1 - ty) * (tx if dx else 1 - tx)) for dy in (0, 1) for dx in (0, 1)]
    tent = [(x0 + dx, y0 + dy, (1 - np.abs(y0 + dy - fy) / 2) * (1 - np.abs(x0 + dx - fx) / 2))
            for dy in (-1, 0, 1, 2) for dx in (-1, 0, 1, 2)]
    t1, t2, t3 = sums(bil, True), sums(tent, True), sums(bil, False)
    # sum of g over the valid taps of the 4 x 4 ring, whatever their spatial weight: what a shift of fx can move
    one = np.ones((h, w))
    ring = [(qx, qy, one) for qx, qy, _ in tent]
    ring_g, ring_1 = sums(ring, True)[1], sums(ring, False)[1]
    take1 = (t1[1] > mw) & (not force3)
    take2 = ~take1 & (t2[1] > 0) & (not force3)
    take3 = ~take1 & ~take2 & (t3[1] > 0)
    tier = np.where(take1, 1, np.where(take2, 2, np.where(take3, 3, 0)))
    pick = lambda k: np.where(take1, t1[k], np.where(take2, t2[k], t3[k]))  # noqa: E731
    S = pick(1)
    dpos = 2 * U * (w_lo + h_lo)
    dw = np.where(take1 | take2, dpos * ring_g, dpos * ring_1) + pick(3)
    sc = np.where(take1[..., None], t1[0], np.where(take2[..., None], t2[0], t3[0]))
    with np.errstate(all="ignore"):
        rgb = np.where((tier > 0)[..., None], sc / np.where(tier > 0, S, 1.0)[..., None], 0.0)
        s_out = None
        if var is not None:
            s_out = np.where(tier > 0, np.sqrt(np.minimum(pick(2), VMAX)) / np.where(tier > 0, S, 1.0), np.inf)
    # the decisions' thresholds: S1 against min_weight, then S2 and S3 against 0 where they were asked
    near = np.zeros((h, w), bool)
    if not force3:
        near |= np.abs(t1[1] - mw) <= NEAR * mw if mw > 0 else (t1[1] > 0) & (t1[1] <= NEAR0)
        near |= ~take1 & (t2[1] > 0) & (t2[1] <= NEAR0)
    near |= ~take1 & ~take2 & (t3[1] > 0) & (t3[1] <= NEAR0)
    return dict(rgb=rgb, sigma=s_out, tier=tier, S=S, near=near, dw=dw)


def tolerance(want):
    """The float32 build's distance from the float64 model, per pixel, for colours in [0, 1] and sigmas below 1,
    from the operations of rt_upscale.h. out = sum w c / S moves by at most sum |dw| / S when the
    weights w = b g move by dw (|c - out| <= 1); model() adds sum |dw| up from the taps it takes:
      position  fx = (float)X * sx is one rounding of a value below w_lo and 1 - tx one more: |dfx| <= 2 u w_lo, the
                same in y. The spatial weights are piecewise linear in fx and fy with slopes of at most 1, and a
                shift can only bring in taps of the 4 x 4 ring: sum |db| g <= 2 u (w_lo + h_lo) times the sum of g
                over the ring's valid taps.
      guides    e is a sum of non-negative terms, each some 10 roundings from the float32 guides (three differences,
                three squares, two sums, the product with 1 / sigma^2, the running sum): |de| <= 10 u e; rt_expf is
                within one ulp: |dg| <= g (10 u e + 2 u), and half a denormal ulp, 2^-149, where g is denormal.
      sums      wgt = b g, the products wgt c and up to 16 additions, then the division: 20 u of sum w |c| / S <= 1.
    sigma_out = sqrt(sum w^2 v) / S moves by at most (max sqrt v + sigma_out) sum |dw| / S, no more than the same
    figure, the square root, the squares and the products adding some 6 u."""
    return want["dw"] / np.maximum(want["S"], 1e-300) + 26 * U


def model_errors(got_rgba, got_sigma, want):
    """(largest colour error, largest sigma error, largest error / tolerance, pixels left out): over the pixels not
    in near; non-finite model values must match exactly."""
    keep = ~want["near"]
    tol = tolerance(want)
    out = []
    worst = 0.0
    # sigma_out: V = sum wgt (wgt v) is rounded to a multiple of 2^-149 where it is denormal, twice per tap: up to 32
    # of them, and sqrt(V + d) - sqrt(V) <= sqrt(d)
    extra = np.sqrt(32 * 2.0 ** -149) / np.maximum(want["S"], 1e-300)
    for g, x in ((got_rgba[..., :3], want["rgb"]), (got_sigma, want["sigma"])):
        if g is None:
            out.append(0.0)
            continue
        k = keep if g.ndim == 2 else np.broadcast_to(keep[..., None], g.shape)
        t = tol + extra if g.ndim == 2 else np.broadcast_to(tol[..., None], g.shape)
        fin = np.isfinite(x)
        assert np.array_equal(np.isnan(g[k]), np.isnan(x[k])) and np.array_equal(np.isinf(g[k]), np.isinf(x[k]))
        e = np.where(fin, np.abs(np.where(fin, g, 0.0).astype(np.float64) - np.where(fin, x, 0.0)), 0.0)
        out.append(float(e[k].max(initial=0.0)))
        worst = max(worst, float((e / t)[k].max(initial=0.0)))
    return out[0], out[1], worst, int(want["near"].sum())


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


def schedule(hostsim, **kw):
    L, hnd = ctx(hostsim)
    for k, v in kw.items():
        rt_amd.check(L, L.rt_test_schedule(hnd, k.encode(), float(v)), hnd, "rt_test_schedule")


def upscale(case, p=None, use_sigma=True, hostsim=True, code=False, **over):
    """(rgba_out, sigma_out) of rt_upscale, or its return code. over: replacements for the call's arguments by name
    (rgba, sigma, alb_lo, nd_lo, alb_hi, nd_hi, out, sigma_out, w_lo, h_lo, w, h)."""
    L, hnd = ctx(hostsim)
    h_lo, w_lo = case["rgba"].shape[:2]
    h, w = case["nd_hi"].shape[:2]
    a = dict(case, w_lo=w_lo, h_lo=h_lo, w=w, h=h, out=np.full((h, w, 4), -5.0, f32),
             sigma_out=np.full((h, w), -5.0, f32) if use_sigma else None)
    if not use_sigma:
        a["sigma"] = None
    a.update(over)
    rc = L.rt_upscale(hnd, a["w_lo"], a["h_lo"], a["w"], a["h"], ptr(a["rgba"]), ptr(a["sigma"]), ptr(a["alb_lo"]),
                      ptr(a["nd_lo"]), ptr(a["alb_hi"]), ptr(a["nd_hi"]), ctypes.byref(p) if p is not None else None,
                      ptr(a["out"]), ptr(a["sigma_out"]))
    if code:
        return rc
    rt_amd.check(L, rc, hnd, "rt_upscale")
    return a["out"], a["sigma_out"]


_host_cache = {}


def host_result(pair, sigma=True):
    """hostsim's outputs for a synthetic case at the default parameters, computed once and shared (read-only)."""
    key = (pair, sigma)
    if key not in _host_cache:
        got = upscale(inputs(*pair), None, sigma)
        for a in got:
            if a is not None:
                a.setflags(write=False)
        _host_cache[key] = got
    return _host_cache[key]
