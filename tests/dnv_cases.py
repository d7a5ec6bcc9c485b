"""The variance-guided filter and the absolute noise figure (rt_denoise_var, rt_progress_noise_sigma;
include/rt_hip.h). The filter's reference is model(): the header comment restated in numpy float64,
never calling the library. The query's reference is sigma_restate(): the definition in numpy float32.

Inputs: test_denoise.py's synth() colour and guides plus sigma_map(): 0 on the left half, 0.05 .. 0.5 on
the right, a NaN entry at flat index n // 3 and a +inf entry at 2 n // 3 + 1 (frames of one pixel: the
NaN alone). Shared by tests/test_dnv.py (hostsim) and tests/test_dnv_gpu.py (gfx950).

Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import adapt_cases as ac
import noise_cases as nc
import progress_cases as pc
import rt_cases
from test_denoise import HK, SIZES, ctx, synth  # noqa: F401

import rt_amd
from rt_amd import DenoiseVarParams, ptr

f32 = np.float32
VMAX = float(np.finfo(np.float32).max)
BK = np.array([0.25, 0.5, 0.25])

# |hostsim - float64 model| over SIZES x passes 1..5 x {guides, colour only}, sigma_out on.
# Colour: largest absolute difference. sigma_out: largest |got - want| / max(1, want): the +inf entry of the
# sigma map leaves values up to 1.8e19 around it, where only a relative figure means anything, and below 1 the
# figure is the absolute difference. Measured on the hostsim build; the bounds are 4x the measurements (float32
# sums, products and quotients against float64; the library's expf against exp). The project's bar for a visible
# pixel change is 1e-4.
# Where the sigma map is 0 the edge-stop's scale is r = (1 / sigma_color^2) / var_floor = 2500 at the defaults, so
# the 1e-7 a float32 colour carries from the pass before becomes 2.5e-4 in e and in the weight's relative error.
# Colour: 4.04e-6 (37x29, 3 passes, guides). sigma_out: 7.17e-4 (37x29, 4 passes, guides), at pixels whose whole v
# is the +inf entry's 3.4e38 times a weight of 1e-13 squared, so the weight's relative error is the result's, and
# the next pass's r carries it into the colour. With the +inf entry replaced by 0.3 the same sweep gives 4.5e-7 and
# 5.2e-8.
COLOR_MEASURED = 4.04e-6
SIGMA_MEASURED = 7.17e-4
COLOR_TOL = 4 * COLOR_MEASURED
SIGMA_TOL = 4 * SIGMA_MEASURED


def sigma_map(w, h, seed=3):
    rng = np.random.default_rng(seed)
    left = (np.arange(w) < (w + 1) // 2)[None, :].repeat(h, 0)
    s = np.where(left, 0.0, 0.05 + 0.45 * rng.random((h, w))).astype(f32)
    n = w * h
    flat = s.reshape(-1)
    flat[n // 3] = np.nan
    if n > 1:
        flat[min(n - 1, 2 * n // 3 + 1)] = np.inf
    return s


def params(passes=4, sc=2.0, sn=0.3, sa=0.1, st=0.1, floor=1e-4):
    return DenoiseVarParams(passes, sc, sn, sa, st, floor)


def inputs(w, h):
    """(rgba, sigma, albedo, normal_depth): synth() and sigma_map()."""
    rgba, alb, nd = synth(w, h)
    return rgba, sigma_map(w, h), alb, nd


# ------------------------------------------------------------------ the reference (numpy float64)
def _inv(s):
    return min(max(1.0 / (float(s) * float(s)), 1.1754943508222875e-38), VMAX)


def model(rgba, sigma, alb, nd, p, blend):
    """(rgba_out [h, w, 4], sigma_out [h, w]) of the filter in float64."""
    h, w = rgba.shape[:2]
    c = rgba[..., :3].astype(np.float64)
    with np.errstate(all="ignore"):
        v = sigma.astype(np.float64) ** 2
    v = np.where(np.isnan(v), 0.0, np.minimum(v, VMAX))
    guides = alb is not None
    if guides:
        n, t, a = nd[..., :3].astype(np.float64), nd[..., 3].astype(np.float64), alb[..., :3].astype(np.float64)
        hit = t > 0
    inv_c = _inv(p.sigma_color)
    for i in range(p.passes):
        s = 1 << i
        # the 3x3 prefilter of v
        gs, gk = np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                ys, xs = np.arange(h) + dy, np.arange(w) + dx
                vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
                if not vy.any() or not vx.any():
                    continue
                P = np.ix_(np.where(vy)[0], np.where(vx)[0])
                Q = np.ix_(ys[vy], xs[vx])
                gs[P] += BK[dy + 1] * BK[dx + 1] * v[Q]
                gk[P] += BK[dy + 1] * BK[dx + 1]
        with np.errstate(all="ignore"):
            r = inv_c / (np.minimum(gs / gk, VMAX) + float(f32(p.var_floor)))
        fin = np.isfinite(c).all(-1)
        num, den, numv = np.zeros_like(c), np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs = np.arange(h) + dy * s, np.arange(w) + dx * s
                vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
                if not vy.any() or not vx.any():
                    continue
                P = np.ix_(np.where(vy)[0], np.where(vx)[0])
                Q = np.ix_(ys[vy], xs[vx])
                ok = fin[Q] & fin[P]
                with np.errstate(all="ignore"):
                    e = ((c[P] - c[Q]) ** 2).sum(-1) * r[P]
                    if guides:
                        e = e + ((n[P] - n[Q]) ** 2).sum(-1) * _inv(p.sigma_normal)
                        e = e + ((a[P] - a[Q]) ** 2).sum(-1) * _inv(p.sigma_albedo)
                        both = hit[P] & hit[Q]
                        q = np.where(both, (t[P] - t[Q]) / np.where(both, np.maximum(t[P], t[Q]), 1.0), 0.0)
                        e = e + q ** 2 * _inv(p.sigma_depth)
                        ok &= hit[P] == hit[Q]
                    ok &= e >= 0  # (a NaN compares false)
                    wgt = np.where(ok, HK[dy + 2] * HK[dx + 2] * np.exp(-np.where(ok, e, 0.0)), 0.0)
                    num[P] += wgt[..., None] * np.where(ok[..., None], c[Q], 0.0)
                    numv[P] += wgt * wgt * v[Q]
                den[P] += wgt
        keep = ~fin | ~(den > 0)
        safe = np.where(den > 0, den, 1.0)
        with np.errstate(all="ignore"):
            c = np.where(keep[..., None], c, num / safe[..., None])
            v = np.where(keep, v, np.minimum(numv / (safe * safe), VMAX))
    out = np.empty((h, w, 4))
    with np.errstate(all="ignore"):
        out[..., :3] = float(f32(blend)) * c + float(f32(1.0) - f32(blend)) * rgba[..., :3]
    out[..., 3] = 1.0
    return out, np.sqrt(v)


# ------------------------------------------------------------------ the calls
def denoise_var(rgba, sigma, alb, nd, p, blend, hostsim=True, code=False, sigma_out=True):
    """(rgba_out, sigma_out) of rt_denoise_var, or its return code."""
    L, h = ctx(hostsim)
    H, W = rgba.shape[:2]
    out = np.full((H, W, 4), -5.0, f32)
    left = np.full((H, W), -5.0, f32) if sigma_out else None
    rc = L.rt_denoise_var(h, W, H, ptr(rgba), ptr(sigma), ptr(alb), ptr(nd), ctypes.byref(p) if p is not None else None,
                          ctypes.c_float(blend), ptr(out), ptr(left))
    if code:
        return rc
    rt_amd.check(L, rc, h, "rt_denoise_var")
    return out, left


_host_cache = {}


def host_result(w, h, passes, guides, blend=1.0):
    """hostsim's (rgba_out, sigma_out) for a synthetic case at the default sigmas, computed once and shared
    (read-only)."""
    key = (w, h, passes, guides, blend)
    if key not in _host_cache:
        rgba, sigma, alb, nd = inputs(w, h)
        got = denoise_var(rgba, sigma, alb if guides else None, nd if guides else None, params(passes), blend)
        for a in got:
            a.setflags(write=False)
        _host_cache[key] = got
    return _host_cache[key]


def model_errors(got, want):
    """(colour error, sigma_out error) as COLOR_TOL and SIGMA_TOL measure them."""
    (o, s), (wo, ws) = got, want
    assert np.isfinite(s).all() and np.isfinite(ws).all()
    return (float(np.abs(o.astype(np.float64) - wo).max()),
            float((np.abs(s.astype(np.float64) - ws) / np.maximum(1.0, ws)).max()))


# ------------------------------------------------------------------ the sigma query
def sigma_restate(state, half, tn, tna):
    """s = k * d in numpy float32 with per-tile counts ([th, tw] int arrays); [rows, w]."""
    state, half = np.asarray(state, f32), np.asarray(half, f32)
    rows, w = state.shape[:2]
    n = ac.expand(tn, rows, w).astype(f32)
    na = ac.expand(tna, rows, w).astype(f32)
    nb = ac.expand(np.asarray(tn) - np.asarray(tna), rows, w).astype(f32)
    with np.errstate(all="ignore"):
        k = np.sqrt(na / nb)
        m, a = state[..., :3] / n[..., None], half[..., :3] / na[..., None]
        d = (np.abs(m[..., 0] - a[..., 0]) + np.abs(m[..., 1] - a[..., 1])) + np.abs(m[..., 2] - a[..., 2])
        s = k * d
        root = np.sqrt(f32(0.01) + ((m[..., 0] + m[..., 1]) + m[..., 2]))
    assert s.dtype == f32 and root.dtype == f32
    return s, root


def noise_sigma(s, device: bool = False):
    """rt_progress_noise_sigma of a session, or the device form read back."""
    i = pc.info(s)
    rows, w = i[7], i[0]
    if device:
        d = s.array(np.full((rows, w), -5.0, f32))
        s.ok(s.L.rt_progress_noise_sigma_device(s.ctx, ctypes.c_void_p(d.ptr), None), "rt_progress_noise_sigma_device")
        return d.get()
    out = np.full((rows, w), -5.0, f32)
    s.ok(s.L.rt_progress_noise_sigma(s.ctx, ptr(out)), "rt_progress_noise_sigma")
    return out


def uneven_state(w=40, h=30, total=8):
    """A version-3 checkpoint with unequal tile counts, among them a tile with nA == 0 and one with nB == 0:
    (blob, state, half, tile_n, tile_nA)."""
    base, state, half = nc.edges(w, h, 2, 2)
    tn, tna = ac.injected_counts(w, h, total, 1)
    assert ((tna == 0) & (tn > 0)).any() and (tna == tn).any() and len(np.unique(tn)) > 2
    blob = ac.pack_v3(base, state, half, tn, tna, total, passes=2, n_a=2, n_b=2, nb=1)
    return blob, state, half, tn, tna


def case_sigma_uneven(hostsim: bool, want=None):
    """The query on uneven_state(), host and device forms, against sigma_restate() (or `want`), bit for bit with
    NaN matching NaN; the identity with rt_progress_noise's pixel map; the state untouched. Returns the map."""
    s = pc.session(hostsim, "cornell")
    blob, state, half, tn, tna = uneven_state()
    assert pc.load_rc(s, blob) == 0, s.where(f"rt_progress_load: {s.error()}")
    ref, root = sigma_restate(state, half, tn, tna)
    assert (~np.isfinite(ref)).any(), "the nA == 0 tile gives non-finite values"
    got = noise_sigma(s)
    nc.assert_bits(got, ref if want is None else want, s.where("rt_progress_noise_sigma, unequal counts"))
    nc.assert_bits(noise_sigma(s, device=True), got, s.where("the device form"))
    px = nc.noise(s)[0]
    both = np.isfinite(px) & np.isfinite(got)
    with np.errstate(all="ignore"):
        nc.assert_bits(px[both], (got / root)[both], s.where("pixel_err == s / sqrt(0.01 + sum m)"))
    assert both.sum() > 100
    assert pc.save(s) == blob, s.where("the query changed the state")
    s.close()
    return got


# ------------------------------------------------------------------ Cornell frames for the quality figures
def cornell_kernel(cameras, manifest, hostsim, W, H, spp, bounces):
    e = rt_cases.golden_case("cornell32_128", manifest)
    return rt_cases.make_kernel(e, cameras, hostsim, W=W, H=H, spp=spp, bounces=bounces)


def frame_uniform(cameras, manifest, hostsim=True, W=64, H=64, bounces=8, split=(8, 8)):
    """Frame U: a tracked uniform progression; (kernel, linear Image, sigma, tile_n)."""
    rk, _ = cornell_kernel(cameras, manifest, hostsim, W, H, sum(split), bounces)
    rk.progress_begin()
    rk.progress_track_noise()
    for k in split:
        rk.progress_advance(k)
    lin = rk.progress_resolve_linear(rt_amd.Image(W, H))
    return rk, lin, rk.progress_noise_sigma(), rk.progress_tile_counts()[0]


def frame_adaptive(cameras, manifest, hostsim=True, W=64, H=64, bounces=8, total=64, step=8):
    """Frame A: an adaptive progression of `total` in passes of `step`, its threshold the median tile error
    after the second pass; (kernel, linear Image, sigma, tile_n)."""
    rk, _ = cornell_kernel(cameras, manifest, hostsim, W, H, total, bounces)
    rk.progress_begin()
    rk.progress_track_noise()
    rk.progress_advance(step)
    rk.progress_advance(step)
    thr = float(np.median(rk.progress_noise(0.0, tile_map=True)["tile_err"]))
    while rk.progress_advance_adaptive(step, thr)["active_tiles"]:
        pass
    lin = rk.progress_resolve_linear(rt_amd.Image(W, H))
    return rk, lin, rk.progress_noise_sigma(), rk.progress_tile_counts()[0]


def rmse(img, ref):
    return float(np.sqrt(((img[..., :3].astype(np.float64) - ref) ** 2).mean()))
