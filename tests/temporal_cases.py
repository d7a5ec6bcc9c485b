"""Temporal accumulation (rt_temporal_accumulate; include/rt_hip.h). The reference is model(): the header
comment restated in numpy float64, never calling the library.

Inputs are synthetic, so no scene is bound: a finite wall (z = -6, |x| <= 3.2, |y| <= 3) and a nearer box
face (z = -3, -0.8 <= x <= 0.6, -0.5 <= y <= 0.7), both with normal (0, 0, 1), seen analytically from the
current camera (normal_depth) and from the previous one (the history's). The cameras, all with the presets'
fov_dist, the current one at (0, 0.1, 1) looking down -z:
  same     the previous camera is the current one
  shift    the previous camera 0.4, 0.2, 0.1 away: a few pixels' worth at these frame sizes
  turn     the previous camera turned about y by a third of the horizontal field of view: a third of the
           frame's history lies outside the image
  away     the previous camera turned by 180 degrees: ratio <= 0 everywhere
Planted faults, on fixed flat-index patterns of the history buffers (i = y * w + x):
  i % 23 == 1   depth scaled by 1.5        i % 23 == 7    normal flipped
  i % 23 == 12  a miss beside hits         i % 23 == 18   len = 0
  i % 29 == 3   NaN colour                 i % 29 == 17   +inf colour
  i % 31 == 5   NaN sigma                  i % 31 == 22   +inf sigma
and in this frame (frames of more than 4 pixels): a NaN colour at n // 3, a +inf colour at n // 3 + 1, a NaN
sigma at n // 2, a +inf sigma at n // 2 + 1, a NaN normal at 2 n // 3. The depth faults are off by x 1.5 and
the normals equal or opposite, far from depth_tol and normal_cos.

Shared by tests/test_temporal.py (hostsim) and tests/test_temporal_gpu.py (gfx950). Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import rt_amd
from rt_amd import TemporalParams, ptr

f32 = np.float32
VMAX = float(np.finfo(np.float32).max)
SHAPES = [(1, 1), (5, 3), (37, 29), (130, 67)]
CAMERAS = ("same", "shift", "turn", "away")
FOV = float(f32(1.0 / np.tan(np.radians(22.5))))
NEAR = 1e-4       # a pixel whose model quantity is this close to its threshold is left out ...
NEAR_CAP = 0.02   # ... and at most this share of a case's pixels may be

# |hostsim - float64 model| over SHAPES x CAMERAS, largest over the compared pixels. Colour: absolute. sigma_out
# and len_out: |got - want| / max(1, want). Measured on the hostsim build; the bounds are 4x the measurements.
# The history here is white noise (neighbouring taps differ by the whole value range: colour 1, len 7), so the
# figure is the float32 error of the tap position, about 130 x 2^-23 at the widest frame, times that range.
COLOR_MEASURED = 3.53e-5  # 130x67, turn
SIGMA_MEASURED = 1.69e-5  # 130x67, turn
LEN_MEASURED = 6.24e-5    # 130x67, turn
COLOR_TOL = 4 * COLOR_MEASURED
SIGMA_TOL = 4 * SIGMA_MEASURED
LEN_TOL = 4 * LEN_MEASURED


def params(depth_tol=0.05, normal_cos=0.9, min_weight=0.1, max_len=32.0):
    return TemporalParams(depth_tol, normal_cos, min_weight, max_len)


# ------------------------------------------------------------------ cameras
def _cam(pos, yaw_deg):
    a = np.radians(yaw_deg)
    rot = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    tr = np.eye(4)
    tr[:3, 3] = pos
    flip = np.diag([1.0, 1.0, -1.0, 1.0])  # the reference's camera looks down -z
    return rt_amd.Camera((tr @ rot @ flip).astype(f32), FOV)


def cameras(kind, w, h):
    """(current, previous) Camera for a case."""
    cur = _cam((0.0, 0.1, 1.0), 0.0)
    if kind == "same":
        return cur, _cam((0.0, 0.1, 1.0), 0.0)
    if kind == "shift":
        return cur, _cam((0.4, 0.3, 1.1), 0.0)
    if kind == "turn":
        hfov = 2 * np.degrees(np.arctan((w / h) / FOV))
        return cur, _cam((0.0, 0.1, 1.0), hfov / 3)
    if kind == "away":
        return cur, _cam((0.0, 0.1, 1.0), 180.0)
    raise KeyError(kind)


def rays(cam, w, h):
    """(o [3], d [h, w, 3]) of the feature pass's rays in float64."""
    M = cam.view_matrix.astype(np.float64)
    aspect = float(f32(w) / f32(h))
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xn = (x / w * 2 - 1) * aspect
    yn = y / h * 2 - 1
    pc = np.stack([xn, yn, np.full_like(xn, cam.fov_dist), np.ones_like(xn)], -1) @ M.T
    pd = pc[..., :3] / pc[..., 3:]
    o4 = M @ np.array([0.0, 0.0, 0.0, 1.0])
    o = o4[:3] / o4[3]
    d = pd - o
    return o, d / np.linalg.norm(d, axis=-1, keepdims=True)


RECTS = ((-6.0, -3.2, 3.2, -3.0, 3.0), (-3.0, -0.8, 0.6, -0.5, 0.7))  # (z, x0, x1, y0, y1): the wall, the box face


def normal_depth(cam, w, h):
    """[h, w, 4] float32 {n, t} of the two rectangles' first hit; a miss is {0, 0, 0, -1}."""
    o, d = rays(cam, w, h)
    t = np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        for z, x0, x1, y0, y1 in RECTS:
            tz = (z - o[2]) / d[..., 2]
            px, py = o[0] + tz * d[..., 0], o[1] + tz * d[..., 1]
            ok = (tz > 0) & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & (tz < t)
            t = np.where(ok, tz, t)
    nd = np.zeros((h, w, 4), f32)
    hit = np.isfinite(t)
    nd[..., 2] = np.where(hit, 1.0, 0.0)
    nd[..., 3] = np.where(hit, t, -1.0)
    return nd


# ------------------------------------------------------------------ inputs
def inputs(kind, w, h, seed=5, faults=True):
    """dict(cur, prev, rgba, sigma, nd, hist=(rgba, sigma, len, nd)) of one case; float32 arrays."""
    rng = np.random.default_rng(seed)
    cur, prev = cameras(kind, w, h)
    n = w * h
    rgba = rng.random((h, w, 4)).astype(f32)
    sigma = (0.05 + 0.45 * rng.random((h, w))).astype(f32)
    nd = normal_depth(cur, w, h)
    h_rgba = rng.random((h, w, 4)).astype(f32)
    h_sigma = (0.05 + 0.45 * rng.random((h, w))).astype(f32)
    h_len = (1 + 7 * rng.random((h, w))).astype(f32)
    h_len[2 * h // 3:] = 40.0  # (above max_len)
    h_nd = normal_depth(prev, w, h)
    if faults:
        i = np.arange(n).reshape(h, w)
        h_nd[..., 3] = np.where((i % 23 == 1) & (h_nd[..., 3] > 0), h_nd[..., 3] * f32(1.5), h_nd[..., 3])
        h_nd[i % 23 == 7, :3] *= f32(-1)
        h_nd[i % 23 == 12] = (0, 0, 0, -1)
        h_len[i % 23 == 18] = 0
        h_rgba[i % 29 == 3, 1] = np.nan
        h_rgba[i % 29 == 17, 2] = np.inf
        h_sigma[i % 31 == 5] = np.nan
        h_sigma[i % 31 == 22] = np.inf
        if n > 4:
            rgba.reshape(-1, 4)[n // 3, 0] = np.nan
            rgba.reshape(-1, 4)[n // 3 + 1, 2] = np.inf
            sigma.reshape(-1)[n // 2] = np.nan
            sigma.reshape(-1)[n // 2 + 1] = np.inf
            nd.reshape(-1, 4)[2 * n // 3, 1] = np.nan
    return dict(cur=cur, prev=prev, rgba=rgba, sigma=sigma, nd=nd, hist=(h_rgba, h_sigma, h_len, h_nd))


# ------------------------------------------------------------------ the reference (numpy float64)
def variance(sigma):
    with np.errstate(all="ignore"):
        v = sigma.astype(np.float64) ** 2
    return np.where(np.isnan(v), 0.0, np.minimum(v, VMAX))


def model(cur, prev, rgba, sigma, nd, hist, p):
    """(rgba_out [h, w, 4], sigma_out, len_out, near [h, w] bool) in float64: near marks the pixels where one of
    the three threshold quantities is within NEAR of its threshold."""
    h, w = sigma.shape
    c = rgba[..., :3].astype(np.float64)
    vc = variance(sigma)
    out = np.concatenate([c, np.ones((h, w, 1))], -1)
    s_out, l_out = np.sqrt(vc), np.ones((h, w))
    near = np.zeros((h, w), bool)
    if hist is None:
        return out, s_out, l_out, near
    h_rgba, h_sigma, h_len, h_nd = hist
    g = nd.astype(np.float64)
    carry = ~np.isfinite(c).all(-1) | np.isnan(g).any(-1)
    o, d = rays(cur, w, h)
    Mp = prev.view_matrix.astype(np.float64)
    inv = np.linalg.inv(Mp).astype(f32).astype(np.float64)  # (the host rounds the inverse to float)
    o4 = Mp @ np.array([0.0, 0.0, 0.0, 1.0])
    op = o4[:3] / o4[3]
    hit = g[..., 3] > 0
    with np.errstate(all="ignore"):
        P = np.where(hit[..., None], o + g[..., 3:] * d, op + d)
        t_exp = np.linalg.norm(P - op, axis=-1)
        q4 = np.concatenate([P, np.ones((h, w, 1))], -1) @ inv.T
        q = q4[..., :3] / q4[..., 3:]
        ratio = q[..., 2] / prev.fov_dist
        aspect = float(f32(w) / f32(h))
        fx = ((q[..., 0] / ratio) / aspect + 1) * 0.5 * w
        fy = (q[..., 1] / ratio + 1) * 0.5 * h
        have = ~carry & (ratio > 0) & (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
    fx, fy = np.where(have, fx, 0.0), np.where(have, fy, 0.0)
    ix, iy = np.floor(fx).astype(int), np.floor(fy).astype(int)
    tx, ty = fx - ix, fy - iy
    hc, hs, hl = h_rgba[..., :3].astype(np.float64), h_sigma.astype(np.float64), h_len.astype(np.float64)
    hg = h_nd.astype(np.float64)
    S, sc, sl, sv = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    for dy in (0, 1):
        for dx in (0, 1):
            qx, qy = ix + dx, iy + dy
            b = (ty if dy else 1 - ty) * (tx if dx else 1 - tx)
            ok = have & (b != 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            X, Y = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            with np.errstate(all="ignore"):
                ok &= hl[Y, X] > 0
                ok &= np.isfinite(hc[Y, X]).all(-1) & np.isfinite(hs[Y, X])
                ok &= (hg[Y, X, 3] > 0) == hit
                rel = np.abs(hg[Y, X, 3] - t_exp) / t_exp
                dots = (g[..., :3] * hg[Y, X, :3]).sum(-1)
                geo = ~hit | ((rel <= float(f32(p.depth_tol))) & (dots >= float(f32(p.normal_cos))))
                near |= ok & hit & ((np.abs(rel - float(f32(p.depth_tol))) < NEAR) |
                                    (np.abs(dots - float(f32(p.normal_cos))) < NEAR))
                ok &= geo
                bb = np.where(ok, b, 0.0)
                S += bb
                sc += bb[..., None] * np.where(ok[..., None], hc[Y, X], 0.0)
                sl += bb * np.where(ok, hl[Y, X], 0.0)
                sv += bb * np.where(ok, hs[Y, X] ** 2, 0.0)
    near |= have & (np.abs(S - float(f32(p.min_weight))) < NEAR)
    have &= S > float(f32(p.min_weight))
    Ss = np.where(have, S, 1.0)
    c_h, len_h, v_h = sc / Ss[..., None], sl / Ss, np.minimum(sv / Ss, VMAX)
    ln = np.minimum(len_h + 1, float(f32(p.max_len)))
    a = 1 / ln
    with np.errstate(all="ignore"):
        rgb = c_h + a[..., None] * (c - c_h)
        v = np.minimum((1 - a) ** 2 * v_h + a * a * vc, VMAX)
    out[..., :3] = np.where(have[..., None], rgb, c)
    return out, np.where(have, np.sqrt(v), s_out), np.where(have, ln, 1.0), near


def model_errors(got, want, near):
    """(colour, sigma_out, len_out) errors over the pixels not in `near`, as the *_TOL measure them; NaN and
    infinite colours must match exactly and are left out of the figure."""
    (o, s, ln), (wo, ws, wl) = got, want[:3]
    keep = ~near
    fin = np.isfinite(wo)
    assert np.array_equal(np.isnan(o[keep]), np.isnan(wo[keep])) and np.array_equal(np.isinf(o[keep]), np.isinf(wo[keep]))
    assert np.isfinite(s).all() and np.isfinite(ln).all()
    eo = np.abs(np.where(fin, o.astype(np.float64) - np.where(fin, wo, 0.0), 0.0))[keep]
    es = (np.abs(s.astype(np.float64) - ws) / np.maximum(1.0, ws))[keep]
    el = (np.abs(ln.astype(np.float64) - wl) / np.maximum(1.0, wl))[keep]
    return (float(eo.max(initial=0.0)), float(es.max(initial=0.0)), float(el.max(initial=0.0)))


# ------------------------------------------------------------------ the calls
_ctx = {}


def ctx(hostsim=True, camera=None):
    """One bare context per library (the stage needs a camera, no scene), with `camera` bound."""
    if hostsim not in _ctx:
        L = rt_amd.lib(hostsim)
        hnd = ctypes.c_void_p()
        rt_amd.check(L, L.rt_create(0, ctypes.byref(hnd)), None, "rt_create")
        _ctx[hostsim] = (L, hnd)
    L, hnd = _ctx[hostsim]
    if camera is not None:
        rt_amd.check(L, L.rt_set_camera(hnd, ptr(camera.view_matrix), camera.fov_dist), hnd, "rt_set_camera")
    return L, hnd


def accumulate(case, p=None, hostsim=True, history=True, code=False, **over):
    """(rgba_out, sigma_out, len_out) of rt_temporal_accumulate on a case of inputs(), or its return code.
    over: replacements for the call's arguments by name (rgba, sigma, nd, hist, out, sigma_out, len_out, prev_view,
    prev_fov)."""
    L, hnd = ctx(hostsim, case["cur"])
    a = dict(rgba=case["rgba"], sigma=case["sigma"], nd=case["nd"], hist=case["hist"] if history else (None,) * 4,
             prev_view=case["prev"].view_matrix, prev_fov=case["prev"].fov_dist)
    H, W = case["sigma"].shape
    a.update(out=np.full((H, W, 4), -5.0, f32), sigma_out=np.full((H, W), -5.0, f32), len_out=np.full((H, W), -5.0, f32))
    a.update(over)
    rc = L.rt_temporal_accumulate(hnd, W, H, ptr(a["rgba"]), ptr(a["sigma"]), ptr(a["nd"]), ptr(a["prev_view"]),
                                  ctypes.c_float(a["prev_fov"]), *(ptr(x) for x in a["hist"]),
                                  ctypes.byref(p) if p is not None else None, ptr(a["out"]), ptr(a["sigma_out"]),
                                  ptr(a["len_out"]))
    if code:
        return rc
    rt_amd.check(L, rc, hnd, "rt_temporal_accumulate")
    return a["out"], a["sigma_out"], a["len_out"]


_host_cache = {}


def host_result(kind, w, h, history=True):
    """hostsim's outputs for a case at the default parameters, computed once and shared (read-only)."""
    key = (kind, w, h, history)
    if key not in _host_cache:
        got = accumulate(inputs(kind, w, h), params(), history=history)
        for a in got:
            a.setflags(write=False)
        _host_cache[key] = got
    return _host_cache[key]


# ------------------------------------------------------------------ Cornell frames by the seeding recipe
def moved_camera(k, step=0.02):
    """The cornell preset moved k steps along x and half as far along y."""
    cam = rt_amd.Camera.preset("cornell")
    m = cam.view_matrix.copy()
    m[0, 3] += f32(step * k)
    m[1, 3] += f32(0.5 * step * k)
    return rt_amd.Camera(m, cam.fov_dist)


def recipe_frame(rk, k, n0, samples, W, H):
    """Frame k of the seeding recipe on the kernel's current camera: a tracked progression of n0 + k samples
    declared, two passes of samples / 2 rendered; (linear Image, sigma)."""
    rk.progress_begin(n0 + k)
    rk.progress_track_noise()
    rk.progress_advance(samples // 2)
    rk.progress_advance(samples // 2)
    lin = rk.progress_resolve_linear(rt_amd.Image(W, H))
    sigma = rk.progress_noise_sigma()
    rk.progress_end()
    return lin, sigma
