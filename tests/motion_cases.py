"""The motion stages (rt_motion_vectors, rt_motion_blur; include/rt_hip.h). The references are vectors_model() and
model(): the header comment of rt_motion.h restated in numpy, never calling the library.

vectors_model() is float32 throughout, operation for operation what feature_ray, xform_point and steps 3 and 4 of
rt_temporal.h do (numpy's float32 is IEEE, its sqrt and division correctly rounded, nothing is contracted), with the
previous view inverted by the library's own elimination in double; so it gives the vectors bit for bit. The cameras, the
two rectangles and their first hits come from temporal_cases.py.

model() computes every comparison and discrete choice in float32 with the code's expressions: the reach l and its clamp,
k, t', iz, the tile key, n, the offsets, cyl, the clamps and so alpha as a whole; so the model shares every decision with
the code and no pixel needs to be left out. The products alpha * c, the sums S and W and the final division run in float64.

Inputs are synthetic, so no scene is bound: the colour is a smooth gradient (0.2 .. 0.8 per channel) plus white noise of
amplitude 0.1 and a random alpha. The distance t comes in four vertical bands of base 2, 8, 1.2 and 2 (x in quarters of
the width), each pixel's t its base times (1 + 0.1 u), u the pixel's own uniform draw: neighbours differ by more and by
less than depth_soft = 0.05. Frames of at least 37 x 29 pixels (x, y) also carry
  misses             t = -1 over the block x in [w / 2, w / 2 + 9), y in [0, 6) and the single pixel (3, h - 2)
  a NaN colour       at (26, 10);  a NaN t at (28, 12);  a pixel 1000 times its surroundings at (12, 20)
  a NaN motion       at (9, 7);  a motion of 1e25 px at (30, 22) (l2 overflows: still);  one of 1e6 px at (33, 5) (clamped)
5 x 3: a miss at (0, 0), a NaN t at (3, 0), a NaN colour at (4, 2), the bright pixel at (2, 1), a NaN motion at (1, 2).
The motion fields, in pixels per frame, with SHUTTER 1 (h = m / 2), R = max_radius:
  horizontal  (1.7 R + 0.6, 0): l = 0.85 R + 0.3, clamped at R = 1       vertical  (0, -(1.5 R + 0.9))
  diagonal    (1.3 R + 0.4, 1.1 R + 0.2)
  random      per 16 x 16 tile a direction and a length up to 2.5 R, a third of the tiles still, each pixel's own
              factor 1 +- 0.1 on top

Shared by tests/test_motion.py (hostsim) and tests/test_motion_gpu.py (gfx950). Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import rt_amd
import temporal_cases as tc
from rt_amd import MotionParams, ptr

f32 = np.float32
SHAPES = [(1, 1), (5, 3), (37, 29), (130, 67), (70, 45)]
RADII = [1, 4, 16]
FIELDS = ["horizontal", "vertical", "diagonal", "random"]
SHUTTER, DEPTH_SOFT = 1.0, 0.05
SEED = 23
TILE = 16

# |hostsim - model| / max(1, |model|) over SHAPES x RADII x FIELDS, the largest over every pixel and channel of rgba_out.
# Measured on the hostsim build; the bound is 4x the measurement, the margin of dof_cases.py for the same kind of
# float32-against-float64 sum (here of up to 33 terms). The figure is float32 rounding of the products alpha * c and of
# the running sums S and W.
MODEL_MEASURED = 4.942e-7  # 130x67, max_radius 16, random (vertical: 4.78e-7; at max_radius 4 at most 2.7e-7, at 1 1.3e-7; 1x1: 6e-8)
MODEL_TOL = 4 * MODEL_MEASURED


def params(shutter=SHUTTER, depth_soft=DEPTH_SOFT, max_radius=8):
    return MotionParams(shutter, depth_soft, max_radius)


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
    elif (w, h) == (5, 3):
        nd[0, 0, 3] = -1.0
        nd[0, 3, 3] = np.nan
        rgba[2, 4, 0] = np.nan
        rgba[1, 2, :3] *= f32(1000.0)
    return rgba, nd


def field(kind, w, h, R, seed=SEED):
    """motion [h, w, 2] float32 of one case."""
    m = np.zeros((h, w, 2), f32)
    if kind == "horizontal":
        m[...] = (1.7 * R + 0.6, 0.0)
    elif kind == "vertical":
        m[...] = (0.0, -(1.5 * R + 0.9))
    elif kind == "diagonal":
        m[...] = (1.3 * R + 0.4, 1.1 * R + 0.2)
    elif kind == "random":
        rng = np.random.default_rng(seed + 1)
        ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
        ang = rng.random((ty, tx)) * 2 * np.pi
        length = rng.random((ty, tx)) * 2.5 * R * (rng.random((ty, tx)) > 1 / 3)
        per = np.stack([length * np.cos(ang), length * np.sin(ang)], -1)
        m[...] = np.repeat(np.repeat(per, TILE, 0), TILE, 1)[:h, :w]
        m *= (0.9 + 0.2 * rng.random((h, w, 1))).astype(f32)
    else:
        raise KeyError(kind)
    if w >= 37 and h >= 29:
        m[7, 9, 0] = np.nan
        m[22, 30] = (1e25, 0.0)
        m[5, 33] = (-1e6, 1e6)
    elif (w, h) == (5, 3):
        m[2, 1, 1] = np.nan
    return m


def bad_pixels(rgba):
    return ~np.isfinite(rgba[..., :3]).all(-1)


# ------------------------------------------------------------------ the vectors' reference (float32)
def invert_view(m):
    """The library's inverse of a row-major 4x4: Gauss-Jordan in double with partial pivoting, rounded to float32."""
    a = [[float(m[r][k]) for k in range(4)] + [1.0 if r == k else 0.0 for k in range(4)] for r in range(4)]
    for col in range(4):
        piv = col
        for r in range(col + 1, 4):
            if abs(a[r][col]) > abs(a[piv][col]):
                piv = r
        assert a[piv][col] != 0.0
        a[piv], a[col] = a[col], a[piv]
        d = a[col][col]
        a[col] = [v / d for v in a[col]]
        for r in range(4):
            f = a[r][col]
            if r == col or f == 0.0:
                continue
            a[r] = [v - f * c for v, c in zip(a[r], a[col])]
    return np.array([row[4:] for row in a], np.float64).astype(f32)


def _xform(m, px, py, pz):
    """xform_point in float32: m [4, 4] float32, the point's components float32 arrays or scalars."""
    m = m.astype(f32)
    with np.errstate(all="ignore"):
        row = [((m[r, 0] * px + m[r, 1] * py) + m[r, 2] * pz) + m[r, 3] for r in range(4)]
        inv = f32(1.0) / row[3]
        one = row[3] == f32(1.0)
        return tuple(np.where(one, row[i], row[i] * inv).astype(f32) for i in range(3))


def vectors_model(cur, prev, nd):
    """m [h, w, 2] float32 of rt_motion_vectors, bit for bit."""
    h, w = nd.shape[:2]
    M = cur.view_matrix.astype(f32)
    zero = f32(0.0)
    o = _xform(M, zero, zero, zero)
    op = _xform(prev.view_matrix.astype(f32), zero, zero, zero)
    inv = invert_view(prev.view_matrix)
    aspect = f32(w) / f32(h)
    x, y = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    g = nd.astype(f32)
    with np.errstate(all="ignore"):
        xn = (x / f32(w) * f32(2.0) - f32(1.0)) * aspect
        yn = y / f32(h) * f32(2.0) - f32(1.0)
        pd = _xform(M, xn, yn, np.full_like(xn, f32(cur.fov_dist)))
        v = [pd[i] - o[i] for i in range(3)]
        kk = f32(1.0) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        d = [kk * v[i] for i in range(3)]
        hit = g[..., 3] > 0
        P = [np.where(hit, o[i] + g[..., 3] * d[i], op[i] + d[i]).astype(f32) for i in range(3)]
        q = _xform(inv, *P)
        ratio = q[2] / f32(prev.fov_dist)
        fx = (((q[0] / ratio) / aspect + f32(1.0)) * f32(0.5)) * f32(w)
        fy = ((q[1] / ratio + f32(1.0)) * f32(0.5)) * f32(h)
        ok = ~np.isnan(g).any(-1) & (ratio > 0) & np.isfinite(fx) & np.isfinite(fy)
        m = np.stack([fx - x, fy - y], -1).astype(f32)
    return np.where(ok[..., None], m, f32(0.0)).astype(f32)


# ------------------------------------------------------------------ the blur's reference
def reach(motion, p):
    """Rule 1 in float32: (hx, hy, l), each [h, w]."""
    a = f32(0.5) * f32(p.shutter)
    R = f32(p.max_radius)
    with np.errstate(all="ignore"):
        hx, hy = a * motion[..., 0].astype(f32), a * motion[..., 1].astype(f32)
        l2 = hx * hx + hy * hy
        fin = np.isfinite(l2)
        l = np.sqrt(np.where(fin, l2, f32(0))).astype(f32)
        over = l > R
        s = R / l
        hx, hy = np.where(over, hx * s, hx), np.where(over, hy * s, hy)
        l = np.where(over, R, l)
    z = f32(0)
    return np.where(fin, hx, z).astype(f32), np.where(fin, hy, z).astype(f32), np.where(fin, l, z).astype(f32)


def far(t):
    t = t.astype(f32)
    big = f32(1e30)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(t) & (t > 0), np.where(big < t, big, t), big).astype(f32)


def tile_lines(hx, hy, l):
    """Rules 2 and 3: (N [ty, tx, 3] float32 = {Nx, Ny, L}, tiles [ty, tx, 3] the per-tile records)."""
    h, w = l.shape
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    tiles = np.zeros((ty, tx, 3), f32)
    for j in range(ty):
        for i in range(tx):
            sl = (slice(j * TILE, (j + 1) * TILE), slice(i * TILE, (i + 1) * TILE))
            sub = l[sl]
            k = np.unravel_index(int(np.argmax(sub)), sub.shape)  # (the first of the largest, in raster order)
            tiles[j, i] = (hx[sl][k], hy[sl][k], sub[k])
    N = np.zeros_like(tiles)
    for j in range(ty):
        for i in range(tx):
            best = None
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if 0 <= j + dy < ty and 0 <= i + dx < tx and (best is None or tiles[j + dy, i + dx, 2] > best[2]):
                        best = tiles[j + dy, i + dx]
            N[j, i] = best
    return N, tiles


def _clamp01(x):
    with np.errstate(all="ignore"):
        return np.where(x > 0, np.where(x < 1, x, f32(1)), f32(0)).astype(f32)


def model(rgba, nd, motion, p):
    """(rgba_out [h, w, 4] float64, reach [h, w] float32); a bad centre and a copied tile are the input's own records."""
    h, w = rgba.shape[:2]
    hx, hy, l = reach(motion, p)
    k = (f32(1) / np.where(l < f32(0.5), f32(0.5), l)).astype(f32)
    tp = far(nd[..., 3])
    with np.errstate(all="ignore"):
        iz = (f32(1) / (f32(p.depth_soft) * tp)).astype(f32)
    ok = ~bad_pixels(rgba)
    c = np.where(ok[..., None], rgba[..., :3], 0).astype(np.float64)
    N, _ = tile_lines(hx, hy, l)
    out = rgba.astype(np.float64)
    for tj in range(N.shape[0]):
        for ti in range(N.shape[1]):
            Nx, Ny, L = (f32(v) for v in N[tj, ti])
            if not L >= f32(0.5):
                continue
            n = int(np.floor(L))
            if f32(n) < L:
                n += 1
            dx, dy, ds = Nx / f32(n), Ny / f32(n), L / f32(n)
            ys, xs = np.mgrid[tj * TILE:min((tj + 1) * TILE, h), ti * TILE:min((ti + 1) * TILE, w)]
            lp, kp, tpp, izp = l[ys, xs], k[ys, xs], tp[ys, xs], iz[ys, xs]
            S, W = np.zeros(ys.shape + (3,)), np.zeros(ys.shape)
            for j in range(-n, n + 1):
                if j == 0:
                    S += kp.astype(np.float64)[..., None] * c[ys, xs]
                    W += kp.astype(np.float64)
                    continue
                ox = int(np.floor(f32(j) * dx + f32(0.5)))
                oy = int(np.floor(f32(j) * dy + f32(0.5)))
                qx, qy = xs + ox, ys + oy
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                X, Y = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                d = f32(abs(j)) * ds
                with np.errstate(all="ignore"):
                    fore = _clamp01(f32(1) - (tp[Y, X] - tpp) * izp)
                    back = _clamp01(f32(1) - (tpp - tp[Y, X]) * izp)
                    cq = np.maximum(f32(1) - d * k[Y, X], f32(0)).astype(f32)
                    cp = np.maximum(f32(1) - d * kp, f32(0)).astype(f32)
                    cy = ((d <= l[Y, X]) & (d <= lp)).astype(f32)
                    alpha = ((fore * cq + back * cp) + f32(2) * cy).astype(f32)
                alpha = np.where(inside & ok[Y, X], alpha, f32(0)).astype(np.float64)
                S += alpha[..., None] * c[Y, X]
                W += alpha
            with np.errstate(all="ignore"):
                res = S / W[..., None]
            keep = ok[ys, xs]
            out[ys, xs, :3] = np.where(keep[..., None], res, out[ys, xs, :3])
    return out, l


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
    """One bare context per library: the blur needs neither a scene nor a camera."""
    if hostsim not in _ctx:
        L = rt_amd.lib(hostsim)
        hnd = ctypes.c_void_p()
        rt_amd.check(L, L.rt_create(0, ctypes.byref(hnd)), None, "rt_create")
        _ctx[hostsim] = (L, hnd)
    return _ctx[hostsim]


def blur(rgba, nd, motion, p=None, hostsim=True, code=False, want_reach=True, **over):
    """(rgba_out, reach_out) of rt_motion_blur, or its return code. over: replacements for the call's arguments by name
    (rgba_in, nd_in, motion_in, out, reach_out, w, h)."""
    L, hnd = ctx(hostsim)
    H, W = rgba.shape[:2]
    a = dict(rgba_in=rgba, nd_in=nd, motion_in=motion, w=W, h=H, out=np.full((H, W, 4), -5.0, f32),
             reach_out=np.full((H, W), -5.0, f32) if want_reach else None)
    a.update(over)
    rc = L.rt_motion_blur(hnd, a["w"], a["h"], ptr(a["rgba_in"]), ptr(a["nd_in"]), ptr(a["motion_in"]),
                          ctypes.byref(p) if p is not None else None, ptr(a["out"]), ptr(a["reach_out"]))
    if code:
        return rc
    rt_amd.check(L, rc, hnd, "rt_motion_blur")
    return a["out"], a["reach_out"]


def vectors(cur, prev, nd, hostsim=True, code=False, **over):
    """motion_out [h, w, 2] of rt_motion_vectors with `cur` bound as the context's camera, or the return code. over:
    replacements by name (nd_in, out, w, h, prev_view, prev_fov)."""
    L, hnd = tc.ctx(hostsim, cur)
    H, W = nd.shape[:2]
    a = dict(nd_in=nd, w=W, h=H, out=np.full((H, W, 2), -5.0, f32), prev_view=prev.view_matrix, prev_fov=prev.fov_dist)
    a.update(over)
    rc = L.rt_motion_vectors(hnd, a["w"], a["h"], ptr(a["nd_in"]), ptr(a["prev_view"]), ctypes.c_float(a["prev_fov"]), ptr(a["out"]))
    if code:
        return rc
    rt_amd.check(L, rc, hnd, "rt_motion_vectors")
    return a["out"]


_host_cache = {}


def host_result(w, h, max_radius, kind):
    """hostsim's two outputs for a synthetic case at SHUTTER and DEPTH_SOFT, computed once and shared (read-only)."""
    key = (w, h, max_radius, kind)
    if key not in _host_cache:
        got = blur(*inputs(w, h), field(kind, w, h, max_radius), params(max_radius=max_radius))
        for a in got:
            a.setflags(write=False)
        _host_cache[key] = got
    return _host_cache[key]


def clean(w, h):
    """inputs() without bad colours."""
    rgba, nd = inputs(w, h)
    rgba[...] = np.where(np.isfinite(rgba), rgba, f32(0.5))
    return rgba, nd


def tie_case():
    """37 x 29, max_radius 8: everything still but two pixels of tile (0, 0) with the same l = 6 and opposite
    directions: (3, 2) moves along +x, (10, 9) along -y. The first in raster order, (3, 2), sets the line of all four
    tiles (each has tile (0, 0) among its neighbours). (rgba, nd, motion, params)."""
    rgba, nd = clean(37, 29)
    nd[..., 3] = 2.0
    m = np.zeros((29, 37, 2), f32)
    m[2, 3] = (12.0, 0.0)
    m[9, 10] = (0.0, -12.0)
    return rgba, nd, m, params(max_radius=8)


def border_case():
    """70 x 45, max_radius 16: the tile column x in [16, 32) moves by h = (12, 0) at the depth of everything else, the
    rest is still. The still tiles beside it take its line: their pixels within 12 px of the moving tile are blurred,
    which a maximum per tile alone would copy. (rgba, nd, motion, params)."""
    rgba, nd = clean(70, 45)
    nd[..., 3] = 2.0
    m = np.zeros((45, 70, 2), f32)
    m[:, 16:32] = (24.0, 0.0)
    return rgba, nd, m, params(max_radius=16)
