"""The geometry zoo: small seeded meshes with the hazards the Cornell box, the MIS scene and the
dragon stand-in do not have (zero-area triangles and slivers, duplicated and coplanar overlapping
triangles, a high-valence vertex, zero extent on an axis, coordinates far from the origin and far
below 1, size ratios of 1e6), their ray sets, material tables and cameras. Shared by
tests/test_zoo.py (hostsim and oracle), tests/test_zoo_gpu.py (gfx950) and
tools/gen_golden_zoo.py (the reference's answers, tests/golden/zoo_*.npz).

Pure numpy: every array is computed in float64 from a seeded generator and rounded to float32
once, so the same bytes come out everywhere."""
from __future__ import annotations

import numpy as np

SCENES = ["soup", "mix", "offset", "tiny", "slivers", "dup", "flat", "grid", "fan"]
# octree (max_depth, leaf_max): the product's, shallow with small leaves, one triangle per leaf,
# a root that splits once, leaves larger than any search-BVH pack
SETTINGS = [(32, 8), (3, 2), (12, 1), (1, 8), (32, 64)]
SEEDS = {"soup": 101, "mix": 102, "slivers": 105, "dup": 106, "flat": 107, "rays": 900}
OFFSET = (4096.0, -2048.0, 8192.0)
N_RAYS = 4096
FRAME = dict(W=40, H=30, spp=2, bounces=4, sky="S")
# Camera(90 degrees): 1 / tan(fov / 2) in the reference's float arithmetic (camera.h:27-31),
# recorded from its `camera` dump (tests/golden/zoo_*.npz hold the whole matrix)
FOV, FOV_DIST_BITS = 90.0, 0x3F800000

_tris: dict = {}
_rays: dict = {}


def _soup(rng, n, smin=1e-3, smax=0.5, box=2.0):
    """n random triangles: centres uniform in the box, sizes log-uniform in [smin, smax]."""
    c = rng.uniform(-box / 2, box / 2, (n, 1, 3))
    s = np.exp(rng.uniform(np.log(smin), np.log(smax), (n, 1, 1)))
    return c + s * rng.uniform(-0.5, 0.5, (n, 3, 3))


def _build(name: str) -> np.ndarray:
    if name in ("soup", "offset", "tiny"):
        t = _soup(np.random.default_rng(SEEDS["soup"]), 3000)
        if name == "offset":
            t = t * 100.0 + np.asarray(OFFSET)
        if name == "tiny":
            t = t * 1e-3
        return t
    rng = np.random.default_rng(SEEDS.get(name, 0))
    if name == "mix":
        small = _soup(rng, 1500, 1e-4, 1e-3)
        big = rng.uniform(-1.0, 1.0, (4, 1, 3)) + rng.uniform(50.0, 100.0, (4, 1, 1)) * rng.uniform(-0.5, 0.5, (4, 3, 3))
        # (the large ones in the middle of the buffer, not at either end)
        return np.concatenate([small[:700], big, small[700:]])
    if name == "slivers":
        t = _soup(rng, 2000, 1e-2, 0.5)
        a, b = t[:, 0], t[:, 1]
        t[:, 2] = a + rng.uniform(0.0, 1.0, (2000, 1)) * (b - a) + rng.uniform(-1e-6, 1e-6, (2000, 3)) / np.sqrt(3.0)
        i = np.arange(2000)
        t[i % 7 == 0, 1] = t[i % 7 == 0, 0]  # two equal vertices
        point = i % 7 == 3
        t[point, 1] = t[point, 0]            # collapsed to a point
        t[point, 2] = t[point, 0]
        return t
    if name == "dup":
        s = _soup(rng, 1000, 1e-2, 0.5)
        # four copies: as is, shuffled, the list reversed, the winding reversed
        return np.concatenate([s, s[rng.permutation(1000)], s[::-1], s[:, [0, 2, 1]]])
    if name == "flat":
        # (large enough to overlap many deep: a ray through the plane meets a stack of equal t)
        t = _soup(rng, 3000, 0.1, 0.5)
        t[:, :, 1] = 0.0
        return t
    if name == "grid":
        # 16 x 16 quads of side 2^-3 in the planes y = 0 and x = 0 (which cross along the z axis),
        # every vertex on the 2^-3 lattice; the y = 0 layer a second time at the end of the buffer
        k = 0.125
        u, v = np.meshgrid(np.arange(16) * k - 1.0, np.arange(16) * k - 1.0, indexing="ij")
        u, v = u.ravel(), v.ravel()
        z0 = np.zeros_like(u)

        def quads(p00, p10, p11, p01):
            return np.concatenate([np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)])

        def layer(axes):
            def pt(a, b):
                cols = [None, None, None]
                cols[axes[0]], cols[axes[1]], cols[axes[2]] = a, b, z0
                return np.stack(cols, 1)
            return quads(pt(u, v), pt(u + k, v), pt(u + k, v + k), pt(u, v + k))

        ly, lx = layer((0, 2, 1)), layer((1, 2, 0))
        return np.concatenate([ly, lx, ly])
    if name == "fan":
        # a cone: 512 triangles around the apex (0, 1, 0), the base ring at y = 0, radius 1
        a = 2.0 * np.pi * np.arange(513) / 512
        ring = np.stack([np.cos(a), np.zeros(513), np.sin(a)], 1)
        ring[512] = ring[0]
        apex = np.broadcast_to(np.array([0.0, 1.0, 0.0]), (512, 3))
        return np.stack([apex, ring[1:], ring[:-1]], 1)
    raise KeyError(name)


def triangles(name: str) -> np.ndarray:
    """[N, 9] float32."""
    if name not in _tris:
        t = np.ascontiguousarray(_build(name).reshape(-1, 9), dtype=np.float32)
        t.setflags(write=False)
        _tris[name] = t
    return _tris[name]


def box(name: str):
    v = triangles(name).astype(np.float64).reshape(-1, 3)
    return v.min(0), v.max(0)


def materials(name: str):
    """(materials [4, 10], material indices [N], emissive triangle indices): a diffuse, a rough
    metal and an emissive material by index % 3, behind the default material that parse_obj puts
    at index 0 (utils.cpp:16-98), so that the tables are what the scene's OBJ / MTL parses to."""
    import rt_amd
    mats = rt_amd.make_materials([((1.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.0, 1.0),
                                  ((0.0, 0.0, 0.0), (0.75, 0.6, 0.45), 0.0, 1.0),
                                  ((0.0, 0.0, 0.0), (0.9, 0.85, 0.7), 1.0, 0.4),
                                  ((6.0, 5.0, 4.0), (0.5, 0.5, 0.5), 0.0, 1.0)])
    n = triangles(name).shape[0]
    mi = (1 + np.arange(n) % 3).astype(np.int32)
    return mats, mi, np.flatnonzero(mi == 3).astype(np.int32)


def rays(name: str) -> np.ndarray:
    """[N_RAYS, 6] float32 = origin, direction. Origins in the scene's box widened by 10 % of its
    largest extent; 8 of 10 aimed at a vertex, an edge midpoint or an interior point of a random
    triangle; 1 of 10 axis-parallel through such a target (exact zeros of both signs in the
    direction); 1 of 10 starting on a triangle (a bounce ray). Shuffled, so that any prefix holds
    every kind."""
    if name in _rays:
        return _rays[name]
    rng = np.random.default_rng([SEEDS["rays"], SCENES.index(name)])
    t = triangles(name).astype(np.float64).reshape(-1, 3, 3)
    lo, hi = box(name)
    w = 0.1 * (hi - lo).max()
    n = N_RAYS
    pick = t[rng.integers(0, t.shape[0], n)]
    kind = rng.integers(0, 3, n)  # 0 vertex, 1 edge midpoint, 2 interior
    bary = rng.dirichlet((1.0, 1.0, 1.0), n)
    corner = rng.integers(0, 3, n)
    vert = np.eye(3)[corner]
    mid = (np.eye(3)[corner] + np.eye(3)[(corner + 1) % 3]) / 2
    wgt = np.where((kind == 0)[:, None], vert, np.where((kind == 1)[:, None], mid, bary))
    target = (wgt[:, :, None] * pick).sum(1)
    o = rng.uniform(lo - w, hi + w, (n, 3))
    d = target - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    role = rng.permutation(n) % 10
    # axis-parallel: the origin is the target moved along one axis
    ax = role == 0
    axis = rng.integers(0, 3, n)
    oa = target.copy()
    oa[np.arange(n), axis] = o[np.arange(n), axis]
    sign = np.where(target[np.arange(n), axis] >= oa[np.arange(n), axis], 1.0, -1.0)
    da = np.where(rng.integers(0, 2, (n, 3)) == 1, -0.0, 0.0)
    da[np.arange(n), axis] = sign
    o[ax], d[ax] = oa[ax], da[ax]
    # bounce rays: from the target point itself, any direction
    bo = role == 1
    db = rng.normal(size=(n, 3))
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    o[bo], d[bo] = target[bo], db[bo]
    r = np.ascontiguousarray(np.concatenate([o, d], 1), dtype=np.float32)
    r.setflags(write=False)
    _rays[name] = r
    return r


def camera(name: str) -> np.ndarray:
    """camera17 (view matrix row-major + fov_dist) of Camera(90, Translation(p)): the reference's
    default axes (looking down -z), p above and in front of the centroid at a quarter of the
    largest extent beyond the box, inside the near box."""
    lo, hi = box(name)
    ext = (hi - lo).max()
    c = triangles(name).astype(np.float64).reshape(-1, 3).mean(0)
    p = np.array([c[0], c[1] + 0.15 * ext, hi[2] + 0.25 * ext]).astype(np.float32)
    m = np.eye(4, dtype=np.float32)
    m[2, 2] = -1.0
    m[:3, 3] = p
    return np.concatenate([m.ravel(), np.array([FOV_DIST_BITS], np.uint32).view(np.float32)]).astype(np.float32)


def camera_spec(name: str) -> str:
    """The same camera as oracle/ref/ref_driver.cpp's "tele:fov:rx:tx:ty:tz"."""
    p = camera(name)[[3, 7, 11]]
    return "tele:%.9g:0:%.9g:%.9g:%.9g" % (FOV, p[0], p[1], p[2])


_kernels: dict = {}


def kernel(name: str, hostsim: bool, setting=(32, 8), brute: bool = False, frame: bool = False):
    """A context over the scene with the octree built at `setting`, cached. frame: sized and lit
    for FRAME, with the scene's camera and its own image (rk.frame_buffer); else a 4 x 4 context for
    ray calls. Tests leave its schedule as they found it."""
    import rt_amd
    import rt_cases
    key = (name, hostsim, tuple(setting), brute, frame)
    if key not in _kernels:
        mats, mi, em = materials(name)
        tris = triangles(name)
        W, H, spp, nb = (FRAME["W"], FRAME["H"], FRAME["spp"], FRAME["bounces"]) if frame else (4, 4, 1, 1)
        sky = rt_amd.Image.from_rgb(rt_cases.sky(FRAME["sky"])) if frame else rt_amd.Image(1, 1)
        rk = rt_amd.RenderKernel(W, H, spp, nb, rt_amd.Image(W, H), tris, mats, em, mi, None,
                                 rt_amd.BVH(tris, setting[0], setting[1]), sky, None, hostsim=hostsim)
        if brute:
            rk.set_use_bvh(False)
        if frame:
            c = camera(name)
            rk.set_camera(rt_amd.Camera(c[:16], c[16]))
        _kernels[key] = rk
    return _kernels[key]


def render(rk) -> np.ndarray:
    """A fresh frame of a frame context."""
    rk.frame_buffer.pixels[...] = np.array([0.0, 0.0, 0.0, 1.0], np.float32)
    rk.render()
    return rk.frame_buffer.pixels.copy()


_oracles: dict = {}


def oracle(name: str, setting=(32, 8), brute: bool = False):
    import rt_cases
    from oracle_bindings import OracleScene
    key = (name, tuple(setting), brute)
    if key not in _oracles:
        mats, mi, em = materials(name)
        S = OracleScene(triangles(name), mi, mats, em, env=rt_cases.sky(FRAME["sky"]), max_depth=setting[0],
                        leaf_max=setting[1])
        if brute:
            S.set_use_bvh(False)
        _oracles[key] = S
    return _oracles[key]


_oracle_out: dict = {}


def oracle_intersect(name: str, setting=(32, 8), brute: bool = False) -> np.ndarray:
    """The oracle's answers for rays(name), computed once."""
    key = (name, tuple(setting), brute)
    if key not in _oracle_out:
        out = oracle(name, setting, brute).intersect(rays(name))
        out.setflags(write=False)
        _oracle_out[key] = out
    return _oracle_out[key]


_oracle_frames: dict = {}


def oracle_frame(name: str, setting=(32, 8), brute: bool = False) -> np.ndarray:
    key = (name, tuple(setting), brute)
    if key not in _oracle_frames:
        fb, _ = oracle(name, setting, brute).render(camera(name), FRAME["W"], FRAME["H"], FRAME["spp"], FRAME["bounces"])
        fb.setflags(write=False)
        _oracle_frames[key] = fb
    return _oracle_frames[key]


def leaf_hits(name: str, setting=(32, 8)) -> np.ndarray:
    """rt_hostsim_leaf_hits over rays(name): [n, 4], see tests/test_trace_fixed_cost.py."""
    from rt_amd import _capi
    r = rays(name)
    out = np.zeros((r.shape[0], 4), np.int32)
    rk = kernel(name, True, setting)
    assert _capi.lib(True).rt_hostsim_leaf_hits(rk.ctx, _capi.ptr(r), r.shape[0], _capi.ptr(out)) == 0
    return out


# ---------------------------------------------------------------- the float64 check
EPS = float(np.float32(0.0000001))  # triangle.h:18
MARGIN = 1e-4
DET_REL = 1e-6
T_REL = 1e-5
# Rounding of the float32 Moller-Trumbore the float64 one is compared with: each of det, u, v, t is
# a dot of a cross product, a handful of roundings of 2^-24 relative to the product of the lengths
# that enter it (not to the result: the cross products cancel), so
#   |d det| <= C ulp |e1||d||e2|,  |d u| <= (C ulp |s||d||e2| + |u||d det|) / |det|,  v and t alike.
# MARGIN alone is below that wherever |det| is near the absolute EPSILON (a 1e-3 triangle seen
# from 2 units away: |d u| ~ 1e-3), so every margin below is MARGIN plus the bound, C = 8.
ULP, C_ERR = 2.0 ** -24, 8.0


def mt64(tris: np.ndarray, r: np.ndarray, chunk: int = 256):
    """Moller-Trumbore (triangle.h:16-60, the same tests in the same order) in float64 over every
    triangle, buffer order, first of equal t. Returns (found, prim, t, unambiguous).

    A triangle is "surely accepted" when every test passes with its margin to spare: barycentrics
    MARGIN + rounding inside, |det| above (1 + MARGIN) EPS + rounding and above DET_REL |e1||e2||d|,
    t above EPS + MARGIN x the scene's largest extent + rounding, and t's rounding below half of
    T_REL; "possibly accepted" when every test passes loosened by the same margins. A hit is
    unambiguous when its triangle is surely accepted and no other possibly accepted triangle can
    have t below (1 + MARGIN) x its t; a miss when no triangle is possibly accepted."""
    t3 = tris.astype(np.float64).reshape(-1, 3, 3)
    a, e1, e2 = t3[:, 0], t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0]
    l1, l2 = np.linalg.norm(e1, axis=1)[None], np.linalg.norm(e2, axis=1)[None]
    v = t3.reshape(-1, 3)
    ext = (v.max(0) - v.min(0)).max()
    n = r.shape[0]
    found, prim = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    tt, unamb = np.full(n, -1.0), np.zeros(n, bool)
    k_err = C_ERR * ULP
    for s in range(0, n, chunk):
        o = r[s:s + chunk, None, 0:3].astype(np.float64)
        d = r[s:s + chunk, None, 3:6].astype(np.float64)
        h = np.cross(d, e2[None])
        det = (e1[None] * h).sum(-1)
        sv = o - a[None]
        q = np.cross(sv, e1[None])
        dl, sl = np.linalg.norm(d, axis=-1), np.linalg.norm(sv, axis=-1)
        ad = np.abs(det)
        e_det = k_err * l1 * l2 * dl
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 / det
            u = f * (sv * h).sum(-1)
            w = f * (d * q).sum(-1)
            t = f * (e2[None] * q).sum(-1)
            m_u = MARGIN + (k_err * sl * dl * l2 + np.abs(u) * e_det) / ad
            m_w = MARGIN + (k_err * sl * dl * l1 + np.abs(w) * e_det) / ad
            e_t = (k_err * sl * l1 * l2 + np.abs(t) * e_det) / ad
        bad = ~np.isfinite(u) | ~np.isfinite(w) | ~np.isfinite(t)  # det = 0
        acc = ~bad & (ad >= EPS) & (u >= 0) & (u <= 1) & (w >= 0) & (u + w <= 1) & (t > EPS)
        sure = (acc & (ad >= EPS * (1 + MARGIN) + e_det) & (ad >= DET_REL * l1 * l2 * dl) & (u >= m_u) & (w >= m_w) &
                (u + w <= 1 - m_u - m_w) & (t - e_t > EPS + MARGIN * ext) & (e_t <= 0.5 * T_REL * np.abs(t)))
        live = ad + e_det >= EPS * (1 - MARGIN)  # (else float32 rejects it at the first test)
        maybe = acc | (live & (bad | ((u >= -m_u) & (u <= 1 + m_u) & (w >= -m_w) & (u + w <= 1 + m_u + m_w) &
                                      (t + e_t > -MARGIN * ext))))
        ta = np.where(acc, t, np.inf)
        k = ta.argmin(1)
        rows = np.arange(ta.shape[0])
        hit = np.isfinite(ta[rows, k])
        tb = np.where(hit, ta[rows, k], np.inf)
        eb = np.where(hit, e_t[rows, k], 0.0)
        t_low = np.where(bad, -np.inf, t - e_t)
        rivals = maybe & (t_low <= ((tb + eb) * (1 + MARGIN))[:, None])
        rivals[rows, k] = False
        ok = np.where(hit, sure[rows, k] & ~rivals.any(1), ~maybe.any(1))
        found[s:s + chunk] = hit
        prim[s:s + chunk] = np.where(hit, k, -1)
        tt[s:s + chunk] = np.where(hit, tb, -1.0)
        unamb[s:s + chunk] = ok
    return found, prim, tt, unamb


# ---------------------------------------------------------------- the scene as OBJ / MTL
def write_obj(name: str, directory: str) -> str:
    """zoo_<name>.obj and .mtl in `directory`: three vertices per triangle, %.9g (which reads
    back to the same float32), the material tables of materials(name). Returns the OBJ's path."""
    import os
    os.makedirs(directory, exist_ok=True)
    mats, mi, _ = materials(name)
    with open(os.path.join(directory, f"zoo_{name}.mtl"), "w") as f:
        for k, m in list(enumerate(mats))[1:]:
            f.write("newmtl m%d\nKe %.9g %.9g %.9g\nKd %.9g %.9g %.9g\nillum 1\nPm %.9g\nPr %.9g\n\n" %
                    (k, m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9]))
    t = triangles(name)
    path = os.path.join(directory, f"zoo_{name}.obj")
    with open(path, "w") as f:
        f.write(f"mtllib zoo_{name}.mtl\no zoo_{name}\n")
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in t.reshape(-1, 3)))
        f.write("".join("usemtl m%d\nf %d %d %d\n" % (mi[i], 3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(t.shape[0])))
    return path
