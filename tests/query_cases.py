"""Ray sets and contexts shared by the ray-query tests (tests/test_query.py on the hostsim
build, tests/test_query_gpu.py on the gfx950 library)."""
from __future__ import annotations

import json
import os

import numpy as np

import golden_io as gio
import rt_cases
from conftest import load_golden, parsed_scene

import rt_amd

with open(os.path.join(gio.GOLDEN, "brute_manifest.json")) as _f:
    BRUTE = json.load(_f)

# fixture file -> (scene, brute-manifest entry that carries its spheres or None, whether the
# reference wrote its hits with USE_BVH 0)
FIXTURES = {
    "far_rays_cornell.npz": ("cornell", None, False),
    "far_rays_dragon.npz": ("dragon", None, False),
    "rays_dragon.npz": ("dragon", None, False),
    "brute_rays_dragon_tie_prone.npz": ("dragon", None, True),
    "brute_rays_cornell_edges.npz": ("cornell", None, True),
    "brute_rays_cornell_regression.npz": ("cornell", None, True),
    "brute_rays_cornell_edges_spheres.npz": ("cornell", "cornell_edges_spheres", True),
}

_kernels: dict = {}


def kernel(scene: str, hostsim: bool, spheres: str | None = None, brute: bool = False):
    """A context over `scene` (+ the analytic spheres of a brute-manifest entry), cached: the
    query tests change no state of it but the rq_variant schedule key."""
    key = (scene, hostsim, spheres, brute)
    if key not in _kernels:
        P = parsed_scene(scene)
        mats, mi, sph = P.materials.copy(), P.material_indices, None
        if spheres:
            mats, mi, sph = rt_cases.sphere_buffers(BRUTE["rays"][spheres], P, mats)
        rk = rt_amd.RenderKernel(4, 4, 1, 1, rt_amd.Image(4, 4), P.triangles, mats, P.emissive_triangle_indices, mi,
                                 sph, rt_amd.BVH(P.triangles), rt_amd.Image(1, 1), None, hostsim=hostsim)
        if brute:
            rk.set_use_bvh(False)
        _kernels[key] = rk
    return _kernels[key]


def fixture_rays(name: str) -> np.ndarray:
    return np.ascontiguousarray(load_golden(name)["rays"][:, :6], dtype=np.float32)


def scene_box(scene: str):
    v = np.asarray(parsed_scene(scene).triangles, np.float64).reshape(-1, 3)
    return v.min(0), v.max(0)


def near_masks(scene: str, o: np.ndarray, scale: float = 0.5):
    """(inside, outside) the near box with a 1e-3 guard band either way (the construction of
    tests/test_far_origin.py _near)."""
    lo, hi = scene_box(scene)
    w = scale * (hi - lo).max()
    inside = ((o >= lo - w + 1e-3) & (o <= hi + w - 1e-3)).all(1)
    outside = ((o < lo - w - 1e-3) | (o > hi + w + 1e-3)).any(1)
    return inside, outside


INBOX_SEEDS = {"cornell": 11, "dragon": 12}
_inbox: dict = {}


def inbox_rays(scene: str, n: int = 4096) -> np.ndarray:
    """The first n <= 8192 of the scene's seeded in-box rays: origins uniform inside the
    scene's box shrunk by 1 %, directions uniform on the sphere."""
    if scene not in _inbox:
        rng = np.random.default_rng(INBOX_SEEDS[scene])
        lo, hi = scene_box(scene)
        c, h = (lo + hi) / 2, (hi - lo) / 2 * 0.99
        o = c + h * rng.uniform(-1.0, 1.0, (8192, 3))
        d = rng.normal(size=(8192, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        _inbox[scene] = np.ascontiguousarray(np.concatenate([o, d], 1), dtype=np.float32)
    return _inbox[scene][:n]


def degenerate_rays(scene: str) -> np.ndarray:
    """NaN origins and directions, zero directions and +-inf components, from a point inside
    the scene's box."""
    nan, inf = np.float32("nan"), np.float32("inf")
    lo, hi = scene_box(scene)
    o = [float(x) for x in lo + (hi - lo) * np.array([0.45, 0.55, 0.4])]
    rows = []
    for i in range(3):
        a = list(o)
        a[i] = nan
        rows.append(a + [0.0, -1.0, 0.1])
        d = [0.3, -0.8, 0.2]
        d[i] = nan
        rows.append(o + d)
        for s in (inf, -inf):
            a = list(o)
            a[i] = s
            rows.append(a + [0.0, -1.0, 0.1])
            d = [0.3, -0.8, 0.2]
            d[i] = s
            rows.append(o + d)
    rows.append(o + [0.0, 0.0, 0.0])
    rows.append(o + [-0.0, 0.0, -0.0])
    rows.append([nan] * 6)
    rows.append(o + [inf, inf, -inf])
    rows.append(o + [0.0, -1.0, 0.0])  # (an ordinary ray among them)
    return np.asarray(rows, np.float32)


def _check_reference_hits(got, g, name):
    """found, prim, t, p, n of the reference-written hits (prim .. n where found)."""
    h = g["hits"]
    np.testing.assert_array_equal(got[:, 0], h["found"], err_msg=name)
    hit = h["found"] == 1
    np.testing.assert_array_equal(got[hit, 1], h["prim"][hit], err_msg=name)
    np.testing.assert_array_equal(got[hit, 2], h["t"][hit].view(np.int32), err_msg=name)
    np.testing.assert_array_equal(got[hit, 3:6], np.ascontiguousarray(h["p"][hit]).view(np.int32), err_msg=name)
    np.testing.assert_array_equal(got[hit, 6:9], np.ascontiguousarray(h["n"][hit]).view(np.int32), err_msg=name)


def check_fixture(name: str, hostsim: bool, brute_context: bool = True):
    """The comparisons every fixture gets, on either library; returns the routed call's
    exact-walk count. The context answers INTERSECT_SCENE with the octree walk; a second
    context in the mode the reference wrote the hits with where that is USE_BVH 0."""
    scene, spheres, brute_hits = FIXTURES[name]
    g = load_golden(name)
    rays = fixture_rays(name)
    n = rays.shape[0]
    rk = kernel(scene, hostsim, spheres)
    want = rk.intersect(rays)
    got = rk.query(rays, "closest")
    routed = rk.query_last_exact()
    np.testing.assert_array_equal(got, want, err_msg=f"{name}: closest")
    np.testing.assert_array_equal(rk.query(rays, "any"), want[:, 0], err_msg=f"{name}: any")
    assert rk.query_last_exact() >= (n if spheres else 0)
    np.testing.assert_array_equal(rk.query(rays, "closest", exact=True), want, err_msg=f"{name}: exact closest")
    assert rk.query_last_exact() == n
    np.testing.assert_array_equal(rk.query(rays, "any", exact=True), want[:, 0], err_msg=f"{name}: exact any")
    assert rk.query_last_exact() == n
    if spheres:
        assert routed == n, f"{name}: a sphere context sends every query to the exact walk"
    if not brute_hits:
        _check_reference_hits(got, g, name)
    elif brute_context:
        rb = kernel(scene, hostsim, spheres, brute=True)
        gb = rb.query(rays, "closest")
        assert rb.query_last_exact() == n, f"{name}: brute mode sends every query to the exact walk"
        np.testing.assert_array_equal(gb, rb.intersect(rays), err_msg=f"{name}: brute closest")
        _check_reference_hits(gb, g, name + " (USE_BVH 0)")
        np.testing.assert_array_equal(rb.query(rays, "any"), g["hits"]["found"], err_msg=f"{name}: brute any")
        assert rb.query_last_exact() == n
    return routed
