"""The per-query work around the search-BVH walks (rt_quad.h, rt_row.h): the occlusion walks'
leaf verification (the ray's terms once per leaf visit, one check per octree leaf, one loop over
the hit lanes), the walks compiled with and without the USE_BVH 0 bookkeeping, and the drain
hand-over. Answers are the exact walk's (rt_intersect), bit for bit.

Ray sets: the reference-pinned dragon rays, the tie-prone rays, and rays aimed at shared
vertices and edge midpoints of the Cornell box and the dragon. The reference side decides which
of the aimed rays are in a set: rt_hostsim_leaf_hits walks the whole search BVH under a ray on
the CPU and counts, per leaf visit (a pack of up to four triangles, one per lane of a quad), the
lanes whose Moller-Trumbore test hits and their octree leaves. A ray stays when some leaf visit
has two or more hit lanes; every set must hold rays with hit lanes in one octree leaf (the
skipped check), in different leaves (a second pass of the loop) and with a first checked leaf
that fails (the pass after a failed check)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import query_cases as qc
import rt_cases
from conftest import parsed_scene

import rt_amd
from rt_amd import _capi

FIXTURES = ["rays_dragon.npz", "brute_rays_dragon_tie_prone.npz"]
N_TARGET_TRIS = 4096  # triangles whose vertices and edge midpoints are aimed at: 6 targets each, 3 origins
N_EDGE_RAYS = 2048    # rays kept per scene at most
_edge: dict = {}


def leaf_hits(scene: str, rays: np.ndarray) -> np.ndarray:
    """Per ray: most hit lanes in one leaf visit; visits with hit lanes in one octree leaf; in
    different leaves; of those, visits whose first hit lane's leaf fails its chain check."""
    out = np.zeros((rays.shape[0], 4), np.int32)
    rk = qc.kernel(scene, hostsim=True)
    assert _capi.lib(True).rt_hostsim_leaf_hits(rk.ctx, _capi.ptr(rays), rays.shape[0], _capi.ptr(out)) == 0
    return out


def edge_rays(scene: str) -> np.ndarray:
    """Rays from three points inside the scene's box through the vertices and edge midpoints of
    evenly spaced triangles, kept where a leaf visit has two or more hit lanes (leaf_hits); at
    most N_EDGE_RAYS, the rays with a failing first leaf first, then different leaves, then the rest."""
    if scene not in _edge:
        tris = np.asarray(parsed_scene(scene).triangles, np.float64).reshape(-1, 3, 3)
        pick = tris[np.linspace(0, tris.shape[0] - 1, min(N_TARGET_TRIS, tris.shape[0])).astype(np.int64)]
        targets = np.concatenate([pick.reshape(-1, 3), ((pick + np.roll(pick, 1, axis=1)) / 2).reshape(-1, 3)])
        lo, hi = qc.scene_box(scene)
        rays = []
        for f in ((0.5, 0.5, 0.5), (0.3, 0.6, 0.7), (0.7, 0.35, 0.45)):
            o = lo + (hi - lo) * np.asarray(f)
            d = targets - o
            dist = np.linalg.norm(d, axis=1)
            ok = dist > 1e-6
            rays.append(np.concatenate([np.broadcast_to(o, d.shape)[ok], d[ok] / dist[ok, None]], 1))
        rays = np.ascontiguousarray(np.concatenate(rays), dtype=np.float32)
        h = leaf_hits(scene, rays)
        keep = np.flatnonzero(h[:, 0] >= 2)
        order = np.lexsort((keep, -(h[keep, 2] > 0).astype(np.int64), -(h[keep, 3] > 0).astype(np.int64)))
        keep = keep[order][:N_EDGE_RAYS]
        # (the cut keeps a third of its places for the rays whose hit lanes share a leaf)
        same = np.flatnonzero((h[:, 0] >= 2) & (h[:, 1] > 0))[:N_EDGE_RAYS // 3]
        keep = np.unique(np.concatenate([keep[:N_EDGE_RAYS - same.size], same]))
        _edge[scene] = np.ascontiguousarray(rays[keep])
    return _edge[scene]


def ray_set(name: str) -> tuple[str, np.ndarray]:
    if name.startswith("edges_"):
        scene = name[len("edges_"):]
        return scene, edge_rays(scene)
    return qc.FIXTURES[name][0], qc.fixture_rays(name)


RAY_SETS = FIXTURES + ["edges_cornell", "edges_dragon"]


@pytest.mark.parametrize("name", RAY_SETS)
def test_ray_sets_have_multi_hit_leaf_visits(name):
    """Every set reaches the skipped check, the loop's second pass and the pass after a failed
    check; the edge / vertex sets hold nothing else, and reach three or four hit lanes."""
    scene, rays = ray_set(name)
    h = leaf_hits(scene, rays)
    occluded = qc.kernel(scene, hostsim=True).intersect(rays)[:, 0] == 1
    print(f"{name}: {rays.shape[0]} rays, most hit lanes {h[:, 0].max()}, one leaf {(h[:, 1] > 0).sum()}, "
          f"different leaves {(h[:, 2] > 0).sum()}, first leaf fails {(h[:, 3] > 0).sum()}, "
          f"unoccluded with different leaves {((h[:, 2] > 0) & ~occluded).sum()}")
    assert (h[:, 1] > 0).any() and (h[:, 2] > 0).any() and (h[:, 3] > 0).any()
    if name.startswith("edges_"):
        assert rays.shape[0] >= 64 and (h[:, 0] >= 2).all() and h[:, 0].max() >= 3


@pytest.mark.parametrize("name", RAY_SETS)
def test_hostsim_walks_equal_exact_walk(name):
    """The CPU build's walks (rt_fast.h, one lane; the quads' and rows' twin) on the same sets."""
    scene, rays = ray_set(name)
    rk = qc.kernel(scene, hostsim=True)
    want = rk.intersect(rays)
    np.testing.assert_array_equal(rk.query(rays, "closest"), want, err_msg=f"{name}: closest (t, k)")
    np.testing.assert_array_equal(rk.query(rays, "any"), want[:, 0], err_msg=f"{name}: occlusion")


def _device_queries(rk, mode, rays):
    n = rays.shape[0]
    rays8 = np.zeros((n, 8), np.float32)
    rays8[:, 0:3], rays8[:, 4:7] = rays[:, 0:3], rays[:, 3:6]
    t, k, ms = np.zeros(n, np.float32), np.zeros(n, np.int32), ctypes.c_double()
    rc = _capi.lib().rt_device_queries(rk.ctx, mode, _capi.ptr(rays8), n, 1, _capi.ptr(t), _capi.ptr(k), ctypes.byref(ms))
    assert rc == 0, _capi.lib().rt_last_error(rk.ctx)
    return t, k


@pytest.mark.gpu
@pytest.mark.parametrize("name", RAY_SETS)
def test_gpu_quad_and_row_walks_equal_exact_walk(name):
    """The quad walks (rt_device_queries modes 4 closest, 5 occlusion) and the row walks (8, 9): every
    answer a walk settles is the exact walk's, bit for bit, and rows and quads hand the same queries to
    the exact walk (an occlusion walk only on a stack overflow: under 1 % of any set)."""
    scene, rays = ray_set(name)
    rk = qc.kernel(scene, hostsim=False)
    want = qc.kernel(scene, hostsim=True).intersect(rays)
    want_t = np.where(want[:, 0] == 1, want[:, 2].view(np.float32), np.float32(-1.0)).astype(np.float32)
    want_k = np.where(want[:, 0] == 1, want[:, 1], -1)
    verdicts = []
    for mode, what in ((4, "quad"), (8, "row")):
        t, k = _device_queries(rk, mode, rays)
        ok = t != -2.0
        assert ok.any(), f"{name}: {what} closest settles nothing"
        np.testing.assert_array_equal(t[ok].view(np.uint32), want_t[ok].view(np.uint32), err_msg=f"{name}: {what} closest t")
        np.testing.assert_array_equal(k[ok], want_k[ok], err_msg=f"{name}: {what} closest k")
        verdicts.append(ok)
    np.testing.assert_array_equal(verdicts[0], verdicts[1], err_msg=f"{name}: hand-overs, rows vs quads")
    flags = []
    for mode, what in ((5, "quad"), (9, "row")):
        a, _ = _device_queries(rk, mode, rays)
        ok = a != -2.0  # (-2: the bounded stack overflowed, the exact walk answers)
        assert ok.mean() >= 0.99, f"{name}: {what} occlusion settles {ok.mean():.3f}"
        np.testing.assert_array_equal(a[ok], want[ok, 0].astype(np.float32), err_msg=f"{name}: {what} occlusion")
        flags.append(a)
    np.testing.assert_array_equal(flags[0], flags[1], err_msg=f"{name}: occlusion, rows vs quads")


@pytest.mark.gpu
@pytest.mark.parametrize("name", RAY_SETS)
def test_gpu_walks_equal_exact_walk(name):
    """rt_query_device, each kernel variant (the product's, plain rounds, per-quad refill), against the
    exact walk on the CPU (hostsim rt_intersect) and on the GPU."""
    from hip_mem import DeviceBuffer
    scene, rays = ray_set(name)
    n = rays.shape[0]
    rk = qc.kernel(scene, hostsim=False)
    want = qc.kernel(scene, hostsim=True).intersect(rays)
    np.testing.assert_array_equal(rk.intersect(rays), want, err_msg=f"{name}: exact walks, GPU vs CPU")
    d_rays = DeviceBuffer(rays.nbytes)
    d_rays.upload(rays)
    try:
        for v in (0, 1, 2):
            rk.test_schedule(rq_variant=v)
            for mode, words, w in (("closest", 11, want), ("any", 1, want[:, 0])):
                d_out = DeviceBuffer(n * words * 4)
                d_out.upload(np.full(n * words, 0x5A5A5A5A, np.int32))
                rk.query_device(d_rays.ptr, n, d_out.ptr, mode=mode)
                got = d_out.download((n * words,), np.int32).reshape(w.shape)
                np.testing.assert_array_equal(got, w, err_msg=f"{name}: {mode}, variant {v}")
    finally:
        rk.test_schedule(rq_variant=0)


@pytest.mark.gpu
def test_gpu_cfg1_bitwise(manifest, cameras):
    e = rt_cases.golden_case("cfg1_cornell12", manifest)
    assert (e["W"], e["H"], e["spp"], e["bounces"]) == (256, 256, 4, 3)
    got = rt_cases.run_case(e, cameras, hostsim=False)
    np.testing.assert_array_equal(got.view(np.uint32), e["expected"].view(np.uint32))


_dragon_ref: dict = {}


def _dragon_frame(manifest, cameras, hostsim, **schedule):
    e = rt_cases.golden_case("cfg2_dragon", manifest)
    e["px"] = None
    rk, fb = rt_cases.make_kernel(e, cameras, hostsim=hostsim, W=64, H=36, spp=4, bounces=8)
    if schedule:
        rk.test_schedule(**schedule)
    rk.render()
    return fb.pixels.copy()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,tail", [(1, 0), (1, 4), (3, 0), (3, 4)])
def test_gpu_dragon_frame_bitwise_vs_hostsim(lanes, tail, manifest, cameras):
    """64x36x4spp x8 on the dragon: k_trace's quads, its drain's rows and (tail on) k_tail."""
    if "ref" not in _dragon_ref:
        _dragon_ref["ref"] = _dragon_frame(manifest, cameras, hostsim=True)
    got = _dragon_frame(manifest, cameras, hostsim=False, lanes=lanes, tail_paths=tail)
    assert np.isfinite(got[..., :3]).any()
    np.testing.assert_array_equal(got.view(np.uint32), _dragon_ref["ref"].view(np.uint32))


@pytest.mark.gpu
def test_gpu_brute_cornell_frame_bitwise_vs_hostsim(manifest, cameras):
    """USE_BVH 0: k_trace's second instantiation (the walks that keep the original indices)."""
    e = rt_cases.golden_case("cfg1_cornell12", manifest)
    frames = []
    for hostsim in (True, False):
        rk, fb = rt_cases.make_kernel(e, cameras, hostsim=hostsim, W=32, H=32, spp=2)
        rk.set_use_bvh(False)
        rk.render()
        frames.append(fb.pixels.copy())
    assert np.isfinite(frames[1][..., :3]).any() and frames[1][..., :3].any()
    np.testing.assert_array_equal(frames[1].view(np.uint32), frames[0].view(np.uint32))
