"""Hand-made meshes and ray sets for the per-trip code of the search-BVH walks (tests/test_trip_code.py on
the CPU build, tests/test_trip_code_gpu.py on the gfx950 library; tools/gen_golden_trip.py records what the
build before the branch-free push / pop did with them).

 * grid: 64 triangles, one per cell of a 4 x 4 x 4 grid, each spanning its whole cell, so the boxes are
   the cells. Axis-parallel rays through cell centres and in the planes between cells (the grid's symmetry
   planes: neighbouring boxes are entered at equal distances, tied keys), diagonals from the corners.
 * strip: 2048 thin triangles side by side: a long run of boxes that a ray along it keeps open.
 * chain: 1600 parallel triangles whose spacing grows by 1 % from one to the next. The builder's tree over
   it is deep and skewed; a ray along the axis holds up to three open entries per level, and, depending on
   where it starts, stops at every stack depth up to the capacity and beyond it.
"""
from __future__ import annotations

import ctypes
import hashlib
import os

import numpy as np

import golden_io as gio

MESHES = ["grid", "strip", "chain"]
GOLDEN = os.path.join(gio.GOLDEN, "trip_code_parent.npz")
CAP = 32  # RT_QSTACK: stack entries of a quad
_cache: dict = {}


def mesh(name: str) -> np.ndarray:
    """[N, 9] float32."""
    if name == "grid":
        t = []
        for z in range(4):
            for y in range(4):
                for x in range(4):
                    o = np.array([x, y, z], np.float64)
                    t.append([o, o + (1.0, 1.0, 0.0), o + (0.0, 1.0, 1.0)])
        t = np.asarray(t)
    elif name == "strip":
        n = 2048
        x = np.arange(n, dtype=np.float64) * 0.01
        t = np.stack([np.stack([x, np.zeros(n), np.zeros(n)], 1),
                      np.stack([x + 0.01, np.ones(n), np.full(n, 0.001)], 1),
                      np.stack([x + 0.005, np.full(n, 0.5), np.full(n, 1.0)], 1)], 1)
    else:
        x = chain_x()
        n, s = x.size, np.full(x.size, 0.5)
        t = np.stack([np.stack([x, -s, -s], 1), np.stack([x, s, -s], 1), np.stack([x + 1e-4, np.zeros(n), s], 1)], 1)
    return np.ascontiguousarray(t.reshape(-1, 9), dtype=np.float32)


def chain_x() -> np.ndarray:
    i = np.arange(1600, dtype=np.float64)
    return (1.01 ** i - 1.0) / 0.01 * 0.001


def rays(name: str) -> np.ndarray:
    """[n, 6] float32 = origin, direction."""
    r = []
    if name == "grid":
        c = np.arange(4) + 0.5
        for a in range(3):
            for u in np.concatenate([c, np.arange(5.0)]):
                for v in np.concatenate([c, np.arange(5.0)]):
                    for s in (1.0, -1.0):
                        o, d = np.zeros(3), np.zeros(3)
                        o[a], o[(a + 1) % 3], o[(a + 2) % 3] = (-0.5 if s > 0 else 4.5), u, v
                        d[a] = s
                        r.append(np.concatenate([o, d]))
        for o in [np.array([x, y, z], np.float64) for x in (-0.5, 4.5) for y in (-0.5, 4.5) for z in (-0.5, 4.5)]:
            for tx in c:
                for ty in c:
                    for tz in (0.5, 2.0, 3.5):
                        d = np.array([tx, ty, tz]) - o
                        r.append(np.concatenate([o, d / np.linalg.norm(d)]))
            d = np.array([2.0, 2.0, 2.0]) - o
            r.append(np.concatenate([o, d / np.linalg.norm(d)]))
        for p in (1.0, 2.0, 3.0):  # in a symmetry plane, diagonal within it
            for o2 in (-0.5, 4.5):
                d = np.array([1.0, 1.0, 0.0]) * (1.0 if o2 < 0 else -1.0) / np.sqrt(2.0)
                r.append(np.concatenate([[o2, o2, p], d]))
                r.append(np.concatenate([[p, o2, o2], np.roll(d, 1)]))
        r.append([10.0, 10.0, 10.0, 1.0, 0.0, 0.0])  # misses the root's children: a pop on an empty stack at depth 0
    elif name == "strip":
        n = 2048
        for y in np.linspace(0.02, 0.98, 25):
            for z in (0.0005, 0.01, 0.3, 0.9):
                for o_x, s in ((-0.5, 1.0), (n * 0.01 + 0.5, -1.0), (n * 0.005, 1.0), (n * 0.005, -1.0)):
                    r.append([o_x, y, z, s, 0.0, 0.0])
                    d = np.array([s, 0.0003, -0.0002])
                    r.append(np.concatenate([[o_x, y, z], d / np.linalg.norm(d)]))
        for i in np.linspace(0, n - 1, 96).astype(np.int64):
            c = np.array([i * 0.01 + 0.005, 0.5, 1.001 / 3.0])
            for off in ((-0.3, 0.2, 0.1), (0.05, -0.3, 0.4)):
                d = -np.asarray(off)
                r.append(np.concatenate([c + off, d / np.linalg.norm(d)]))
    else:
        x = chain_x()
        for x0 in np.concatenate([[-1.0, x.max() + 1.0], x[::2] * (1 + 1e-6) + 1e-5]):
            for s in (1.0, -1.0):
                r.append([x0, 0.01, 0.02, s, 0.0, 0.0])
    return np.ascontiguousarray(np.asarray(r), dtype=np.float32)


def rays_digest(name: str) -> str:
    return hashlib.sha256(mesh(name).tobytes() + rays(name).tobytes()).hexdigest()[:16]


def kernel(name: str, hostsim: bool):
    import rt_amd
    key = (name, hostsim)
    if key not in _cache:
        tris = mesh(name)
        mats = rt_amd.make_materials([((1.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.0, 1.0), ((0.0, 0.0, 0.0), (0.7, 0.7, 0.7), 0.0, 1.0)])
        _cache[key] = rt_amd.RenderKernel(4, 4, 1, 1, rt_amd.Image(4, 4), tris, mats, np.zeros(0, np.int32),
                                          np.ones(tris.shape[0], np.int32), None, rt_amd.BVH(tris), rt_amd.Image(1, 1),
                                          None, hostsim=hostsim)
    return _cache[key]


def exact(name: str) -> np.ndarray:
    """The exact walk's answers (CPU build), computed once."""
    key = (name, "exact")
    if key not in _cache:
        out = kernel(name, True).intersect(rays(name))
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def cases(name: str) -> np.ndarray:
    """rt_hostsim_trip_cases over rays(name): [n, 10] (rt_hostsim.cpp), computed once."""
    from rt_amd import _capi
    key = (name, "cases")
    if key not in _cache:
        r = rays(name)
        out = np.zeros((r.shape[0], 10), np.int32)
        assert _capi.lib(True).rt_hostsim_trip_cases(kernel(name, True).ctx, _capi.ptr(r), r.shape[0], _capi.ptr(out)) == 0
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def cpu_handovers(name: str) -> np.ndarray:
    """Queries the CPU build's one-lane twin of the quad walk leaves to the exact walk."""
    from rt_amd import _capi
    r = rays(name)
    t, k = np.zeros(r.shape[0], np.float32), np.zeros(r.shape[0], np.int32)
    assert _capi.lib(True).rt_hostsim_fast_queries(kernel(name, True).ctx, _capi.ptr(r), r.shape[0], _capi.ptr(t), _capi.ptr(k)) == 0
    return t == -2.0


def rays8(r: np.ndarray) -> np.ndarray:
    out = np.zeros((r.shape[0], 8), np.float32)
    out[:, 0:3], out[:, 4:7] = r[:, 0:3], r[:, 3:6]
    return out


def device_queries(rk, mode: int, r: np.ndarray):
    from rt_amd import _capi
    n = r.shape[0]
    t, k, ms = np.zeros(n, np.float32), np.zeros(n, np.int32), ctypes.c_double()
    rc = _capi.lib().rt_device_queries(rk.ctx, mode, _capi.ptr(rays8(r)), n, 1, _capi.ptr(t), _capi.ptr(k), ctypes.byref(ms))
    assert rc == 0, _capi.lib().rt_last_error(rk.ctx)
    return t, k


def device_trips(rk, any_: int, r: np.ndarray) -> np.ndarray:
    from rt_amd import _capi
    out = np.zeros((r.shape[0], 3), np.int32)
    rc = _capi.lib().rt_device_query_trips(rk.ctx, any_, _capi.ptr(rays8(r)), r.shape[0], _capi.ptr(out))
    assert rc == 0, _capi.lib().rt_last_error(rk.ctx)
    return out


def golden() -> dict:
    if "golden" not in _cache:
        _cache["golden"] = dict(np.load(GOLDEN))
    return _cache["golden"]
