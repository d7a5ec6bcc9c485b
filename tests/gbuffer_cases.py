"""Contexts, sizes and expected records shared by the G-buffer tests (tests/test_gbuffer.py on the hostsim
build, tests/test_gbuffer_gpu.py on the gfx950 library): rt_render_gbuffer against the records derived in
numpy from rt_query(CLOSEST) on rt_camera_rays and against rt_render_features."""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np

import golden_io as gio
import query_cases as qc
import rt_cases
from conftest import parsed_scene

import rt_amd

SCENES = ("cornell", "dragon")  # (each under its preset camera of the same name, as the feature tests)
# (scene, kind of kernel()): the presets, and Cornell from inside the near box, where the search-BVH walks answer
CASES = [("cornell", "plain"), ("dragon", "plain"), ("cornell", "near")]
CPU_SIZES = [(1, 1), (5, 3), (130, 67)]
# one short of and one past a wave's 16-pixel round, a block's 64 quads and 256, then several blocks of odd rows
GPU_SIZES = [(1, 1), (5, 3), (15, 1), (17, 1), (65, 1), (257, 1), (130, 67)]
BIG = (130, 67)
FAR_SIZE = (33, 9)
# gb_force_every -> entries of the fallback list at 130 x 67 (8710 pixels): ceil(8710 / N), either side of
# one octet (1), one wave of octets (7, 9), one block of octets (33) and several blocks (257); 1: every pixel
FORCE = {8710: 1, 1400: 7, 1000: 9, 270: 33, 34: 257, 1: 8710}

_cameras = np.load(os.path.join(gio.GOLDEN, "cameras.npz"))
with open(os.path.join(gio.GOLDEN, "brute_manifest.json")) as _f:
    _BRUTE = json.load(_f)

_kernels: dict = {}


def camera(scene: str, kind: str = "plain") -> rt_amd.Camera:
    """The scene's preset camera; "far": moved back along its view axis by three times the scene's largest
    extent, outside the near box; "near": moved forward by 0.8 of that extent (Cornell's preset stands outside
    the near box, so its pixels all take the exact walk: this one stands inside)."""
    c = np.asarray(_cameras[scene], np.float32)
    if kind not in ("far", "near"):
        return rt_amd.Camera(c[:16], c[16])
    m = c[:16].astype(np.float64).reshape(4, 4).copy()
    lo, hi = qc.scene_box(scene)
    axis = m[:3, 2] / np.linalg.norm(m[:3, 2])
    m[:3, 3] += (-3.0 if kind == "far" else 0.8) * (hi - lo).max() * axis
    return rt_amd.Camera(m.astype(np.float32).reshape(-1), c[16])


def camera_inside(scene: str, kind: str = "plain") -> bool:
    """Does the camera stand inside the near box (else outside; never within 1e-3 of its faces)?"""
    inside, outside = qc.near_masks(scene, camera_origin(camera(scene, kind))[None, :])
    assert inside[0] != outside[0]
    return bool(inside[0])


def camera_origin(cam: rt_amd.Camera) -> np.ndarray:
    m = np.asarray(cam.as17()[:16], np.float64).reshape(4, 4)
    q = m @ np.array([0.0, 0.0, 0.0, 1.0])
    return q[:3] / q[3]


def kernel(scene: str, hostsim: bool, kind: str = "plain"):
    """A cached context over `scene` under its preset camera. kind: "plain"; "far" and "near" (camera()); "spheres" (Cornell with the analytic spheres of the brute manifest); "brute"
    (rt_set_intersect_mode(0)). The tests change only the gb_* schedule keys of it and reset them."""
    key = (scene, hostsim, kind)
    if key not in _kernels:
        P = parsed_scene(scene)
        mats, mi, sph = P.materials.copy(), P.material_indices, None
        if kind == "spheres":
            mats, mi, sph = rt_cases.sphere_buffers(_BRUTE["rays"]["cornell_edges_spheres"], P, mats)
        rk = rt_amd.RenderKernel(4, 4, 1, 1, rt_amd.Image(4, 4), P.triangles, mats, P.emissive_triangle_indices, mi, sph,
                                 rt_amd.BVH(P.triangles), rt_amd.Image(1, 1), None, hostsim=hostsim)
        if kind == "brute":
            rk.set_use_bvh(False)
        rk.set_camera(camera(scene, kind))
        rk.gb_mats, rk.gb_mat_idx = np.asarray(mats, np.float32).reshape(-1, 10), np.asarray(mi, np.int32)
        _kernels[key] = rk
    return _kernels[key]


def reset_schedules(hostsim: bool):
    for key, rk in _kernels.items():
        if key[1] == hostsim:
            rk.test_schedule(gb_variant=0, gb_force_every=0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what: str):
    """(albedo, normal_depth[, ids]) bit for bit."""
    for g, w, name in zip(got, want, ("albedo", "normal_depth", "ids")):
        if g.dtype == np.int32:
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")
        else:
            np.testing.assert_array_equal(bits(g), bits(w), err_msg=f"{what}: {name}")


def camera_rays(rk, w: int, h: int) -> np.ndarray:
    rays = np.empty((h * w, 6), np.float32)
    assert rk.L.rt_camera_rays(rk.ctx, w, h, rt_amd.ptr(rays)) == 0
    return rays


def records_from_query(rk, w: int, h: int):
    """(albedo, normal_depth, ids, query records) that rt_query(CLOSEST) on rt_camera_rays(w, h) implies under
    feature_pixel's rule: a hit where word 0 says so, t word 2, the normal words 6..8, the primitive word 1."""
    out = rk.query(camera_rays(rk, w, h), "closest")
    found = out[:, 0] == 1
    nd = np.zeros((h * w, 4), np.float32)
    alb = np.zeros((h * w, 4), np.float32)
    ids = np.full((h * w, 2), -1, np.int32)
    nd[:, 3] = -1.0
    nd.view(np.int32)[found, 0:3] = out[found, 6:9]
    nd.view(np.int32)[found, 3] = out[found, 2]
    ids[found, 0] = out[found, 1]
    ids[found, 1] = rk.gb_mat_idx[out[found, 1]]
    alb[found, 0:3] = rk.gb_mats[ids[found, 1], 4:7]
    return alb.reshape(h, w, 4), nd.reshape(h, w, 4), ids.reshape(h, w, 2), out


_host: dict = {}


def host_reference(scene: str, size, kind: str = "plain"):
    """The hostsim build's (albedo, normal_depth, ids) for a case, computed once."""
    key = (scene, size, kind)
    if key not in _host:
        _host[key] = kernel(scene, True, kind).gbuffer(size, ids=True)
    return _host[key]


def raw_context(hostsim: bool):
    L = rt_amd.lib(hostsim)
    h = ctypes.c_void_p()
    assert L.rt_create(0, ctypes.byref(h)) == 0
    return L, h
