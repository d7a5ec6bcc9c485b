"""Sessions: one long-lived rt_context driven through rebinds and resizes, held to a fresh oracle
after every step. Every other parity test builds a context, binds one scene, one BVH and one env,
renders at one size and destroys it; what survives between calls on a live context (device buffers
that only grow, the scene view rebuilt by each upload, the flags derived at upload, the scratch
carved per call from buffers an earlier call sized) is exercised only here.

A Session holds one context over the raw C ABI and, beside it, the bound state as plain numpy;
Session.oracle() builds an OracleScene from that state, which has no memory of the steps before.
Shared by tests/test_session.py (hostsim: the state flags of rt_capi_host.cpp, which both builds
run) and tests/test_session_gpu.py (gfx950: the device state).

Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import rt_cases
import shade_cases
import zoo_cases
from conftest import load_golden, parsed_scene

import rt_amd
from rt_amd import _capi
from rt_amd._capi import RT_ERR_ARG, RT_ERR_STATE, RT_OK

FRAME = dict(W=40, H=30, spp=2, bounces=4)
N_RAYS = 256
SEED = 8200
# the two extra schedules of the geometry zoo (tests/test_zoo_gpu.py), set once at session start
SCHEDULES = {"default": {}, "lanes1_notail": dict(lanes=1, tail_paths=0),
             "lanes3_tail": dict(lanes=3, tail_paths=1, tail_enter=1000)}

# the oracle's answers by (session, step, what): the scripts are deterministic, so the GPU file's
# three schedules of a session share one computation. Read-only once stored.
_want: dict = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bits(got, want, msg):
    """Bitwise equality of two float32 / int32 arrays of one shape, NaN matching NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{msg}: shape {got.shape} != {want.shape}"
    bad = _bits(got) != _bits(want)
    if got.dtype == np.float32 and want.dtype == np.float32:
        bad &= ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError(f"{msg}: {int(bad.sum())} of {bad.size} words differ, first at {tuple(int(v) for v in i)}: "
                             f"{got[tuple(i)]!r} != {want[tuple(i)]!r}")


def records(S, rays) -> np.ndarray:
    """The oracle's hit records as rt_intersect reports them: words 0..8 (found, primitive, t, point,
    normal) are the oracle's, u and v are -1 (include/rt_hip.h: unused downstream)."""
    out = S.intersect(rays).copy()
    out[:, 9:11] = np.float32(-1.0).view(np.int32)
    return out


class _HostArray:
    """The hostsim build's "device" buffer: a host array (its device pointers are host pointers)."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a).copy()
        self.ptr = self.a.ctypes.data

    def get(self):
        return self.a.copy()


class _DeviceArray:
    """A plain HIP allocation on the default stream, as in every device-pointer test here."""

    def __init__(self, a):
        from hip_mem import DeviceBuffer
        a = np.ascontiguousarray(a)
        self.shape, self.dtype = a.shape, a.dtype
        self.buf = DeviceBuffer(a.nbytes)
        self.buf.upload(a)
        self.ptr = self.buf.ptr

    def get(self):
        return self.buf.download(self.shape, self.dtype)


def _vp(a):
    return ctypes.c_void_p(a) if a else None


def camera_of(scene: str) -> np.ndarray:
    """camera17 of a named scene: its preset (cameras.npz), or the zoo's camera."""
    if scene in zoo_cases.SCENES:
        return zoo_cases.camera(scene)
    return load_golden("cameras.npz")["cornell" if scene.startswith("cornell") else scene]


class Session:
    """One context for its whole life; the methods mirror include/rt_hip.h and keep the bound
    state beside it. name: the session's key in SESSIONS (the oracle cache's key)."""

    def __init__(self, hostsim: bool, name: str = "", devices=None, loopback: bool = False, schedule=None):
        self.hostsim, self.name = hostsim, name
        self.L = _capi.lib(hostsim)
        h = ctypes.c_void_p()
        if devices is None:
            _capi.check(self.L, self.L.rt_create(0, ctypes.byref(h)), None, "rt_create")
        else:
            ids = np.ascontiguousarray(devices, np.int32)
            create = self.L.rt_create_multi_loopback if loopback else self.L.rt_create_multi
            _capi.check(self.L, create(ids.shape[0], _capi.ptr(ids), ctypes.byref(h)), None, "rt_create_multi")
        self.ctx = h
        self.step, self.tag = 0, "start"
        self.tris = self.mi = self.mats = self.em = self.spheres = None
        self.env = self.env_cdf = None
        self.bvh = None          # (max_depth, leaf_max) of the bound octree; None between set_scene and a build
        self.use_bvh = True
        self.cam = None
        for k, v in (schedule or {}).items():
            self.schedule(k, v)

    def close(self):
        if getattr(self, "ctx", None):
            self.L.rt_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def where(self, what: str = "") -> str:
        return f"session {self.name} step {self.step} ({self.tag}){': ' + what if what else ''}"

    def ok(self, rc, what):
        _capi.check(self.L, rc, self.ctx, self.where(what))

    def error(self) -> str:
        return (self.L.rt_last_error(self.ctx) or b"").decode()

    def array(self, a):
        return _HostArray(a) if self.hostsim else _DeviceArray(a)

    # ------------------------------------------------------------ setters
    def set_scene(self, tris, mi, mats, em, spheres=None):
        self.tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
        self.mi = np.ascontiguousarray(mi, np.int32)
        self.mats = np.ascontiguousarray(mats, np.float32).reshape(-1, 10).copy()
        self.em = np.ascontiguousarray(em, np.int32)
        self.spheres = None if spheres is None else np.ascontiguousarray(spheres, np.float32).reshape(-1, 5)
        ns = 0 if self.spheres is None else self.spheres.shape[0]
        self.ok(self.L.rt_set_scene(self.ctx, _capi.ptr(self.tris), self.tris.shape[0], _capi.ptr(self.mi),
                                    self.mi.shape[0], _capi.ptr(self.mats), self.mats.shape[0], _capi.ptr(self.em),
                                    self.em.shape[0], _capi.ptr(self.spheres), ns), "rt_set_scene")
        self.bvh = None

    def set_named_scene(self, scene: str):
        """A parsed scene or a zoo mesh, with its own camera."""
        if scene in zoo_cases.SCENES:
            mats, mi, em = zoo_cases.materials(scene)
            self.set_scene(zoo_cases.triangles(scene), mi, mats, em)
        else:
            P = parsed_scene(scene)
            self.set_scene(P.triangles, P.material_indices, P.materials, P.emissive_triangle_indices)

    def set_materials(self, mats):
        self.mats = np.ascontiguousarray(mats, np.float32).reshape(-1, 10).copy()
        self.ok(self.L.rt_set_materials(self.ctx, _capi.ptr(self.mats), self.mats.shape[0]), "rt_set_materials")

    def build_bvh(self, max_depth=32, leaf_max=8):
        self.ok(self.L.rt_build_bvh(self.ctx, max_depth, leaf_max), "rt_build_bvh")
        self.bvh = (max_depth, leaf_max)

    def set_bvh_preorder(self, dump: bytes, setting=None):
        """setting: the (max_depth, leaf_max) whose octree the dump is (None: the call is expected
        to fail and the bound tree stays). Returns the code."""
        buf = ctypes.create_string_buffer(dump, len(dump))
        rc = self.L.rt_set_bvh_preorder(self.ctx, buf, len(dump))
        if rc == RT_OK:
            assert setting is not None, self.where("rt_set_bvh_preorder accepted a dump that should fail")
            self.bvh = tuple(setting)
        return rc

    def set_env(self, img, own_cdf: bool = False):
        """img [h, w, 3 or 4]; own_cdf: pass rt_env_luminance_cdf's CDF as the caller's."""
        self.env = np.ascontiguousarray(img, np.float32)
        h, w, ch = self.env.shape
        self.env_cdf = None
        if own_cdf:
            lum, cdf = np.empty(w * h, np.float32), np.empty(w * h, np.float32)
            assert self.L.rt_env_luminance_cdf(_capi.ptr(self.env), w, h, ch, _capi.ptr(lum), _capi.ptr(cdf)) == RT_OK
            self.env_cdf = cdf
        self.ok(self.L.rt_set_env(self.ctx, _capi.ptr(self.env), w, h, ch, _capi.ptr(self.env_cdf)), "rt_set_env")

    def set_camera(self, cam17):
        self.cam = np.ascontiguousarray(cam17, np.float32).copy()
        view = np.ascontiguousarray(self.cam[:16])
        self.ok(self.L.rt_set_camera(self.ctx, _capi.ptr(view), float(self.cam[16])), "rt_set_camera")

    def set_intersect_mode(self, use_bvh: bool):
        self.ok(self.L.rt_set_intersect_mode(self.ctx, 1 if use_bvh else 0), "rt_set_intersect_mode")
        self.use_bvh = bool(use_bvh)

    def set_stats(self, on: int):
        self.ok(self.L.rt_set_stats(self.ctx, int(on)), "rt_set_stats")

    def stats(self) -> dict:
        n = len(_capi.STAT_NAMES)
        out = np.zeros(2 * n, np.uint64)
        self.ok(self.L.rt_get_stats(self.ctx, _capi.ptr(out), 2 * n), "rt_get_stats")
        return {k: int(v) for k, v in zip(_capi.STAT_NAMES, out[:n])}

    def schedule(self, key: str, value: float = 0.0):
        self.ok(self.L.rt_test_schedule(self.ctx, key.encode(), float(value)), f"rt_test_schedule {key}")

    # ------------------------------------------------------------ calls (each returns its code)
    @staticmethod
    def blank(W, H):
        fb = np.zeros((H, W, 4), np.float32)
        fb[..., 3] = 1.0
        return fb

    def render_rc(self, W, H, spp, nb, fb):
        return self.L.rt_render(self.ctx, W, H, spp, nb, _capi.ptr(fb))

    def render(self, W, H, spp, nb, fb=None) -> np.ndarray:
        fb = self.blank(W, H) if fb is None else np.ascontiguousarray(fb, np.float32).copy()
        self.ok(self.render_rc(W, H, spp, nb, fb), "rt_render")
        return fb

    def render_pixels(self, W, H, spp, nb, xy, rgba) -> np.ndarray:
        n = 0 if xy is None else xy.shape[0]
        rgba = np.ascontiguousarray(rgba, np.float32).copy()
        self.ok(self.L.rt_render_pixels(self.ctx, W, H, spp, nb, _capi.ptr(xy), n, _capi.ptr(rgba)), "rt_render_pixels")
        return rgba

    def render_device(self, W, H, spp, nb, shard, off, stride) -> np.ndarray:
        """The shard's rows on entry -> on return, through a device buffer on the default stream."""
        d = self.array(np.ascontiguousarray(shard, np.float32))
        self.ok(self.L.rt_render_device(self.ctx, W, H, spp, nb, _vp(d.ptr), off, stride, None), "rt_render_device")
        return d.get()

    def intersect_rc(self, rays, out):
        return self.L.rt_intersect(self.ctx, _capi.ptr(rays), rays.shape[0], _capi.ptr(out))

    def intersect(self, rays) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.full((rays.shape[0], 11), -7, np.int32)
        self.ok(self.intersect_rc(rays, out), "rt_intersect")
        return out

    def query_rc(self, rays, out, mode=_capi.QUERY_CLOSEST):
        return self.L.rt_query(self.ctx, mode, _capi.ptr(rays), rays.shape[0], _capi.ptr(out))

    def query(self, rays, any_hit: bool = False) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        out = np.full((n,) if any_hit else (n, 11), -7, np.int32)
        self.ok(self.query_rc(rays, out, _capi.QUERY_ANY if any_hit else _capi.QUERY_CLOSEST), "rt_query")
        return out

    def query_device(self, rays, any_hit: bool = False) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        d_rays, d_out = self.array(rays), self.array(np.full((n,) if any_hit else (n, 11), -7, np.int32))
        self.ok(self.L.rt_query_device(self.ctx, _capi.QUERY_ANY if any_hit else _capi.QUERY_CLOSEST, _vp(d_rays.ptr), n,
                                       _vp(d_out.ptr), None), "rt_query_device")
        return d_out.get()

    def query_last_exact(self) -> int:
        r = int(self.L.rt_query_last_exact(self.ctx))
        assert r >= 0, self.where(f"rt_query_last_exact {r}: {self.error()}")
        return r

    def camera_rays(self, W, H) -> np.ndarray:
        rays = np.empty((H * W, 6), np.float32)
        self.ok(self.L.rt_camera_rays(self.ctx, W, H, _capi.ptr(rays)), "rt_camera_rays")
        return rays

    def features_rc(self, W, H, alb, nd):
        return self.L.rt_render_features(self.ctx, W, H, _capi.ptr(alb), _capi.ptr(nd))

    def features(self, W, H, device: bool = False):
        """(albedo, normal_depth), [H, W, 4] each; device: through rt_render_features_device."""
        seven = np.full((H, W, 4), 7.0, np.float32)
        if device:
            d_alb, d_nd = self.array(seven), self.array(seven)
            self.ok(self.L.rt_render_features_device(self.ctx, W, H, _vp(d_alb.ptr), _vp(d_nd.ptr), None),
                    "rt_render_features_device")
            return d_alb.get(), d_nd.get()
        alb, nd = seven.copy(), seven.copy()
        self.ok(self.features_rc(W, H, alb, nd), "rt_render_features")
        return alb, nd

    def denoise(self, rgba, alb, nd, passes: int, blend: float, device: bool = False) -> np.ndarray:
        H, W = rgba.shape[:2]
        p = rt_amd.denoise_default_params(self.hostsim)
        p.passes = passes
        if device:
            d = [self.array(a) for a in (rgba, alb, nd, np.full_like(rgba, -5.0))]
            self.ok(self.L.rt_denoise_device(self.ctx, W, H, _vp(d[0].ptr), _vp(d[1].ptr), _vp(d[2].ptr), ctypes.byref(p),
                                             ctypes.c_float(blend), _vp(d[3].ptr), None), "rt_denoise_device")
            return d[3].get()
        out = np.full_like(rgba, -5.0)
        self.ok(self.L.rt_denoise(self.ctx, W, H, _capi.ptr(rgba), _capi.ptr(alb), _capi.ptr(nd), ctypes.byref(p),
                                  ctypes.c_float(blend), _capi.ptr(out)), "rt_denoise")
        return out

    def bvh_dump(self):
        """The dump, or the negative code."""
        n = self.L.rt_bvh_dump(self.ctx, None, 0)
        if n < 0:
            return n
        buf = ctypes.create_string_buffer(n)
        assert self.L.rt_bvh_dump(self.ctx, buf, n) == n
        return buf.raw

    def env_search(self, form: int, values) -> np.ndarray:
        v = np.ascontiguousarray(values, np.float32)
        out = np.full((v.shape[0], 2), -7, np.int32)
        self.ok(self.L.rt_device_env_search(self.ctx, form, _capi.ptr(v), v.shape[0], _capi.ptr(out)),
                "rt_device_env_search")
        return out

    # ------------------------------------------------------------ the oracle's side
    def oracle(self):
        """A fresh OracleScene of the bound state."""
        from oracle_bindings import OracleScene
        assert self.bvh is not None, self.where("no octree bound")
        S = OracleScene(self.tris, self.mi, self.mats, self.em, env=np.ascontiguousarray(self.env[..., :3]),
                        spheres=self.spheres, max_depth=self.bvh[0], leaf_max=self.bvh[1])
        if not self.use_bvh:
            S.set_use_bvh(False)
        return S

    def want(self, what: str, fn):
        key = (self.name, self.step, what)
        if key not in _want:
            r = fn()
            if isinstance(r, np.ndarray):
                r.setflags(write=False)
            _want[key] = r
        return _want[key]

    def box(self):
        """(lo, hi) of the triangles' vertices in float64, or None for an empty scene."""
        if self.tris.shape[0] == 0:
            return None
        v = self.tris.astype(np.float64).reshape(-1, 3)
        return v.min(0), v.max(0)

    def rays(self, n: int = N_RAYS, salt: int = 0) -> np.ndarray:
        """Seeded by the step. Half aimed at uniform points of uniformly chosen triangles from
        origins inside the scene box, half uniform directions from the box centre; an empty scene:
        all uniform directions (from the origin)."""
        rng = np.random.default_rng([SEED, self.step, n, salt])
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        b = self.box()
        o = np.zeros((n, 3))
        if b is not None:
            lo, hi = b
            o[:] = (lo + hi) / 2
            k = n // 2
            t = self.tris.astype(np.float64).reshape(-1, 3, 3)[rng.integers(0, self.tris.shape[0], k)]
            target = (rng.dirichlet((1.0, 1.0, 1.0), k)[:, :, None] * t).sum(1)
            o[:k] = rng.uniform(lo, hi, (k, 3))
            aim = target - o[:k]
            d[:k] = aim / np.maximum(np.linalg.norm(aim, axis=1, keepdims=True), 1e-300)
        return np.ascontiguousarray(np.concatenate([o, d], 1), np.float32)

    def expected_features(self, W, H):
        """(albedo, normal_depth) implied by rt_intersect on rt_camera_rays and the material
        lookup, as tests/test_features.py."""
        out = self.intersect(self.camera_rays(W, H))
        found = out[:, 0] == 1
        nd = np.zeros((H * W, 4), np.float32)
        alb = np.zeros((H * W, 4), np.float32)
        nd[:, 3] = -1.0
        nd.view(np.int32)[found, 0:3] = out[found, 6:9]
        nd.view(np.int32)[found, 3] = out[found, 2]
        alb[found, 0:3] = self.mats[self.mi[out[found, 1]], 4:7]
        return alb.reshape(H, W, 4), nd.reshape(H, W, 4)

    def check_features(self, W, H, device: bool = False):
        alb, nd = self.features(W, H, device)
        want_alb, want_nd = self.expected_features(W, H)
        assert_bits(nd, want_nd, self.where("features normal_depth vs rt_intersect of rt_camera_rays"))
        assert_bits(alb, want_alb, self.where("features albedo vs the material lookup"))
        return alb, nd

    def check_frame(self, W, H, spp, nb, what="frame") -> np.ndarray:
        cam = self.cam
        want = self.want(f"{what} {W}x{H}x{spp}x{nb}", lambda: self.oracle().render(cam, W, H, spp, nb)[0])
        got = self.render(W, H, spp, nb)
        assert_bits(got, want, self.where(f"rt_render {W}x{H} {spp} spp {nb} bounces vs the oracle"))
        return got

    def check(self, W=None, H=None, spp=None, nb=None, frame: bool = True):
        """The whole bound state against a fresh oracle, in this order: the octree dump, rt_intersect
        and rt_query (closest, any) on N_RAYS rays, the feature buffers, the frame."""
        W, H = W or FRAME["W"], H or FRAME["H"]
        spp, nb = spp or FRAME["spp"], FRAME["bounces"] if nb is None else nb
        S = None

        def oracle():
            nonlocal S
            S = S or self.oracle()
            return S

        dump = self.bvh_dump()
        assert isinstance(dump, bytes), self.where(f"rt_bvh_dump returned {dump}")
        assert dump == self.want("dump", lambda: oracle().octree_dump()), self.where("rt_bvh_dump vs the oracle's octree")
        rays = self.rays()
        want = self.want("intersect", lambda: records(oracle(), rays))
        assert_bits(self.intersect(rays), want, self.where("rt_intersect vs the oracle"))
        assert_bits(self.query(rays), want, self.where("rt_query closest vs the oracle"))
        assert_bits(self.query(rays, any_hit=True), want[:, 0], self.where("rt_query any vs the oracle's found word"))
        self.check_features(W, H)
        if frame:
            cam = self.cam
            fb = self.want("frame", lambda: oracle().render(cam, W, H, spp, nb)[0])
            got = self.render(W, H, spp, nb)
            assert_bits(got, fb, self.where(f"rt_render {W}x{H} {spp} spp {nb} bounces vs the oracle"))
            return got
        return None


# ---------------------------------------------------------------- the scripts
# A step is (tag, fn(session)); every fn ends in a check against the oracle.
def _bind(scene, setting=(32, 8), state_errors: bool = False):
    def fn(s: Session):
        if scene.startswith("tiny"):
            tris, mi, mats, em = rt_cases.tiny_scene(int(scene[4:]))
            s.set_scene(tris, mi, mats, em)
            cam = camera_of("cornell12")
        else:
            s.set_named_scene(scene)
            cam = camera_of(scene)
        if state_errors:
            assert_state_errors(s)
        s.build_bvh(*setting)
        s.set_camera(cam)
        if s.env is None:
            s.set_env(rt_cases.sky("S"))
        s.check()
    return (f"scene {scene}", fn)


def assert_state_errors(s: Session):
    """Between rt_set_scene and a build: every call that walks the tree is RT_ERR_STATE."""
    fb, rays = s.blank(4, 4), np.zeros((4, 6), np.float32)
    rays[:, 5] = 1.0
    out, a, b = np.zeros((4, 11), np.int32), np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32)
    assert s.render_rc(4, 4, 1, 1, fb) == RT_ERR_STATE, s.where("rt_render between rt_set_scene and rt_build_bvh")
    assert s.intersect_rc(rays, out) == RT_ERR_STATE, s.where("rt_intersect between rt_set_scene and rt_build_bvh")
    assert s.query_rc(rays, out) == RT_ERR_STATE, s.where("rt_query between rt_set_scene and rt_build_bvh")
    assert s.features_rc(4, 4, a, b) == RT_ERR_STATE, s.where("rt_render_features between rt_set_scene and rt_build_bvh")
    assert s.bvh_dump() == RT_ERR_STATE, s.where("rt_bvh_dump between rt_set_scene and rt_build_bvh")
    assert not out.any() and not a.any() and np.array_equal(fb, s.blank(4, 4)), s.where("an error call wrote its output")


SCENE_SWAP = [_bind(n, state_errors=True) for n in
              ("mis", "cornell12", "tiny0", "tiny1", "tiny5", "cornell", "fan", "flat", "cornell12")]


# ---- light_flags: bl_rays, any_rays, the queries' routing (cornell12)
def _lights(em: str, spheres: bool, exact):
    def fn(s: Session):
        P = parsed_scene("cornell12")
        mats, mi, sph = P.materials, P.material_indices, None
        if spheres:
            entry = dict(spheres=_sphere_entry())
            mats, mi, sph = rt_cases.sphere_buffers(entry, P, P.materials)
        s.set_scene(P.triangles, mi, mats, shade_cases.emissive(em), sph)
        s.build_bvh()
        if s.env is None:
            s.set_env(rt_cases.sky("S"))
            s.set_camera(camera_of("cornell12"))
        s.check()
        s.query(s.rays())
        n = s.query_last_exact()
        if exact == "all":
            assert n == N_RAYS, s.where(f"with spheres every query takes the exact walk: {n} of {N_RAYS}")
        elif exact == "some":
            assert n < N_RAYS, s.where(f"without spheres the search-BVH walk answers: {n} of {N_RAYS} exact")
    return (f"emissive {em}{' + spheres' if spheres else ''}", fn)


def _sphere_entry():
    import json
    import os

    import golden_io as gio
    with open(os.path.join(gio.GOLDEN, "manifest.json")) as f:
        return json.load(f)["renders"]["spheres_cornell32_128"]["spheres"]


LIGHT_FLAGS = [_lights("default", False, None), _lights("empty", False, None), _lights("repeat", False, None),
               _lights("default", True, "all"), _lights("default", False, "some"), _lights("empty", True, "all")]


# ---- bvh_rebind (zoo soup)
def _soup_first(s: Session):
    s.set_named_scene("soup")
    s.build_bvh(32, 8)
    s.set_camera(camera_of("soup"))
    s.set_env(rt_cases.sky("S"))
    s.check()


def _rebuild(setting):
    def fn(s: Session):
        s.build_bvh(*setting)
        s.check()
    return (f"rt_build_bvh{setting}", fn)


def _preorder(s: Session):
    from oracle_bindings import OracleScene
    dump = OracleScene(s.tris, s.mi, s.mats, s.em, max_depth=32, leaf_max=8).octree_dump()
    assert s.set_bvh_preorder(dump, (32, 8)) == RT_OK, s.where(f"rt_set_bvh_preorder: {s.error()}")
    s.check()


def _malformed(s: Session):
    dump = s.bvh_dump()
    assert s.set_bvh_preorder(dump[:-7]) == RT_ERR_ARG, s.where("a dump cut by 7 bytes must be RT_ERR_ARG")
    assert "malformed" in s.error(), s.where(s.error())
    s.check()  # (still the previous tree)


def _mode(use_bvh):
    def fn(s: Session):
        s.set_intersect_mode(use_bvh)
        s.check()
    return (f"rt_set_intersect_mode({int(use_bvh)})", fn)


def _sched(key, value):
    def fn(s: Session):
        s.schedule(key, value)
        s.check()
    return (f"rt_test_schedule({key}, {value})", fn)


# (the brute-force loop is the one reader of the view's triangle count: 12 triangles in buffers that held 3000)
SCENE_SWAP += [_mode(False), _mode(True)]

BVH_REBIND = ([("soup (32, 8)", _soup_first)] + [_rebuild(v) for v in ((3, 2), (12, 1), (1, 8))] +
              [("rt_set_bvh_preorder of the oracle's (32, 8)", _preorder), _mode(False), _mode(True),
               _sched("chain_full", 1), _sched("chain_full", 0), ("malformed dump", _malformed)])


# ---- env_rebind (cornell12): every transition between the LDS-staged, global-fence and binary
# search forms, a smaller table after a larger one. The binary envs of that order are narrower than
# 32 texels, so none reads the coarse column table (cdf_coarse, cdf_cw = w / 32, which only the binary
# form uses); the last step is a binary env that does, after envs of 1 and 16 coarse columns.
ENV_ORDER = ["grad_20x9", "grad_1x1", "grad_16x1024", "grad_16x1025", "grad_48x7", "rgba_48x7", "grad_16x4097",
             "grad_16x1", "S", "S+cdf", "grad_127x5"]


def _env(name):
    def fn(s: Session):
        if s.tris is None:
            s.set_named_scene("cornell12")
            s.build_bvh()
            s.set_camera(camera_of("cornell12"))
        img = shade_cases.env(name.split("+")[0])
        s.set_env(img, own_cdf=name.endswith("+cdf"))
        values = shade_cases.search_values(img)
        want = s.want("env search", lambda: shade_cases.ref_search(img, values))
        for form in (0, 1):
            got = s.env_search(form, values)
            assert np.array_equal(got, want), s.where(
                f"rt_device_env_search form {form} on {name}: {int((got != want).any(1).sum())} of {want.shape[0]} differ")
        s.check()
    return (f"env {name}", fn)


ENV_REBIND = [_env(n) for n in ENV_ORDER]


# ---- sizes_and_entries (mis, one camera)
BIG = dict(W=64, H=48)


def _mis_first(s: Session):
    s.set_named_scene("mis")
    s.build_bvh()
    s.set_camera(camera_of("mis"))
    s.set_env(rt_cases.sky("S"))
    s.check(**BIG)


def _size(W, H, spp=None, nb=None):
    def fn(s: Session):
        s.check(W, H, spp, nb)
    return (f"render {W}x{H}" + (f" {spp} spp {nb} bounces" if spp else ""), fn)


def _random_fb(s: Session, W, H):
    rng = np.random.default_rng([SEED, 55, s.step])
    fb = np.empty((H, W, 4), np.float32)
    fb[..., :3] = rng.uniform(0.0, 2.0, (H, W, 3))
    fb[..., 3] = rng.uniform(0.0, 1.0, (H, W))
    return fb


def _pixels(n):
    def fn(s: Session):
        W, H, spp, nb = BIG["W"], BIG["H"], FRAME["spp"], FRAME["bounces"]
        fb = _random_fb(s, W, H)
        rng = np.random.default_rng([SEED, 56, s.step])
        flat = rng.permutation(W * H)[:n]  # (distinct pixels)
        xy = np.ascontiguousarray(np.stack([flat % W, flat // W], 1), np.int32)
        if n == 0:
            rgba = np.full((3, 4), 9.0, np.float32)
            assert_bits(s.render_pixels(W, H, spp, nb, None, rgba), rgba, s.where("rt_render_pixels n = 0 wrote"))
        else:
            cam = s.cam
            want = s.want("pixels", lambda: np.ascontiguousarray(s.oracle().render(cam, W, H, spp, nb, pixels=xy,
                                                                                  fb=fb.copy())[0]))
            got = s.render_pixels(W, H, spp, nb, xy, fb[xy[:, 1], xy[:, 0]])
            assert_bits(got, want, s.where(f"rt_render_pixels of {n} pixels vs the oracle"))
        s.check(frame=False, **BIG)
    return (f"rt_render_pixels n = {n}", fn)


def _shard(off, stride):
    def fn(s: Session):
        W, H, spp, nb = BIG["W"], BIG["H"], FRAME["spp"], FRAME["bounces"]
        fb = _random_fb(s, W, H)
        cam = s.cam
        want = s.want("shard", lambda: s.oracle().render(cam, W, H, spp, nb, fb=fb.copy())[0])
        got = s.render_device(W, H, spp, nb, fb[off::stride], off, stride)
        assert_bits(got, want[off::stride], s.where(f"rt_render_device shard ({off}, {stride}) vs the oracle"))
        s.check(frame=False, **BIG)
    return (f"rt_render_device shard ({off}, {stride})", fn)


def _stats(s: Session):
    s.set_stats(1)
    with_stats = s.check(**BIG)
    st = s.stats()
    assert st["rays"] > 0 and st["steps"] >= 0, s.where(f"rt_get_stats after a stats render: {st}")
    s.set_stats(0)
    plain = s.check_frame(BIG["W"], BIG["H"], FRAME["spp"], FRAME["bounces"], what="plain frame")
    assert_bits(plain, with_stats, s.where("the stats render's frame vs the plain one's"))


def _lanes(s: Session):
    for lanes in (3, 4, 1):
        s.schedule("lanes", lanes)
        s.check(**BIG)
    s.schedule("reset")
    s.check(**BIG)


SIZES_AND_ENTRIES = [("mis 64x48", _mis_first), _size(7, 5), _size(1, 1), _size(200, 3), _pixels(5), _pixels(1), _pixels(0),
                     _shard(1, 3), _shard(0, 1), _size(64, 48, 1, 0), _size(64, 48, 5, 9), ("stats on, off", _stats),
                     ("lanes 3, 4, 1, reset", _lanes)]


# ---- stages_interleaved (cornell)
_fresh_host: dict = {}


def hostsim_denoise(rgba, alb, nd, passes, blend) -> np.ndarray:
    """rt_denoise of the hostsim build on a bare context of its own (it needs no scene)."""
    if "s" not in _fresh_host:
        _fresh_host["s"] = Session(True, "denoise reference")
    return _fresh_host["s"].denoise(rgba, alb, nd, passes, blend)


def _cornell_first(s: Session):
    s.set_named_scene("cornell")
    s.build_bvh()
    s.set_camera(camera_of("cornell"))
    s.set_env(rt_cases.sky("S"))
    s.check()


def _query(n, device=False):
    def fn(s: Session):
        rays = s.rays(n, salt=1)
        want = s.want("query", lambda: records(s.oracle(), rays))
        run = s.query_device if device else s.query
        assert_bits(run(rays), want, s.where(f"rt_query{'_device' if device else ''} closest n = {n} vs the oracle"))
        assert_bits(run(rays, any_hit=True), want[:, 0], s.where(f"rt_query{'_device' if device else ''} any n = {n}"))
        s.check()
    return (f"rt_query{'_device' if device else ''} n = {n}", fn)


def _post(W, H, device=False):
    def fn(s: Session):
        frame = s.check_frame(W, H, FRAME["spp"], FRAME["bounces"])
        alb, nd = s.check_features(W, H, device)
        got = s.denoise(frame, alb, nd, 3, 0.75, device)
        assert_bits(got, hostsim_denoise(frame, alb, nd, 3, 0.75), s.where(f"rt_denoise {W}x{H} vs hostsim"))
        s.check()
    return (f"render, features{'_device' if device else ''} + denoise {W}x{H}", fn)


def _mats_and_env(s: Session):
    m = s.mats.copy()
    m[2, 9] = np.float32(0.25)  # one roughness
    s.set_materials(m)
    s.set_env(rt_cases.sky("L"))  # (with the full dirty: one upload carries both)
    s.check()


def _mats_alone(s: Session):
    before, _ = s.features(FRAME["W"], FRAME["H"])
    m = s.mats.copy()
    m[1:, 4:7] = m[1:, 4:7] * np.float32(0.5) + np.float32(0.125)  # every diffuse colour
    s.set_materials(m)
    alb, _ = s.check_features(FRAME["W"], FRAME["H"])
    assert (alb != before).any(), s.where("the albedo must show the new diffuse")
    s.check()


STAGES_INTERLEAVED = [("cornell 40x30", _cornell_first), _query(100), _post(40, 30), _query(5000), _post(16, 12),
                      _query(10, device=True), _post(40, 30, device=True), ("rt_set_materials + rt_set_env (sky L)", _mats_and_env),
                      ("rt_set_materials alone, features, render", _mats_alone)]


# ---- camera_across_near_box (cornell12)
NEAR = 0.5     # RT_NEAR_SCALE: the near box is the scene box widened by this x its largest extent
SHELL = 0.3    # the fourth camera: this x the largest extent outside the scene box


def _outside(p, lo, hi):
    """Largest per-axis distance of p outside [lo, hi] (0 inside)."""
    return float(np.maximum(np.maximum(lo - p, p - hi), 0.0).max())


def _moved_back(cam17, dist=None, until=None, lo=None, hi=None):
    """The view translated along its viewing axis: back by dist, or to the point behind the box
    where the origin lies `until` outside it (the distance outside is convex along the axis: the
    point of least distance by a scan, then a bisection behind it)."""
    c = np.asarray(cam17, np.float64).copy()
    m = c[:16].reshape(4, 4)
    back = -m[:3, 2] / np.linalg.norm(m[:3, 2])
    o = m[:3, 3].copy()
    if dist is None:
        reach = 16.0 * float((hi - lo).max()) + float(np.abs(o).max())
        grid = np.linspace(-reach, reach, 4097)
        a = float(grid[int(np.argmin([_outside(o + g * back, lo, hi) for g in grid]))])
        b = reach
        assert _outside(o + a * back, lo, hi) < until < _outside(o + b * back, lo, hi)
        for _ in range(100):
            mid = (a + b) / 2
            a, b = (mid, b) if _outside(o + mid * back, lo, hi) < until else (a, mid)
        dist = b
    m[:3, 3] = o + dist * back
    return np.concatenate([m.ravel(), c[16:]]).astype(np.float32)


def _camera(which):
    def fn(s: Session):
        if s.tris is None:
            s.set_named_scene("cornell12")
            s.build_bvh()
            s.set_env(rt_cases.sky("S"))
        lo, hi = s.box()
        ext = float((hi - lo).max())
        preset = camera_of("cornell12")
        if which == "preset":
            s.set_camera(preset)
        elif which == "far":
            cam = _moved_back(preset, dist=3.0 * ext)
            assert _outside(cam[:16].reshape(4, 4)[:3, 3].astype(np.float64), lo, hi) > NEAR * ext * 1.01
            s.set_camera(cam)
            # far_check is on: every camera ray takes the exact walk
            rays = s.camera_rays(FRAME["W"], FRAME["H"])
            want = s.want("camera rays", lambda: records(s.oracle(), rays))
            assert_bits(s.query(rays), want, s.where("rt_query of the far camera's rays vs the oracle"))
            n = s.query_last_exact()
            assert n == rays.shape[0], s.where(f"queries from outside the near box: {n} of {rays.shape[0]} exact")
        else:
            cam = _moved_back(preset, until=SHELL * ext, lo=lo, hi=hi)
            d = _outside(cam[:16].reshape(4, 4)[:3, 3].astype(np.float64), lo, hi)
            assert 0.9 * SHELL * ext < d < NEAR * ext, s.where(f"camera {d / ext:.3f} x extent outside the box")
            s.set_camera(cam)
        s.check()
    return (f"camera {which}", fn)


CAMERA_ACROSS_NEAR_BOX = [_camera("preset"), _camera("far"), _camera("preset"), _camera("shell")]


# ---- multi_loopback: three "devices" (gfx950: rt_create_multi_loopback over one GPU)
MULTI = dict(W=48, H=36)


def _multi_scene(scene, **size):
    def fn(s: Session):
        s.set_named_scene(scene)
        s.build_bvh()
        s.set_camera(camera_of(scene))
        if s.env is None:
            s.set_env(rt_cases.sky("S"))
        s.check(**size)
    return (f"{scene} {size['W']}x{size['H']}", fn)


def _multi_pixels(s: Session):
    W, H, spp, nb = MULTI["W"], MULTI["H"], FRAME["spp"], FRAME["bounces"]
    fb = _random_fb(s, W, H)
    flat = np.random.default_rng([SEED, 57]).permutation(W * H)[:7]
    xy = np.ascontiguousarray(np.stack([flat % W, flat // W], 1), np.int32)
    cam = s.cam
    want = s.want("pixels", lambda: np.ascontiguousarray(s.oracle().render(cam, W, H, spp, nb, pixels=xy, fb=fb.copy())[0]))
    assert_bits(s.render_pixels(W, H, spp, nb, xy, fb[xy[:, 1], xy[:, 0]]), want, s.where("rt_render_pixels of 7 pixels"))
    s.check(frame=False, **MULTI)


def _multi_fail(s: Session):
    s.ok(s.L.rt_test_fail_device(s.ctx, 1), "rt_test_fail_device")
    fb = s.blank(MULTI["W"], MULTI["H"])
    rc = s.render_rc(MULTI["W"], MULTI["H"], FRAME["spp"], FRAME["bounces"], fb)
    assert rc == RT_ERR_STATE and "device 1: injected failure" in s.error(), s.where(f"{rc}: {s.error()}")
    s.ok(s.L.rt_test_fail_device(s.ctx, -1), "rt_test_fail_device")
    s.check(**MULTI)


def _multi_rebind(s: Session):
    s.set_env(shade_cases.env("grad_48x7"))
    s.set_named_scene("mis")
    s.build_bvh()
    s.set_camera(camera_of("mis"))
    s.check(**MULTI)


MULTI_LOOPBACK = [_multi_scene("mis", **MULTI), _multi_scene("cornell12", **MULTI),
                  ("10x2: device 2 has no rows", lambda s: s.check(10, 2)), ("1x1", lambda s: s.check(1, 1)),
                  ("rt_render_pixels of 7 pixels", _multi_pixels), ("device 1 fails, then recovers", _multi_fail),
                  ("rt_set_env, rt_set_scene(mis), 48x36", _multi_rebind)]

SESSIONS = {"scene_swap": SCENE_SWAP, "light_flags": LIGHT_FLAGS, "bvh_rebind": BVH_REBIND, "env_rebind": ENV_REBIND,
            "sizes_and_entries": SIZES_AND_ENTRIES, "stages_interleaved": STAGES_INTERLEAVED,
            "camera_across_near_box": CAMERA_ACROSS_NEAR_BOX, "multi_loopback": MULTI_LOOPBACK}


def run(name: str, hostsim: bool, schedule: str = "default"):
    """The session's script on one context, start to end."""
    kw = {}
    if name == "multi_loopback":
        kw = dict(devices=[0, 1, 2]) if hostsim else dict(devices=[0, 0, 0], loopback=True)
    s = Session(hostsim, name, schedule=SCHEDULES[schedule], **kw)
    try:
        for i, (tag, fn) in enumerate(SESSIONS[name]):
            s.step, s.tag = i, tag
            fn(s)
    finally:
        s.close()


def run_state_errors(hostsim: bool):
    """The implicit 1x1 env of rt_intersect, rt_query and rt_render_features (a placeholder that
    keeps the device view valid) is not the caller's env: rt_render still asks for one."""
    s = Session(hostsim, "state_errors")
    try:
        s.tag = "no env"
        s.set_named_scene("cornell12")
        s.build_bvh()
        rays = s.rays()
        s.intersect(rays)
        s.query(rays)
        s.set_camera(camera_of("cornell12"))
        s.features(8, 6)
        fb = s.blank(8, 6)
        rc = s.render_rc(8, 6, 1, 1, fb)
        assert rc == RT_ERR_STATE and "environment map not set" in s.error(), s.where(f"rt_render: {rc} {s.error()!r}")
        assert np.array_equal(fb, s.blank(8, 6)), s.where("the refused render wrote its framebuffer")
        xy, rgba = np.zeros((1, 2), np.int32), np.zeros((1, 4), np.float32)
        assert s.L.rt_render_pixels(s.ctx, 8, 6, 1, 1, _capi.ptr(xy), 1, _capi.ptr(rgba)) == RT_ERR_STATE
        s.step, s.tag = 1, "a real env"
        s.set_env(rt_cases.sky("S"))
        s.check()
    finally:
        s.close()
