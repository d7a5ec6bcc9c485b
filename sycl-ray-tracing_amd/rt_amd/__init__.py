"""rt_amd — Python mirror of the reference host API over librt_hip.so.

Names, argument meaning and mutation semantics follow the reference
(TomClabault/SYCL-ray-tracing @ 2024-08-07) so tests read like its own:

  Camera / presets     include/camera.h:10-40, source/camera.cpp:3-8
  Image                include/image.h:25-178  (RGBA float32, black = (0,0,0,1))
  parse_obj            source/utils.cpp:16-98  -> ParsedOBJ (include/parsed_obj.h)
  compute_env_map_cdf  source/utils.cpp:126-142
  read_image_float     source/utils.cpp:100-124  (Radiance .hdr, stb_image 2.28 decode, flipY)
  write_image_png      source/image_io.cpp:165-182
  BVH                  include/bvh.h:211-280, source/bvh.cpp:19-37
  RenderKernel         include/render_kernel.h:21-96
     render()            mutates the image buffer in place (render_kernel.cpp:189-211)
     ray_trace_pixel()   one pixel (render_kernel.cpp:75-181)

All compute runs in the native library (C++ host preparation + gfx950 HIP
kernels); this module only moves numpy buffers across the C ABI.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _capi
from ._capi import (METER_STATS, METER_WORDS, BloomParams, DenoiseParams, DenoiseVarParams, DisplayParams, DofParams,  # noqa: F401
                    FireflyParams, MotionParams,
                    MeterParams, MeterResult, NoiseStats, TemporalParams, UpscaleParams)
from ._capi import (RT_ERR_ARG, RT_ERR_HIP, RT_ERR_IO, RT_ERR_NODEV, RT_ERR_STATE, RT_OK,  # noqa: F401
                    RtError, check, lib, ptr)

__all__ = ["Camera", "Image", "ParsedOBJ", "parse_obj", "compute_env_map_cdf", "luminance_of_pixels", "BVH",
           "RenderKernel", "RtError", "octree_dump", "make_materials", "read_image_float", "write_image_png",
           "image_to_rgba8", "DenoiseParams", "denoise_default_params", "DisplayParams", "write_image_hdr", "DenoiseVarParams",
           "denoise_var_default_params", "TemporalParams", "temporal_default_params", "TemporalHistory",
           "FireflyParams", "firefly_default_params", "MeterParams", "meter_default_params", "meter_stats", "meter_solve",
           "ExposureAdapter", "METER_WORDS", "METER_STATS", "UpscaleParams", "upscale_default_params",
           "BloomParams", "bloom_default_params", "DofParams", "dof_default_params", "focus_at",
           "MotionParams", "motion_default_params"]


# ------------------------------------------------------------------ camera
class Camera:
    """view_matrix: 4x4 float32 row-major (Transform::m); fov_dist (camera.h:38-40)."""

    PRESETS = ("default", "cornell", "ganesha", "ite", "dragon", "mis")

    def __init__(self, view_matrix=None, fov_dist=None):
        if view_matrix is None:
            c = Camera.preset("default")
            view_matrix, fov_dist = c.view_matrix, c.fov_dist
        self.view_matrix = np.ascontiguousarray(view_matrix, dtype=np.float32).reshape(4, 4)
        self.fov_dist = float(np.float32(fov_dist))

    @staticmethod
    def preset(name: str) -> "Camera":
        v = np.zeros(16, dtype=np.float32)
        f = ctypes.c_float()
        check(lib(), lib().rt_camera_preset(name.encode(), ptr(v), ctypes.byref(f)), None, f"camera preset {name}")
        return Camera(v, f.value)

    def as17(self) -> np.ndarray:
        return np.concatenate([self.view_matrix.ravel(), [np.float32(self.fov_dist)]]).astype(np.float32)


# ------------------------------------------------------------------- image
class Image:
    """Image(w, h[, color]) — pixels is a [h, w, 4] float32 array (RGBA)."""

    def __init__(self, width: int, height: int, color=(0.0, 0.0, 0.0, 1.0), pixels=None):
        if pixels is not None:
            self.pixels = np.ascontiguousarray(pixels, dtype=np.float32).reshape(height, width, 4)
        else:
            self.pixels = np.empty((height, width, 4), dtype=np.float32)
            self.pixels[...] = np.asarray(color, dtype=np.float32)
        self.width, self.height = width, height

    @staticmethod
    def from_rgb(rgb: np.ndarray, alpha: float = 0.0) -> "Image":
        """Like Utils::read_image_float (utils.cpp:100-124): alpha forced to 0."""
        h, w = rgb.shape[:2]
        px = np.empty((h, w, 4), dtype=np.float32)
        px[..., :3] = rgb[..., :3]
        px[..., 3] = alpha
        return Image(w, h, pixels=px)

    def data(self) -> np.ndarray:
        return self.pixels


def luminance_of_pixels(img: Image) -> np.ndarray:
    lum = np.empty(img.width * img.height, dtype=np.float32)
    cdf = np.empty_like(lum)
    check(lib(), lib().rt_env_luminance_cdf(ptr(img.pixels), img.width, img.height, 4, ptr(lum), ptr(cdf)))
    return lum


def compute_env_map_cdf(img: Image) -> np.ndarray:
    lum = np.empty(img.width * img.height, dtype=np.float32)
    cdf = np.empty_like(lum)
    check(lib(), lib().rt_env_luminance_cdf(ptr(img.pixels), img.width, img.height, 4, ptr(lum), ptr(cdf)))
    return cdf


def read_image_float(filepath: str, flipY: bool = True) -> Image:
    """Utils::read_image_float (utils.cpp:100-124) for Radiance .hdr files:
    RGB decoded like stb_image 2.28, alpha 0, rows flipped when flipY."""
    L_ = lib()
    w, h = ctypes.c_int(), ctypes.c_int()
    check(L_, L_.rt_read_hdr(filepath.encode(), int(flipY), ctypes.byref(w), ctypes.byref(h), None), None,
          f"read_image_float({filepath})")
    img = Image(w.value, h.value)
    check(L_, L_.rt_read_hdr(filepath.encode(), int(flipY), ctypes.byref(w), ctypes.byref(h), ptr(img.pixels)), None,
          f"read_image_float({filepath})")
    return img


def image_to_rgba8(img: Image) -> np.ndarray:
    """write_image_png's 8-bit conversion (image_io.cpp:170-177), no flip: [h, w, 4] uint8."""
    out = np.empty((img.height, img.width, 4), dtype=np.uint8)
    check(lib(), lib().rt_image_to_rgba8(ptr(img.pixels), img.width * img.height, ptr(out)), None, "image_to_rgba8")
    return out


def write_image_png(image: Image, filename: str, flipY: bool = True) -> bool:
    """write_image_png (image_io.cpp:165-182): False for an empty image."""
    if image.width * image.height == 0:
        return False
    check(lib(), lib().rt_write_png(filename.encode(), ptr(image.pixels), image.width, image.height, int(flipY)), None,
          f"write_image_png({filename})")
    return True


def write_image_hdr(image: Image, filename: str, flipY: bool = True) -> bool:
    """write_image_hdr (image_io.cpp:208-214): the rgb channels as a Radiance RGBE file that
    read_image_float decodes (rt_write_hdr); False for an empty image."""
    if image.width * image.height == 0:
        return False
    px = np.ascontiguousarray(image.pixels, dtype=np.float32)
    check(lib(), lib().rt_write_hdr(filename.encode(), ptr(px), image.width, image.height, int(flipY)), None,
          f"write_image_hdr({filename})")
    return True


def _vp(a):
    """A device address (an int, or None / 0 for "not given") as the void* argument of a *_device call."""
    return ctypes.c_void_p(a) if a else None


def _params(L_, cls, stage: str, params):
    """A stage's parameter struct. params: None (rt_<stage>_default_params), a cls, or a dict of its fields
    over the defaults."""
    if isinstance(params, cls):
        return params
    p = cls()
    getattr(L_, f"rt_{stage}_default_params")(ctypes.byref(p))
    for k, v in (params or {}).items():
        if k not in dict(cls._fields_):
            raise TypeError(f"unknown {stage} parameter {k}")
        setattr(p, k, v)
    return p


def denoise_default_params(hostsim: bool = False) -> DenoiseParams:
    """rt_denoise_default_params: the à-trous filter's defaults (passes and the four sigmas)."""
    return _params(lib(hostsim), DenoiseParams, "denoise", None)


def denoise_var_default_params(hostsim: bool = False) -> DenoiseVarParams:
    """rt_denoise_var_default_params: the variance-guided filter's defaults."""
    return _params(lib(hostsim), DenoiseVarParams, "denoise_var", None)


def temporal_default_params(hostsim: bool = False) -> TemporalParams:
    """rt_temporal_default_params: temporal accumulation's defaults."""
    return _params(lib(hostsim), TemporalParams, "temporal", None)


def firefly_default_params(hostsim: bool = False) -> FireflyParams:
    """rt_firefly_default_params: the firefly rejection stage's defaults."""
    return _params(lib(hostsim), FireflyParams, "firefly", None)


def upscale_default_params(hostsim: bool = False) -> UpscaleParams:
    """rt_upscale_default_params: the guided upscale stage's defaults."""
    return _params(lib(hostsim), UpscaleParams, "upscale", None)


def bloom_default_params(hostsim: bool = False) -> BloomParams:
    """rt_bloom_default_params: the bloom stage's defaults."""
    return _params(lib(hostsim), BloomParams, "bloom", None)


def dof_default_params(hostsim: bool = False) -> DofParams:
    """rt_dof_default_params: the depth-of-field stage's defaults."""
    return _params(lib(hostsim), DofParams, "dof", None)


def focus_at(normal_depth, x: int, y: int) -> float:
    """The focus distance for RenderKernel.dof that puts pixel (x, y) in focus: the t of normal_depth [h, w, 4]
    (features() or gbuffer()) under it. A miss there (t not finite or not > 0): the nearest hit, the smallest t, of
    the smallest square window about the pixel that holds one. ValueError for a frame without a hit."""
    t = np.asarray(normal_depth)[..., 3]
    h, w = t.shape
    if not (0 <= x < w and 0 <= y < h):
        raise ValueError(f"focus_at: pixel ({x}, {y}) is outside the {w} x {h} frame")
    with np.errstate(all="ignore"):
        hit = np.isfinite(t) & (t > 0)
    for n in range(max(w, h)):
        ys, xs = slice(max(y - n, 0), y + n + 1), slice(max(x - n, 0), x + n + 1)
        if hit[ys, xs].any():
            return float(t[ys, xs][hit[ys, xs]].min())
    raise ValueError("focus_at: the frame has no hit")


def motion_default_params(hostsim: bool = False) -> MotionParams:
    """rt_motion_default_params: the motion-blur stage's defaults."""
    return _params(lib(hostsim), MotionParams, "motion", None)


def meter_default_params(hostsim: bool = False) -> MeterParams:
    """rt_meter_default_params: the defaults of rt_meter_solve."""
    return _params(lib(hostsim), MeterParams, "meter", None)


def meter_stats(hist) -> dict:
    """The words of an rt_meter_hist by name: "bins" (a view of the 256 counts) and the stat words as ints."""
    h = np.asarray(hist, dtype=np.uint32).reshape(METER_WORDS)
    return {"bins": h[:256], **{k: int(h[256 + i]) for i, k in enumerate(METER_STATS)}}


def meter_solve(hist, prev: float = 0.0, dt: float = 0.0, hostsim: bool = False, **params) -> dict:
    """rt_meter_solve: a histogram of RenderKernel.meter (264 uint32 words) to the exposure display() takes.
    prev: the last frame's exposure (<= 0: none) and dt the seconds since, for the adaptation with tau_up /
    tau_down; params: fields of MeterParams over the defaults, or params=MeterParams. Host code only (no
    context); hostsim picks the library that is asked. Returns {"exposure", "target", "log2_mean", "valid"}."""
    return _meter_solve(lib(hostsim), hist, prev, dt, params)


def _meter_solve(L_, hist, prev, dt, params) -> dict:
    p = _params(L_, MeterParams, "meter", params.pop("params") if "params" in params else params)
    h = np.ascontiguousarray(hist, dtype=np.uint32).reshape(METER_WORDS)
    r = MeterResult()
    check(L_, L_.rt_meter_solve(ptr(h), ctypes.byref(p), float(prev), float(dt), ctypes.byref(r)), None, "rt_meter_solve")
    return {"exposure": float(r.exposure), "target": float(r.target), "log2_mean": float(r.log2_mean), "valid": bool(r.valid)}


class ExposureAdapter:
    """The exposure carried from frame to frame, TemporalHistory's sibling for the display stage:
    update(linear, dt) meters the frame (RenderKernel.meter), solves with the exposure of the last update as
    prev and dt seconds since, keeps the result and returns it. The first update, or one after reset(), jumps
    to the target. tau_up / tau_down: the time constants in seconds while the exposure rises and falls (0: at
    once); kernel: the RenderKernel whose context meters (or pass one to update); params: further fields of
    MeterParams."""

    def __init__(self, tau_up: float = 0.0, tau_down: float = 0.0, kernel: "RenderKernel | None" = None, **params):
        self.params = dict(params, tau_up=tau_up, tau_down=tau_down)
        self.kernel = kernel
        self.exposure = 0.0
        self.last = None  # (the last update's whole result)

    def reset(self):
        self.exposure, self.last = 0.0, None

    def update(self, linear, dt: float, kernel: "RenderKernel | None" = None) -> float:
        kernel = kernel or self.kernel
        if kernel is None:
            raise ValueError("ExposureAdapter.update: no RenderKernel given here or to the constructor")
        self.last = kernel.auto_exposure(linear, prev=self.exposure, dt=dt, full=True, **self.params)
        self.exposure = self.last["exposure"]
        return self.exposure


class TemporalHistory:
    """The state temporal accumulation carries from frame to frame: the accumulated colour, its standard
    deviation, the history length, the previous frame's normal_depth and the previous camera.

    push(kernel, linear, sigma, firefly=None) renders the features under the kernel's current camera, calls
    RenderKernel.temporal_accumulate against what the last push kept (nothing on the first) and keeps the
    result; it returns (rgba Image, sigma, length), which rt_denoise_var takes as its image and sigma.
    firefly: a FireflyParams or a dict of its fields ({}: the defaults) puts RenderKernel.firefly_clamp in front,
    so that a spike is limited before the history keeps it; None: the frame is accumulated as it is.

    Seeding across frames. A render seeds pixel (x, y) with 31 + x * y * N, N the declared sample total, so
    two frames with the same total draw the same random numbers and their noise is correlated: accumulating
    them averages nothing. Declare a different total per frame and stop early instead. Frame k:
        kernel.set_camera(camera_k)
        kernel.progress_begin(N0 + k); kernel.progress_track_noise()
        kernel.progress_advance(s // 2); kernel.progress_advance(s // 2)
        linear = kernel.progress_resolve_linear(Image(w, h)); sigma = kernel.progress_noise_sigma()
        rgba, sigma_acc, length = history.push(kernel, linear, sigma)
    and never finish the progression: a preview of the first s samples of the (N0 + k)-sample chain is a
    supported state. Pixels with x * y == 0 (the first row and column) keep seed 31 in every frame."""

    def __init__(self, params=None):
        self.params = params
        self.rgba = self.sigma = self.length = self.normal_depth = self.camera = None

    def reset(self):
        self.rgba = self.sigma = self.length = self.normal_depth = self.camera = None

    def push(self, kernel: "RenderKernel", linear: Image, sigma, firefly=None):
        if firefly is not None:
            linear, sigma = kernel.firefly_clamp(linear, sigma, firefly)
        _, nd = kernel.guides()
        hist = None if self.rgba is None else (self.rgba, self.sigma, self.length, self.normal_depth)
        cam = kernel.camera if self.camera is None else self.camera
        out, s_out, l_out = kernel.temporal_accumulate(linear, sigma, nd, cam, hist, self.params)
        self.rgba, self.sigma, self.length, self.normal_depth = out, s_out, l_out, nd
        self.camera = Camera(kernel.camera.view_matrix.copy(), kernel.camera.fov_dist)
        return out, s_out, l_out

    def motion_vectors(self, kernel: "RenderKernel", normal_depth):
        """RenderKernel.motion_vectors of normal_depth (guides under the kernel's current camera) against the camera of
        the last push; before the first push the kernel's own camera, which gives zeroes but for rounding."""
        return kernel.motion_vectors(normal_depth, kernel.camera if self.camera is None else self.camera)


# --------------------------------------------------------------------- OBJ
@dataclass
class ParsedOBJ:
    triangles: np.ndarray                  # [N, 9] float32
    materials: np.ndarray                  # [M, 10] float32
    emissive_triangle_indices: np.ndarray  # [E] int32
    material_indices: np.ndarray           # [N] int32
    spheres: np.ndarray = field(default_factory=lambda: np.zeros((0, 5), np.float32))


def parse_obj(path: str) -> ParsedOBJ:
    L_ = lib()
    m = ctypes.c_void_p()
    check(L_, L_.rt_mesh_load(path.encode(), ctypes.byref(m)), None, f"parse_obj({path})")
    try:
        nt, nm, ne = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L_.rt_mesh_counts(m, ctypes.byref(nt), ctypes.byref(nm), ctypes.byref(ne))
        tris = np.empty((nt.value, 9), np.float32)
        mi = np.empty(nt.value, np.int32)
        mats = np.empty((nm.value, 10), np.float32)
        em = np.empty(ne.value, np.int32)
        L_.rt_mesh_copy(m, ptr(tris), ptr(mi), ptr(mats), ptr(em))
    finally:
        L_.rt_mesh_free(m)
    return ParsedOBJ(tris, mats, em, mi)


def make_materials(rows) -> np.ndarray:
    """rows of (emission rgb, diffuse rgb, metalness, roughness) -> [M,10] SimpleMaterial buffer."""
    out = []
    for e, d, metal, rough in rows:
        out.append([*e, 1.0, *d, 1.0, metal, rough])
    return np.asarray(out, dtype=np.float32)


def octree_dump(triangles: np.ndarray, max_depth: int = 32, leaf_max: int = 8) -> bytes:
    tris = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    L_ = lib()
    n = L_.rt_octree_dump(ptr(tris), tris.shape[0], max_depth, leaf_max, None, 0)
    buf = ctypes.create_string_buffer(n)
    L_.rt_octree_dump(ptr(tris), tris.shape[0], max_depth, leaf_max, buf, n)
    return buf.raw


class BVH:
    """BVH(triangles, max_depth=32, leaf_max_obj_count=8) (bvh.cpp:19-37).

    The octree itself is built natively when a RenderKernel binds it. Pass
    ``preorder=`` (a pre-order walk of a reference BVH::_root) to bind an
    externally built tree instead."""

    def __init__(self, triangles, max_depth: int = 32, leaf_max_obj_count: int = 8, preorder: bytes | None = None):
        self.triangles = triangles
        self.max_depth = max_depth
        self.leaf_max_obj_count = leaf_max_obj_count
        self.preorder = preorder


# -------------------------------------------------------------- RenderKernel
class RenderKernel:
    """RenderKernel(width, height, render_samples, max_bounces, image_buffer,
    triangles, materials, emissive_triangle_indices, materials_indices,
    analytic_spheres, bvh, skysphere, env_map_cdf) — render_kernel.h:24-46.

    device: a HIP ordinal, or a sequence of them for one context over several
    GPUs (rt_create_multi: rows sharded over the devices, RCCL scatter/gather
    through the first). Like the reference, which keeps a reference to the
    material vector (render_kernel.h:81-93), a render picks up in-place edits
    of `materials_buffer` (rt_set_materials: no BVH rebuild); the triangles,
    BVH and sky are bound at construction."""

    def __init__(self, width, height, render_samples, max_bounces, image_buffer: Image, triangle_buffer,
                 materials_buffer, emissive_triangle_indices_buffer, materials_indices_buffer, analytic_spheres_buffer,
                 bvh: BVH, skysphere: Image, env_map_cdf, device=0, hostsim: bool = False, loopback: bool = False,
                 rccl_clique: bool = False):
        self.L = lib(hostsim)
        self.width, self.height = int(width), int(height)
        self.render_samples, self.max_bounces = int(render_samples), int(max_bounces)
        self.frame_buffer = image_buffer
        h = ctypes.c_void_p()
        if isinstance(device, (list, tuple)):
            # loopback (tests / rehearsals only): the list may repeat a GPU, shards move by device copies
            ids = np.ascontiguousarray(device, dtype=np.int32)
            # rccl_clique (tests only): the RCCL driver even for one device (rt_test_create_multi_rccl)
            create = (self.L.rt_create_multi_loopback if loopback else
                      self.L.rt_test_create_multi_rccl if rccl_clique else self.L.rt_create_multi)
            check(self.L, create(ids.shape[0], ptr(ids), ctypes.byref(h)), None, "rt_create_multi")
        else:
            check(self.L, self.L.rt_create(int(device), ctypes.byref(h)), None, "rt_create")
        self.ctx = h
        self.n_devices = int(self.L.rt_device_count(self.ctx))
        tris = np.ascontiguousarray(triangle_buffer, dtype=np.float32).reshape(-1, 9)
        mats = np.ascontiguousarray(materials_buffer, dtype=np.float32).reshape(-1, 10)
        self.materials_buffer = materials_buffer if isinstance(materials_buffer, np.ndarray) else mats
        self._mats_sent = mats.copy()
        em = np.ascontiguousarray(emissive_triangle_indices_buffer, dtype=np.int32)
        mi = np.ascontiguousarray(materials_indices_buffer, dtype=np.int32)
        sph = np.ascontiguousarray(analytic_spheres_buffer if analytic_spheres_buffer is not None else np.zeros((0, 5)),
                                   dtype=np.float32).reshape(-1, 5)
        check(self.L, self.L.rt_set_scene(self.ctx, ptr(tris), tris.shape[0], ptr(mi), mi.shape[0], ptr(mats),
                                          mats.shape[0], ptr(em), em.shape[0], ptr(sph), sph.shape[0]), self.ctx,
              "rt_set_scene")
        if bvh.preorder is not None:
            buf = ctypes.create_string_buffer(bvh.preorder, len(bvh.preorder))
            check(self.L, self.L.rt_set_bvh_preorder(self.ctx, buf, len(bvh.preorder)), self.ctx, "rt_set_bvh_preorder")
        else:
            check(self.L, self.L.rt_build_bvh(self.ctx, bvh.max_depth, bvh.leaf_max_obj_count), self.ctx,
                  "rt_build_bvh")
        cdf = None if env_map_cdf is None else np.ascontiguousarray(env_map_cdf, dtype=np.float32)
        check(self.L, self.L.rt_set_env(self.ctx, ptr(skysphere.pixels), skysphere.width, skysphere.height, 4,
                                        ptr(cdf)), self.ctx, "rt_set_env")
        self.set_camera(Camera())

    def __del__(self):
        if getattr(self, "ctx", None):
            self.L.rt_destroy(self.ctx)
            self.ctx = None

    def set_camera(self, camera: Camera):
        self.camera = camera
        check(self.L, self.L.rt_set_camera(self.ctx, ptr(camera.view_matrix), camera.fov_dist), self.ctx,
              "rt_set_camera")

    def _sync_materials(self):
        """Push the material table again if the caller edited it in place."""
        m = np.ascontiguousarray(self.materials_buffer, dtype=np.float32).reshape(-1, 10)
        if m.shape != self._mats_sent.shape or not np.array_equal(m.view(np.uint32), self._mats_sent.view(np.uint32)):
            self.set_materials(m)

    def set_materials(self, materials):
        """rt_set_materials: a new material table for the bound scene (the cfg5 sweep)."""
        m = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 10)
        check(self.L, self.L.rt_set_materials(self.ctx, ptr(m), m.shape[0]), self.ctx, "rt_set_materials")
        self._mats_sent = m.copy()

    def render(self):
        self._sync_materials()
        fb = self.frame_buffer.pixels
        assert fb.flags.c_contiguous and fb.dtype == np.float32 and fb.shape == (self.height, self.width, 4)
        check(self.L, self.L.rt_render(self.ctx, self.width, self.height, self.render_samples, self.max_bounces,
                                       ptr(fb)), self.ctx, "rt_render")

    def render_device(self, d_fb: int, row_offset: int = 0, row_stride: int = 1, stream: int | None = None):
        """Render into a device buffer (e.g. a torch tensor's data_ptr()); no host copies."""
        self._sync_materials()
        check(self.L, self.L.rt_render_device(self.ctx, self.width, self.height, self.render_samples,
                                              self.max_bounces, ctypes.c_void_p(d_fb), row_offset, row_stride,
                                              ctypes.c_void_p(stream) if stream else None), self.ctx,
              "rt_render_device")

    # ---- linear radiance and the display stage (rt_render_linear, rt_display; include/rt_hip.h)
    def render_linear(self):
        """render() without the tone-map: the bound Image ends as entry.rgb + final_color / samples, alpha
        untouched (the reference's hdrColor). display() of it at the defaults is render()'s frame."""
        self._sync_materials()
        fb = self.frame_buffer.pixels
        assert fb.flags.c_contiguous and fb.dtype == np.float32 and fb.shape == (self.height, self.width, 4)
        check(self.L, self.L.rt_render_linear(self.ctx, self.width, self.height, self.render_samples,
                                              self.max_bounces, ptr(fb)), self.ctx, "rt_render_linear")

    def render_linear_device(self, d_fb: int, row_offset: int = 0, row_stride: int = 1, stream: int | None = None):
        """rt_render_linear_device: the same into a device buffer; no host copies, no wait."""
        self._sync_materials()
        check(self.L, self.L.rt_render_linear_device(self.ctx, self.width, self.height, self.render_samples,
                                                     self.max_bounces, ctypes.c_void_p(d_fb), row_offset, row_stride,
                                                     ctypes.c_void_p(stream) if stream else None), self.ctx,
              "rt_render_linear_device")

    def display(self, linear: Image | None = None, exposure: float = 1.5, gamma: float = 2.2, flip_y: bool = False,
                want=("rgba",)):
        """rt_display: the exposure / gamma tone-map of a linear frame (default: the bound Image, after
        render_linear()). want names the outputs: "rgba" a new Image, "rgba8" a [h, w, 4] uint8 array of
        write_image_png's conversion (rows reversed when flip_y). One name: that output; both: the pair,
        in want's order."""
        linear = self.frame_buffer if linear is None else linear
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in ("rgba", "rgba8") for k in want):
            raise ValueError(f"display: want {want!r} must name 'rgba', 'rgba8' or both")
        src = np.ascontiguousarray(linear.pixels, dtype=np.float32)
        h, w = src.shape[:2]
        out = Image(w, h) if "rgba" in want else None
        out8 = np.empty((h, w, 4), np.uint8) if "rgba8" in want else None
        p = DisplayParams(float(exposure), float(gamma), int(bool(flip_y)))
        check(self.L, self.L.rt_display(self.ctx, w, h, ptr(src), ctypes.byref(p), None if out is None else ptr(out.pixels),
                                        ptr(out8)), self.ctx, "rt_display")
        got = tuple(out if k == "rgba" else out8 for k in want)
        return got[0] if len(got) == 1 else got

    def display_device(self, d_linear: int, d_rgba: int | None = None, d_rgba8: int | None = None, exposure: float = 1.5,
                       gamma: float = 2.2, flip_y: bool = False, stream: int | None = None, width=None, height=None):
        """rt_display_device: device buffers (w*h*4 floats in and out, w*h*4 bytes), no wait; d_rgba may be
        d_linear (in place)."""
        p = DisplayParams(float(exposure), float(gamma), int(bool(flip_y)))
        check(self.L, self.L.rt_display_device(self.ctx, int(width or self.width), int(height or self.height),
                                               _vp(d_linear), ctypes.byref(p), _vp(d_rgba), _vp(d_rgba8), _vp(stream)),
              self.ctx, "rt_display_device")

    # ---- exposure metering (rt_meter, rt_meter_solve; include/rt_hip.h)
    def meter(self, linear=None) -> np.ndarray:
        """rt_meter: the luminance histogram of a linear frame (an Image or a [h, w, 4] float32 array; default:
        the bound Image, after render_linear()): the 264 uint32 words of rt_meter_hist, 256 bins of an eighth
        of an octave over [2^-20, 2^12) and the stat words (meter_stats names them). It needs no scene."""
        linear = self.frame_buffer if linear is None else linear
        src = np.ascontiguousarray(getattr(linear, "pixels", linear), dtype=np.float32)
        assert src.ndim == 3 and src.shape[2] == 4, "a linear frame is [h, w, 4] float32"
        h, w = src.shape[:2]
        hist = np.empty(METER_WORDS, np.uint32)
        check(self.L, self.L.rt_meter(self.ctx, w, h, ptr(src), ptr(hist)), self.ctx, "rt_meter")
        return hist

    def meter_device(self, d_linear: int, d_hist: int, stream: int | None = None, width=None, height=None):
        """rt_meter_device: device buffers (w*h*4 floats in, 264 words out, cleared by the call), no wait."""
        check(self.L, self.L.rt_meter_device(self.ctx, int(width or self.width), int(height or self.height), _vp(d_linear),
                                             _vp(d_hist), _vp(stream)), self.ctx, "rt_meter_device")

    def auto_exposure(self, linear=None, prev: float = 0.0, dt: float = 0.0, full: bool = False, **params):
        """meter(), then meter_solve: the exposure display() should take for this linear frame. prev / dt and
        params as meter_solve's. Returns the exposure, or with full the whole result and the histogram
        ({"exposure", "target", "log2_mean", "valid", "hist"})."""
        hist = self.meter(linear)
        r = _meter_solve(self.L, hist, prev, dt, params)
        return dict(r, hist=hist) if full else r["exposure"]

    # ---- progressive rendering (rt_progress_*, include/rt_hip.h)
    def progress_begin(self, samples_total: int | None = None, row_offset: int = 0, row_stride: int = 1):
        """Begin a frame of samples_total samples (default: render_samples) rendered in passes, over the
        rows row_offset::row_stride of the bound Image, whose values are the base the frame adds to."""
        self._sync_materials()
        total = self.render_samples if samples_total is None else int(samples_total)
        base = np.ascontiguousarray(self.frame_buffer.pixels[row_offset::row_stride], dtype=np.float32)
        check(self.L, self.L.rt_progress_begin(self.ctx, self.width, self.height, total, self.max_bounces, ptr(base),
                                               row_offset, row_stride), self.ctx, "rt_progress_begin")

    def progress_advance(self, samples: int, stream: int | None = None):
        """The next min(samples, remaining) samples of every pixel. Returns the samples done so far."""
        check(self.L, self.L.rt_progress_advance(self.ctx, int(samples), ctypes.c_void_p(stream) if stream else None),
              self.ctx, "rt_progress_advance")
        return self.progress_info()["done"]

    def progress_info(self) -> dict:
        info = np.zeros(8, np.int32)
        check(self.L, self.L.rt_progress_info(self.ctx, ptr(info)), self.ctx, "rt_progress_info")
        keys = ("width", "height", "total", "done", "bounces", "row_offset", "row_stride", "rows_local")
        return {k: int(v) for k, v in zip(keys, info)}

    def progress_resolve(self, image: Image | None = None) -> Image:
        """The image after the samples done so far into the shard's rows of `image` (default: the bound
        Image). Before the last pass it is a preview: the mean of the first `done` samples of the
        samples_total chain, not the frame a render of `done` samples gives."""
        image = self.frame_buffer if image is None else image
        i = self.progress_info()
        out = np.empty((i["rows_local"], self.width, 4), np.float32)
        check(self.L, self.L.rt_progress_resolve(self.ctx, ptr(out)), self.ctx, "rt_progress_resolve")
        image.pixels[i["row_offset"]::i["row_stride"]] = out
        return image

    def progress_resolve_device(self, d_fb: int, stream: int | None = None):
        check(self.L, self.L.rt_progress_resolve_device(self.ctx, ctypes.c_void_p(d_fb),
                                                        ctypes.c_void_p(stream) if stream else None), self.ctx,
              "rt_progress_resolve_device")

    def progress_resolve_linear(self, image: Image | None = None) -> Image:
        """progress_resolve without the tone-map: base + state.rgb / done, the base's alpha, into the
        shard's rows of `image` (default: the bound Image)."""
        image = self.frame_buffer if image is None else image
        i = self.progress_info()
        out = np.empty((i["rows_local"], self.width, 4), np.float32)
        check(self.L, self.L.rt_progress_resolve_linear(self.ctx, ptr(out)), self.ctx, "rt_progress_resolve_linear")
        image.pixels[i["row_offset"]::i["row_stride"]] = out
        return image

    def progress_resolve_linear_device(self, d_fb: int, stream: int | None = None):
        """rt_progress_resolve_linear_device: the same into a device buffer (rows_local*w*4 floats) on
        `stream`; no wait."""
        check(self.L, self.L.rt_progress_resolve_linear_device(self.ctx, ctypes.c_void_p(d_fb),
                                                               ctypes.c_void_p(stream) if stream else None), self.ctx,
              "rt_progress_resolve_linear_device")

    def progress_save(self) -> bytes:
        """The checkpoint: header, base, state. It does not fingerprint the scene."""
        n = int(self.L.rt_progress_save(self.ctx, None, 0))
        if n < 0:
            check(self.L, n, self.ctx, "rt_progress_save")
        buf = ctypes.create_string_buffer(n)
        got = int(self.L.rt_progress_save(self.ctx, buf, n))
        if got != n:
            check(self.L, got if got < 0 else RT_ERR_STATE, self.ctx, "rt_progress_save")
        return buf.raw

    def progress_load(self, data: bytes):
        """Install a checkpoint of the same scene, env, camera and intersect mode at its `done`."""
        self._sync_materials()
        buf = ctypes.create_string_buffer(data, len(data))
        check(self.L, self.L.rt_progress_load(self.ctx, buf, len(data)), self.ctx, "rt_progress_load")

    def progress_end(self):
        self.L.rt_progress_end(self.ctx)

    # ---- noise estimate of a progression (rt_progress_noise_track, rt_progress_noise; include/rt_hip.h)
    def progress_track_noise(self):
        """Track the running progression (before its first pass): it keeps the sum of the samples of its
        even-numbered passes, which progress_noise compares with the sum of all of them."""
        check(self.L, self.L.rt_progress_noise_track(self.ctx), self.ctx, "rt_progress_noise_track")

    def progress_noise(self, threshold: float, pixel_map: bool = False, tile_map: bool = False) -> dict:
        """rt_progress_noise after at least two passes: the stats as a dict (max_tile, tiles, tiles_over,
        nonfinite, samples_a, samples_b, passes), with "pixel_err" [rows_local, w] and "tile_err"
        [ceil(rows_local / 8), ceil(w / 8)] float32 arrays when asked for. tiles_over == 0: every 8x8 tile's
        error is at or below the threshold."""
        i = self.progress_info()
        rows, w = i["rows_local"], self.width
        px = np.empty((rows, w), np.float32) if pixel_map else None
        tl = np.empty(((rows + 7) // 8, (w + 7) // 8), np.float32) if tile_map else None
        st = NoiseStats()
        check(self.L, self.L.rt_progress_noise(self.ctx, float(threshold), ctypes.byref(st), ptr(px), ptr(tl)), self.ctx,
              "rt_progress_noise")
        out = {k: getattr(st, k) for k, _ in NoiseStats._fields_}
        if pixel_map:
            out["pixel_err"] = px
        if tile_map:
            out["tile_err"] = tl
        return out

    # ---- adaptive sampling (rt_progress_advance_adaptive, rt_progress_tile_counts; include/rt_hip.h)
    def progress_advance_adaptive(self, samples: int, threshold: float, stream: int | None = None) -> dict:
        """One adaptive pass of a tracked progression: `samples` more samples for every 8x8 tile whose noise
        estimate is above `threshold` and that still fits under the total (every tile that fits during the first
        two passes). Returns {"active_tiles", "active_pixels", "capped_tiles", "min_count", "max_count", "tiles"};
        active_tiles == 0: nothing was rendered."""
        info = np.zeros(8, np.int32)
        check(self.L, self.L.rt_progress_advance_adaptive(self.ctx, int(samples), float(threshold),
                                                          ctypes.c_void_p(stream) if stream else None, ptr(info)),
              self.ctx, "rt_progress_advance_adaptive")
        keys = ("active_tiles", "active_pixels", "capped_tiles", "min_count", "max_count", "tiles")
        return {k: int(v) for k, v in zip(keys, info)}

    def progress_tile_counts(self):
        """(tile_n, tile_nA): [ceil(rows_local / 8), ceil(w / 8)] int32 arrays, the samples every pixel of the
        tile has done and how many of them fell in A passes. Waits for the passes."""
        i = self.progress_info()
        shape = ((i["rows_local"] + 7) // 8, (self.width + 7) // 8)
        n, na = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        check(self.L, self.L.rt_progress_tile_counts(self.ctx, ptr(n), ptr(na)), self.ctx, "rt_progress_tile_counts")
        return n, na

    # ---- post stage (what replaces Utils::OIDN_denoise, utils.cpp:144-196)
    def camera_rays(self) -> np.ndarray:
        """rt_camera_rays: the feature pass's rays, [h, w, 6] = origin, direction (host only)."""
        rays = np.empty((self.height, self.width, 6), np.float32)
        check(self.L, self.L.rt_camera_rays(self.ctx, self.width, self.height, ptr(rays)), self.ctx, "rt_camera_rays")
        return rays

    def features(self, size=None):
        """rt_render_features: (albedo, normal_depth), each [h, w, 4] float32: the first hit of
        every pixel's centre ray, {diffuse rgb, 0} and {n.xyz, t} (miss: zeros and t = -1).
        size: (w, h) of the guides, default the kernel's own (upscale() takes them at both sizes)."""
        self._sync_materials()
        w, h = size if size is not None else (self.width, self.height)
        alb = np.empty((h, w, 4), np.float32)
        nd = np.empty_like(alb)
        check(self.L, self.L.rt_render_features(self.ctx, w, h, ptr(alb), ptr(nd)), self.ctx, "rt_render_features")
        return alb, nd

    def features_device(self, d_albedo: int, d_normal_depth: int, stream: int | None = None):
        """rt_render_features_device: the same into device buffers (w*h*4 floats each); no wait."""
        self._sync_materials()
        check(self.L, self.L.rt_render_features_device(self.ctx, self.width, self.height, ctypes.c_void_p(d_albedo),
                                                       ctypes.c_void_p(d_normal_depth),
                                                       ctypes.c_void_p(stream) if stream else None), self.ctx,
              "rt_render_features_device")

    # ---- first-hit G-buffer on the render's walks (rt_render_gbuffer; include/rt_hip.h)
    def gbuffer(self, size=None, exact: bool = False, ids: bool = False):
        """rt_render_gbuffer: features()' (albedo, normal_depth) from the search-BVH walks with the
        8-lane exact walk behind them; ids=True adds [h, w, 2] int32 = {primitive, material index},
        {-1, -1} for a miss. exact=True sends every pixel down the exact walk (RT_GBUFFER_EXACT):
        features()' bits with no exception. size: (w, h), default the kernel's own."""
        self._sync_materials()
        w, h = size if size is not None else (self.width, self.height)
        alb = np.empty((h, w, 4), np.float32)
        nd = np.empty_like(alb)
        pid = np.empty((h, w, 2), np.int32) if ids else None
        check(self.L, self.L.rt_render_gbuffer(self.ctx, w, h, _capi.GBUFFER_EXACT if exact else 0, ptr(alb), ptr(nd),
                                               ptr(pid)), self.ctx, "rt_render_gbuffer")
        return (alb, nd, pid) if ids else (alb, nd)

    def gbuffer_device(self, d_albedo: int, d_normal_depth: int, d_ids: int | None = None, exact: bool = False,
                       stream: int | None = None, size=None):
        """rt_render_gbuffer_device: the same into device buffers (w*h*4 floats each, ids w*h*2 int32 or
        None); no wait."""
        self._sync_materials()
        w, h = size if size is not None else (self.width, self.height)
        check(self.L, self.L.rt_render_gbuffer_device(self.ctx, w, h, _capi.GBUFFER_EXACT if exact else 0, _vp(d_albedo),
                                                      _vp(d_normal_depth), _vp(d_ids), _vp(stream)), self.ctx,
              "rt_render_gbuffer_device")

    def gbuffer_last_exact(self) -> int:
        """rt_gbuffer_last_exact: pixels of the last gbuffer call that took the exact walk (waits)."""
        r = int(self.L.rt_gbuffer_last_exact(self.ctx))
        if r < 0:
            check(self.L, r, self.ctx, "rt_gbuffer_last_exact")
        return r

    # guides of the stages below: features() or, with guide_source = "walks" (the CLI's --guides=walks), gbuffer()
    guide_source = "exact"

    def guides(self, size=None):
        """The (albedo, normal_depth) pair the stages below are guided by, from guide_source."""
        return self.gbuffer(size) if self.guide_source == "walks" else self.features(size)

    def denoise(self, image: Image | None = None, blend_factor: float = 1.0, guides=True, params=None) -> Image:
        """The call shape of Utils::OIDN_denoise(image, blend_factor): a new Image,
        blend_factor * filtered + (1 - blend_factor) * image, alpha 1. image: default the frame
        buffer. guides: True renders the feature buffers for the bound camera, False filters
        on colour alone, or an (albedo, normal_depth) pair from features(). params: None, a
        DenoiseParams or a dict of its fields."""
        image = self.frame_buffer if image is None else image
        src = np.ascontiguousarray(image.pixels, dtype=np.float32)
        h, w = src.shape[:2]
        alb = nd = None
        if guides is True:
            assert (w, h) == (self.width, self.height), "guides are rendered at the kernel's own size"
            alb, nd = self.guides()
        elif guides:
            alb, nd = (np.ascontiguousarray(g, dtype=np.float32).reshape(h, w, 4) for g in guides)
        out = Image(w, h)
        p = _params(self.L, DenoiseParams, "denoise", params)
        check(self.L, self.L.rt_denoise(self.ctx, w, h, ptr(src), ptr(alb), ptr(nd), ctypes.byref(p),
                                        float(blend_factor), ptr(out.pixels)), self.ctx, "rt_denoise")
        return out

    def denoise_device(self, d_in: int, d_out: int, d_albedo: int | None = None, d_normal_depth: int | None = None,
                       blend_factor: float = 1.0, params=None, stream: int | None = None, width=None, height=None):
        """rt_denoise_device: device buffers (w*h*4 floats each), no wait."""
        p = _params(self.L, DenoiseParams, "denoise", params)
        check(self.L, self.L.rt_denoise_device(self.ctx, int(width or self.width), int(height or self.height), _vp(d_in),
                                               _vp(d_albedo), _vp(d_normal_depth), ctypes.byref(p), float(blend_factor),
                                               _vp(d_out), _vp(stream)), self.ctx, "rt_denoise_device")

    # ---- variance-guided denoise (rt_progress_noise_sigma, rt_denoise_var; include/rt_hip.h)
    def progress_noise_sigma(self) -> np.ndarray:
        """rt_progress_noise_sigma after at least two passes of a tracked progression: [rows_local, w]
        float32, the noise estimate's numerator k * d per pixel, in the units of the linear frame."""
        i = self.progress_info()
        s = np.empty((i["rows_local"], self.width), np.float32)
        check(self.L, self.L.rt_progress_noise_sigma(self.ctx, ptr(s)), self.ctx, "rt_progress_noise_sigma")
        return s

    def progress_noise_sigma_device(self, d_sigma: int, stream: int | None = None):
        """rt_progress_noise_sigma_device: the same into a device buffer (rows_local*w floats); no wait."""
        check(self.L, self.L.rt_progress_noise_sigma_device(self.ctx, ctypes.c_void_p(d_sigma),
                                                            ctypes.c_void_p(stream) if stream else None), self.ctx,
              "rt_progress_noise_sigma_device")

    def denoise_var(self, image: Image | None = None, sigma=None, blend_factor: float = 1.0, guides=True, params=None,
                    return_sigma: bool = False):
        """denoise() with the colour edge-stop scaled per pixel by sigma ([h, w] float32, a standard
        deviation of the image's colour; None: progress_noise_sigma() of the live progression, which
        must cover the whole frame). params: None, a DenoiseVarParams or a dict of its fields.
        return_sigma: (Image, sigma_out), the standard deviation left after the last pass."""
        image = self.frame_buffer if image is None else image
        src = np.ascontiguousarray(image.pixels, dtype=np.float32)
        h, w = src.shape[:2]
        sig = self.progress_noise_sigma() if sigma is None else sigma
        sig = np.ascontiguousarray(sig, dtype=np.float32)
        assert sig.shape == (h, w), "sigma is one float per pixel of the image"
        alb = nd = None
        if guides is True:
            assert (w, h) == (self.width, self.height), "guides are rendered at the kernel's own size"
            alb, nd = self.guides()
        elif guides:
            alb, nd = (np.ascontiguousarray(g, dtype=np.float32).reshape(h, w, 4) for g in guides)
        out = Image(w, h)
        left = np.empty((h, w), np.float32) if return_sigma else None
        p = _params(self.L, DenoiseVarParams, "denoise_var", params)
        check(self.L, self.L.rt_denoise_var(self.ctx, w, h, ptr(src), ptr(sig), ptr(alb), ptr(nd), ctypes.byref(p),
                                            float(blend_factor), ptr(out.pixels), ptr(left)), self.ctx, "rt_denoise_var")
        return (out, left) if return_sigma else out

    def denoise_var_device(self, d_in: int, d_sigma: int, d_out: int, d_albedo: int | None = None,
                           d_normal_depth: int | None = None, blend_factor: float = 1.0, params=None,
                           d_sigma_out: int | None = None, stream: int | None = None, width=None, height=None):
        """rt_denoise_var_device: device buffers (w*h*4 floats each, sigma and sigma_out w*h floats), no wait."""
        p = _params(self.L, DenoiseVarParams, "denoise_var", params)
        check(self.L, self.L.rt_denoise_var_device(self.ctx, int(width or self.width), int(height or self.height), _vp(d_in),
                                                   _vp(d_sigma), _vp(d_albedo), _vp(d_normal_depth), ctypes.byref(p),
                                                   float(blend_factor), _vp(d_out), _vp(d_sigma_out), _vp(stream)), self.ctx,
              "rt_denoise_var_device")

    # ---- temporal accumulation (rt_temporal_accumulate; include/rt_hip.h)
    def temporal_accumulate(self, image: Image, sigma, normal_depth, prev_camera: Camera, history=None, params=None):
        """rt_temporal_accumulate: the history reprojected from prev_camera into the kernel's current camera
        and blended with this frame. image: a linear frame (progress_resolve_linear); sigma: [h, w] float32,
        its standard deviation (progress_noise_sigma); normal_depth: features()[1] under the current camera;
        history: None (the first frame) or (rgba, sigma, length, normal_depth), the previous call's result
        and the previous frame's normal_depth. params: None, a TemporalParams or a dict of its fields.
        Returns (rgba Image, sigma [h, w], length [h, w])."""
        src = np.ascontiguousarray(image.pixels, dtype=np.float32)
        h, w = src.shape[:2]
        sig = np.ascontiguousarray(sigma, dtype=np.float32)
        nd = np.ascontiguousarray(normal_depth, dtype=np.float32)
        assert sig.shape == (h, w) and nd.shape == (h, w, 4), "sigma is one float per pixel, normal_depth four"
        hist = [None] * 4
        if history is not None:
            shapes = ((h, w, 4), (h, w), (h, w), (h, w, 4))
            hist = [np.ascontiguousarray(getattr(a, "pixels", a), dtype=np.float32).reshape(s)
                    for a, s in zip(history, shapes)]
        out, s_out, l_out = Image(w, h), np.empty((h, w), np.float32), np.empty((h, w), np.float32)
        p = _params(self.L, TemporalParams, "temporal", params)
        check(self.L, self.L.rt_temporal_accumulate(self.ctx, w, h, ptr(src), ptr(sig), ptr(nd), ptr(prev_camera.view_matrix),
                                                    prev_camera.fov_dist, *(ptr(a) for a in hist), ctypes.byref(p),
                                                    ptr(out.pixels), ptr(s_out), ptr(l_out)), self.ctx,
              "rt_temporal_accumulate")
        return out, s_out, l_out

    def temporal_accumulate_device(self, d_in: int, d_sigma: int, d_normal_depth: int, prev_camera: Camera, d_out: int,
                                   d_sigma_out: int, d_len_out: int, d_history=None, params=None,
                                   stream: int | None = None, width=None, height=None):
        """rt_temporal_accumulate_device: device buffers (w*h*4 floats for the float4 buffers, w*h floats for the
        others), d_history None or (d_rgba, d_sigma, d_len, d_normal_depth); no wait."""
        p = _params(self.L, TemporalParams, "temporal", params)
        hist = d_history if d_history is not None else (None,) * 4
        check(self.L, self.L.rt_temporal_accumulate_device(self.ctx, int(width or self.width), int(height or self.height),
                                                           _vp(d_in), _vp(d_sigma), _vp(d_normal_depth),
                                                           ptr(prev_camera.view_matrix), prev_camera.fov_dist,
                                                           *(_vp(a) for a in hist), ctypes.byref(p), _vp(d_out),
                                                           _vp(d_sigma_out), _vp(d_len_out), _vp(stream)), self.ctx,
              "rt_temporal_accumulate_device")

    # ---- firefly rejection (rt_firefly; include/rt_hip.h)
    def firefly_clamp(self, image: Image, sigma=None, params=None, return_scale: bool = False):
        """rt_firefly: every pixel of a linear frame whose luminance is above gain * M + floor, M the rank-th
        largest luminance among its neighbours, scaled down to that limit, and its sigma ([h, w] float32, or None)
        with it. params: None, a FireflyParams or a dict of its fields. Returns (Image, sigma_out), sigma_out None
        without a sigma; return_scale: (Image, sigma_out, scale), scale [h, w] float32, below 1 where clamped."""
        src = np.ascontiguousarray(image.pixels, dtype=np.float32)
        h, w = src.shape[:2]
        sig = s_out = None
        if sigma is not None:
            sig = np.ascontiguousarray(sigma, dtype=np.float32)
            assert sig.shape == (h, w), "sigma is one float per pixel of the image"
            s_out = np.empty((h, w), np.float32)
        out = Image(w, h)
        scale = np.empty((h, w), np.float32) if return_scale else None
        p = _params(self.L, FireflyParams, "firefly", params)
        check(self.L, self.L.rt_firefly(self.ctx, w, h, ptr(src), ptr(sig), ctypes.byref(p), ptr(out.pixels), ptr(s_out),
                                        ptr(scale)), self.ctx, "rt_firefly")
        return (out, s_out, scale) if return_scale else (out, s_out)

    def firefly_clamp_device(self, d_in: int, d_out: int, d_sigma: int | None = None, d_sigma_out: int | None = None,
                             d_scale_out: int | None = None, params=None, stream: int | None = None, width=None,
                             height=None):
        """rt_firefly_device: device buffers (w*h*4 floats for the frames, w*h floats for the others), no wait."""
        p = _params(self.L, FireflyParams, "firefly", params)
        check(self.L, self.L.rt_firefly_device(self.ctx, int(width or self.width), int(height or self.height), _vp(d_in),
                                               _vp(d_sigma), ctypes.byref(p), _vp(d_out), _vp(d_sigma_out), _vp(d_scale_out),
                                               _vp(stream)), self.ctx, "rt_firefly_device")

    # ---- guided upscale (rt_upscale; include/rt_hip.h)
    def upscale(self, low_rgba, low_albedo, low_nd, hi_albedo, hi_nd, sigma=None, params=None):
        """rt_upscale: a low-resolution linear frame (an Image or [h_lo, w_lo, 4] float32) taken to the size of the
        full-size guides by joint-bilateral upsampling along them. low_albedo / low_nd and hi_albedo / hi_nd:
        features() at the two sizes. sigma: the low frame's [h_lo, w_lo] noise figure, or None. params: None, an
        UpscaleParams or a dict of its fields. Returns the Image, or (Image, sigma_out [h, w]) with a sigma."""
        f4 = lambda a: np.ascontiguousarray(a.pixels if isinstance(a, Image) else a, dtype=np.float32)  # noqa: E731
        lo, la, ln, ha, hn = f4(low_rgba), f4(low_albedo), f4(low_nd), f4(hi_albedo), f4(hi_nd)
        h_lo, w_lo = lo.shape[:2]
        h, w = hn.shape[:2]
        assert la.shape == ln.shape == (h_lo, w_lo, 4) and lo.shape == la.shape, "the low frame and its guides: one size"
        assert ha.shape == (h, w, 4) and hn.shape == ha.shape, "the full-size guides: one size"
        sig = s_out = None
        if sigma is not None:
            sig = np.ascontiguousarray(sigma, dtype=np.float32)
            assert sig.shape == (h_lo, w_lo), "sigma is one float per pixel of the low frame"
            s_out = np.empty((h, w), np.float32)
        out = Image(w, h)
        p = _params(self.L, UpscaleParams, "upscale", params)
        check(self.L, self.L.rt_upscale(self.ctx, w_lo, h_lo, w, h, ptr(lo), ptr(sig), ptr(la), ptr(ln), ptr(ha), ptr(hn),
                                        ctypes.byref(p), ptr(out.pixels), ptr(s_out)), self.ctx, "rt_upscale")
        return out if sigma is None else (out, s_out)

    def upscale_device(self, size_lo, size, d_low_rgba: int, d_low_albedo: int, d_low_nd: int, d_hi_albedo: int,
                       d_hi_nd: int, d_out: int, d_sigma: int | None = None, d_sigma_out: int | None = None, params=None,
                       stream: int | None = None):
        """rt_upscale_device: device buffers (4 floats per pixel for the frames and guides, 1 for the sigmas) at
        size_lo = (w_lo, h_lo) and size = (w, h); no wait."""
        p = _params(self.L, UpscaleParams, "upscale", params)
        check(self.L, self.L.rt_upscale_device(self.ctx, int(size_lo[0]), int(size_lo[1]), int(size[0]), int(size[1]),
                                               _vp(d_low_rgba), _vp(d_sigma), _vp(d_low_albedo), _vp(d_low_nd),
                                               _vp(d_hi_albedo), _vp(d_hi_nd), ctypes.byref(p), _vp(d_out), _vp(d_sigma_out),
                                               _vp(stream)), self.ctx, "rt_upscale_device")

    # ---- bloom (rt_bloom; include/rt_hip.h)
    def bloom(self, linear: Image, threshold=None, knee=None, intensity=None, levels=None, return_layer: bool = False,
              params=None):
        """rt_bloom: the energy of a linear frame above `threshold` (luminance, soft knee of half-width `knee`) spread by
        a Gaussian pyramid of `levels` levels and added back, intensity / levels times the pyramid's sum. It goes between
        render_linear() / the last filter and display(). A keyword left None keeps the stage's default (params: a
        BloomParams or a dict of its fields instead). Returns the Image, or (Image, layer) with return_layer: layer
        [h, w, 4] float32 = {what was added, 0}."""
        src = np.ascontiguousarray(linear.pixels, dtype=np.float32)
        h, w = src.shape[:2]
        over = {k: v for k, v in dict(threshold=threshold, knee=knee, intensity=intensity, levels=levels).items() if v is not None}
        p = _params(self.L, BloomParams, "bloom", params if params is not None else over)
        if params is not None:
            for k, v in over.items():
                setattr(p, k, v)
        out = Image(w, h)
        layer = np.empty((h, w, 4), np.float32) if return_layer else None
        check(self.L, self.L.rt_bloom(self.ctx, w, h, ptr(src), ctypes.byref(p), ptr(out.pixels), ptr(layer)), self.ctx,
              "rt_bloom")
        return (out, layer) if return_layer else out

    def bloom_device(self, d_in: int, d_out: int, d_layer_out: int | None = None, params=None, stream: int | None = None,
                     width=None, height=None):
        """rt_bloom_device: device buffers of w*h*4 floats, no wait."""
        p = _params(self.L, BloomParams, "bloom", params)
        check(self.L, self.L.rt_bloom_device(self.ctx, int(width or self.width), int(height or self.height), _vp(d_in),
                                             ctypes.byref(p), _vp(d_out), _vp(d_layer_out), _vp(stream)), self.ctx,
              "rt_bloom_device")

    # ---- depth of field (rt_dof; include/rt_hip.h)
    def dof(self, linear: Image, normal_depth, params=None, coc: bool = False):
        """rt_dof: a thin lens's blur built from a linear frame and its first-hit distances, normal_depth [h, w, 4]
        (features() or gbuffer() at the frame's size; only t is read). It goes behind the last filter or upscale and in
        front of bloom(), auto_exposure() and display(). params: None (the defaults), a DofParams, or a dict of its
        fields over the defaults; focus_at() gives the focus for a pixel. Returns the Image, or (Image, radius) with
        coc: radius [h, w] float32, each pixel's circle of confusion in pixels."""
        src = np.ascontiguousarray(linear.pixels, dtype=np.float32)
        h, w = src.shape[:2]
        nd = np.ascontiguousarray(normal_depth, dtype=np.float32)
        if nd.shape != (h, w, 4):
            raise ValueError(f"dof: normal_depth is {nd.shape}, the frame ({h}, {w}, 4)")
        p = _params(self.L, DofParams, "dof", params)
        out = Image(w, h)
        radius = np.empty((h, w), np.float32) if coc else None
        check(self.L, self.L.rt_dof(self.ctx, w, h, ptr(src), ptr(nd), ctypes.byref(p), ptr(out.pixels), ptr(radius)), self.ctx,
              "rt_dof")
        return (out, radius) if coc else out

    def dof_device(self, d_in: int, d_normal_depth: int, d_out: int, d_coc_out: int | None = None, params=None,
                   stream: int | None = None, width=None, height=None):
        """rt_dof_device: device buffers of w*h*4 floats (d_coc_out: w*h floats or None), no wait."""
        p = _params(self.L, DofParams, "dof", params)
        check(self.L, self.L.rt_dof_device(self.ctx, int(width or self.width), int(height or self.height), _vp(d_in),
                                           _vp(d_normal_depth), ctypes.byref(p), _vp(d_out), _vp(d_coc_out), _vp(stream)),
              self.ctx, "rt_dof_device")

    # ---- motion vectors and motion blur (rt_motion_vectors, rt_motion_blur; include/rt_hip.h)
    def motion_vectors(self, normal_depth, prev_camera: Camera):
        """rt_motion_vectors: [h, w, 2] float32, for every pixel where its first hit stood in prev_camera's frame minus
        where it stands now, in pixels. normal_depth [h, w, 4]: features() or gbuffer() under the kernel's current
        camera. prev_camera: a Camera, or (view_matrix, fov_dist)."""
        nd = np.ascontiguousarray(normal_depth, dtype=np.float32)
        if nd.ndim != 3 or nd.shape[2] != 4:
            raise ValueError(f"motion_vectors: normal_depth is {nd.shape}, not (h, w, 4)")
        h, w = nd.shape[:2]
        view, fov = (prev_camera.view_matrix, prev_camera.fov_dist) if hasattr(prev_camera, "view_matrix") else prev_camera
        view = np.ascontiguousarray(view, dtype=np.float32)
        out = np.empty((h, w, 2), np.float32)
        check(self.L, self.L.rt_motion_vectors(self.ctx, w, h, ptr(nd), ptr(view), float(fov), ptr(out)), self.ctx, "rt_motion_vectors")
        return out

    def motion_vectors_device(self, d_normal_depth: int, prev_camera: Camera, d_motion_out: int, stream: int | None = None,
                              width=None, height=None):
        """rt_motion_vectors_device: device buffers of w*h*4 and w*h*2 floats, no wait."""
        check(self.L, self.L.rt_motion_vectors_device(self.ctx, int(width or self.width), int(height or self.height),
                                                      _vp(d_normal_depth), ptr(prev_camera.view_matrix), prev_camera.fov_dist,
                                                      _vp(d_motion_out), _vp(stream)), self.ctx, "rt_motion_vectors_device")

    def motion_blur(self, linear: Image, normal_depth, motion, params=None, reach: bool = False):
        """rt_motion_blur: a shutter's blur built from a linear frame, its first-hit distances normal_depth [h, w, 4]
        (only t is read) and motion [h, w, 2] (motion_vectors(), or the caller's own). It goes behind dof() and in front
        of bloom(), auto_exposure() and display(). params: None (the defaults), a MotionParams, or a dict of its fields
        over the defaults. Returns the Image, or (Image, reach) with reach: [h, w] float32, each pixel's half streak."""
        src = np.ascontiguousarray(linear.pixels, dtype=np.float32)
        h, w = src.shape[:2]
        nd = np.ascontiguousarray(normal_depth, dtype=np.float32)
        mv = np.ascontiguousarray(motion, dtype=np.float32)
        if nd.shape != (h, w, 4):
            raise ValueError(f"motion_blur: normal_depth is {nd.shape}, the frame ({h}, {w}, 4)")
        if mv.shape != (h, w, 2):
            raise ValueError(f"motion_blur: motion is {mv.shape}, not ({h}, {w}, 2)")
        p = _params(self.L, MotionParams, "motion", params)
        out = Image(w, h)
        r = np.empty((h, w), np.float32) if reach else None
        check(self.L, self.L.rt_motion_blur(self.ctx, w, h, ptr(src), ptr(nd), ptr(mv), ctypes.byref(p), ptr(out.pixels), ptr(r)),
              self.ctx, "rt_motion_blur")
        return (out, r) if reach else out

    def motion_blur_device(self, d_in: int, d_normal_depth: int, d_motion: int, d_out: int, d_reach_out: int | None = None,
                           params=None, stream: int | None = None, width=None, height=None):
        """rt_motion_blur_device: device buffers (w*h*4 floats, d_motion w*h*2, d_reach_out w*h or None), no wait."""
        p = _params(self.L, MotionParams, "motion", params)
        check(self.L, self.L.rt_motion_blur_device(self.ctx, int(width or self.width), int(height or self.height), _vp(d_in),
                                                   _vp(d_normal_depth), _vp(d_motion), ctypes.byref(p), _vp(d_out),
                                                   _vp(d_reach_out), _vp(stream)), self.ctx, "rt_motion_blur_device")

    def render_variants(self, materials, frames=None, device_ptrs=None, row_offset: int = 0, row_stride: int = 1):
        """rt_render_variants: the material sweep as replicas. `materials` is
        [n_variants, n_materials, 10] (or a list of [n_materials, 10] tables); variant v
        renders rows row_offset + j*row_stride of its own frame on device v mod N of the
        context, no exchange between devices. Output into `frames` (host float32
        [n_variants, rows, W, 4], read-modify-written like render()), or into
        `device_ptrs[v]` (device buffers of rows*W*4 floats, each on device v mod N).
        Returns `frames` (host mode). The bound material table is untouched."""
        tabs = np.ascontiguousarray(np.stack([np.asarray(m, np.float32).reshape(-1, 10) for m in materials]),
                                    dtype=np.float32)
        n_var, n_mats = tabs.shape[0], tabs.shape[1]
        rows = len(range(row_offset, self.height, row_stride))
        self._sync_materials()
        if device_ptrs is not None:
            assert len(device_ptrs) == n_var
            arr = (ctypes.c_void_p * n_var)(*[ctypes.c_void_p(int(p)) for p in device_ptrs])
            fb_p, d_p = None, ctypes.cast(arr, ctypes.c_void_p)
        else:
            if frames is None:
                frames = np.zeros((n_var, rows, self.width, 4), np.float32)
                frames[..., 3] = 1.0  # (Image's default alpha, as Image(w, h))
            assert frames.flags.c_contiguous and frames.dtype == np.float32 and frames.shape == (n_var, rows,
                                                                                                  self.width, 4)
            fb_p, d_p = ptr(frames), None
        check(self.L, self.L.rt_render_variants(self.ctx, self.width, self.height, self.render_samples,
                                                self.max_bounces, n_var, ptr(tabs), n_mats, row_offset, row_stride,
                                                fb_p, d_p), self.ctx, "rt_render_variants")
        return frames

    def ray_trace_pixels(self, xy) -> None:
        self._sync_materials()
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        fb = self.frame_buffer.pixels
        rgba = np.ascontiguousarray(fb[xy[:, 1], xy[:, 0]])
        check(self.L, self.L.rt_render_pixels(self.ctx, self.width, self.height, self.render_samples,
                                              self.max_bounces, ptr(xy), xy.shape[0], ptr(rgba)), self.ctx,
              "rt_render_pixels")
        fb[xy[:, 1], xy[:, 0]] = rgba

    def ray_trace_pixel(self, x: int, y: int) -> None:
        self.ray_trace_pixels(np.array([[x, y]], dtype=np.int32))

    def intersect(self, rays) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        out = np.zeros((rays.shape[0], 11), dtype=np.int32)
        check(self.L, self.L.rt_intersect(self.ctx, ptr(rays), rays.shape[0], ptr(out)), self.ctx, "rt_intersect")
        return out

    # ---- batched ray queries (rt_query: the render's search-BVH walks, the exact walk behind them)
    def _query_mode(self, mode, exact) -> int:
        modes = {"closest": _capi.QUERY_CLOSEST, "any": _capi.QUERY_ANY}
        if mode not in modes:
            raise ValueError(f"query mode {mode!r}: 'closest' or 'any'")
        return modes[mode] | (_capi.QUERY_EXACT if exact else 0)

    def query(self, rays, mode: str = "closest", exact: bool = False) -> np.ndarray:
        """rt_query on rays [n, 6] = origin, direction, in the caller's order. mode "closest":
        int32 [n, 11], intersect()'s record bit for bit ({found, primitive, t, point, normal,
        u, v}; .view(np.float32) for the float words); "any": int32 [n], its `found` word.
        exact=True sends every query down the exact walk (RT_QUERY_EXACT)."""
        m = self._query_mode(mode, exact)
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        out = np.zeros((n, 11) if mode == "closest" else (n,), dtype=np.int32)
        check(self.L, self.L.rt_query(self.ctx, m, ptr(rays), n, ptr(out)), self.ctx, "rt_query")
        return out

    def query_device(self, d_rays: int, n: int, d_out: int, mode: str = "closest", exact: bool = False,
                     stream: int | None = None):
        """rt_query_device: device buffers (n*6 floats in, n*11 or n int32 out) on `stream`; no wait."""
        check(self.L, self.L.rt_query_device(self.ctx, self._query_mode(mode, exact), _vp(d_rays), int(n), _vp(d_out),
                                             _vp(stream)), self.ctx, "rt_query_device")

    def query_last_exact(self) -> int:
        """rt_query_last_exact: queries of the last query call that took the exact walk (waits)."""
        r = int(self.L.rt_query_last_exact(self.ctx))
        if r < 0:
            check(self.L, r, self.ctx, "rt_query_last_exact")
        return r

    def set_use_bvh(self, use_bvh: bool = True):
        """USE_BVH (render_kernel.h:13): False switches INTERSECT_SCENE to the
        brute-force intersect_scene loop (render_kernel.cpp:453-483)."""
        check(self.L, self.L.rt_set_intersect_mode(self.ctx, 1 if use_bvh else 0), self.ctx, "rt_set_intersect_mode")

    def test_fail_device(self, device: int = -1):
        """Tests only (rt_test_fail_device): later multi-device renders fail `device` (-1: off)."""
        check(self.L, self.L.rt_test_fail_device(self.ctx, int(device)), self.ctx, "rt_test_fail_device")

    def test_schedule(self, **params):
        """Tests and measurement tools only (rt_test_schedule): override wavefront-schedule
        parameters of the later renders, e.g. test_schedule(lanes=2, tail_paths=0,
        force_fallback=7); reset=1 restores the product's schedule. No parameter changes
        a result."""
        for k, v in params.items():
            check(self.L, self.L.rt_test_schedule(self.ctx, k.encode(), float(v)), self.ctx, "rt_test_schedule")

    def test_walk_log(self, min_calls: int, capacity: int = 1 << 20, sample_every: int = 1):
        """Tests and diagnostics only (rt_test_walk_log): stats renders record every walk of at
        least min_calls quad_visit calls (0: off), or every sample_every-th by a hash."""
        check(self.L, self.L.rt_test_walk_log(self.ctx, int(min_calls), int(sample_every), int(capacity)), self.ctx,
              "rt_test_walk_log")
        self._wlog_cap = int(capacity)

    def walk_log(self) -> tuple[np.ndarray, int]:
        """The last stats render's walk records as a structured array, and how many walks
        qualified (include/rt_hip.h rt_test_walk_log)."""
        cap = getattr(self, "_wlog_cap", 0)
        raw = np.zeros((max(cap, 1), 12), np.float32)
        total = int(self.L.rt_test_walk_log_read(self.ctx, ptr(raw), cap))
        if total < 0:
            check(self.L, total, self.ctx, "rt_test_walk_log_read")
        raw = raw[:min(total, cap)]
        iv = raw.view(np.int32)
        dt = np.dtype([("o", np.float32, 3), ("kind", np.int32), ("where", np.int32), ("d", np.float32, 3),
                       ("calls", np.int32), ("t", np.float32), ("tri", np.int32), ("iter", np.int32), ("slot", np.int32)])
        out = np.zeros(raw.shape[0], dt)
        out["o"], out["kind"], out["where"] = raw[:, 0:3], iv[:, 3] & 0xff, iv[:, 3] >> 8
        out["d"], out["calls"], out["t"] = raw[:, 4:7], iv[:, 7], raw[:, 8]
        out["tri"], out["iter"], out["slot"] = iv[:, 9], iv[:, 10], iv[:, 11]
        return out, total

    def set_stats(self, on):
        """True / 1: counters of the next renders; 2: the same with unpaired occlusion walks
        (the box tests a walk must make: same answers); False / 0: off."""
        self.L.rt_set_stats(self.ctx, int(on) if not isinstance(on, bool) else (1 if on else 0))

    def stats(self) -> dict:
        """Counters of the last render (rt_set_stats(True) first), by name."""
        from ._capi import STAT_NAMES
        n = len(STAT_NAMES)
        out = np.zeros(2 * n, dtype=np.uint64)
        self.L.rt_get_stats(self.ctx, ptr(out), 2 * n)
        d = {k: int(v) for k, v in zip(STAT_NAMES, out[:n])}
        d.update({"tail_" + k: int(v) for k, v in zip(STAT_NAMES, out[n:])})  # the tail kernel's share
        return d

    def kernel_timing(self, enable: int = -1):
        """Per-kernel-class GPU time (HIP events around every launch) since
        timing was last enabled: {class: (total_ms, launches)} for the
        query kernel (k_trace), the path step (k_step, with the exact-walk
        roles) and "other" (the tail kernel k_tail), summed over the
        context's devices. enable=1/0
        turns timing on/off and resets the totals; -1 only reads."""
        ms = np.zeros(3, dtype=np.float64)
        n = np.zeros(3, dtype=np.int64)
        check(self.L, self.L.rt_device_kernel_timing(self.ctx, enable, ptr(ms), ptr(n)), self.ctx, "kernel_timing")
        return {k: (float(a), int(b)) for k, a, b in zip(("trace", "step", "other"), ms, n)}

    def set_lanes(self, lanes: int):
        """Wavefront lanes (streams) per render on every device (1: launches serialized; 0: auto,
        4 for launches of at most 1.5 M pixels, else 3)."""
        check(self.L, self.L.rt_device_set_lanes(self.ctx, int(lanes)), self.ctx, "rt_device_set_lanes")

    def last_iterations(self) -> int:
        return int(self.L.rt_device_last_iterations(self.ctx))

    def exact_handovers(self, reset: bool = False) -> int:
        """Queries the search-BVH walks handed to the exact octree walk in every render since
        the last reset (GPU build; waits for the device): ~2e-6 per sample on cfg2."""
        import ctypes
        v = ctypes.c_ulonglong(0)
        check(self.L, self.L.rt_device_exact_handovers(self.ctx, ctypes.byref(v), 1 if reset else 0), self.ctx,
              "rt_device_exact_handovers")
        return int(v.value)

    def last_kernel_ms(self) -> float:
        return float(self.L.rt_last_kernel_ms(self.ctx))

    def device_last_kernel_ms(self) -> float:
        return float(self.L.rt_device_last_kernel_ms(self.ctx))

    def bvh_info(self) -> dict:
        info = np.zeros(5, dtype=np.int64)
        check(self.L, self.L.rt_bvh_info(self.ctx, ptr(info)), self.ctx, "rt_bvh_info")
        return dict(octree_nodes=int(info[0]), gpu_records=int(info[1]), triangles=int(info[2]),
                    max_depth=int(info[3]), gpu_bytes=int(info[4]))

    def bvh_dump(self) -> bytes:
        n = self.L.rt_bvh_dump(self.ctx, None, 0)
        buf = ctypes.create_string_buffer(n)
        self.L.rt_bvh_dump(self.ctx, buf, n)
        return buf.raw
