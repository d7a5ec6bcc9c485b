"""ctypes bindings for the C ABI in include/rt_hip.h.

``lib()`` loads the product library ``lib/librt_hip.so`` (gfx950 kernels).
There is no CPU fallback: creating a context without a HIP device raises.
``lib(hostsim=True)`` loads ``lib/librt_hostsim.so`` — the same device code
compiled for the host — which only the CPU test-suite uses to validate the
kernel algorithm in a GPU-less container.
"""
from __future__ import annotations

import ctypes
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(PKG_DIR, "lib")
PRODUCT = os.environ.get("RT_HIP_LIB") or os.path.join(LIB_DIR, "librt_hip.so")  # (override: debug builds)
HOSTSIM = os.environ.get("RT_HOSTSIM_LIB") or os.path.join(LIB_DIR, "librt_hostsim.so")  # (override: study builds)

# every symbol declared in include/rt_hip.h (tests check the export table)
EXPORTS = [
    "rt_create", "rt_destroy", "rt_last_error", "rt_version", "rt_build_id", "rt_set_scene", "rt_build_bvh",
    "rt_set_bvh_preorder", "rt_bvh_dump", "rt_bvh_info", "rt_set_env", "rt_set_camera", "rt_render",
    "rt_render_device", "rt_render_pixels", "rt_intersect", "rt_set_stats", "rt_get_stats", "rt_last_kernel_ms",
    "rt_mesh_load", "rt_mesh_counts", "rt_mesh_copy", "rt_mesh_free", "rt_camera_preset", "rt_env_luminance_cdf",
    "rt_octree_dump", "rt_read_hdr", "rt_write_png", "rt_image_to_rgba8",
    "rt_set_intersect_mode", "rt_create_multi", "rt_device_count", "rt_set_materials", "rt_render_variants",
    "rt_create_multi_loopback", "rt_test_create_multi_rccl", "rt_test_fail_device", "rt_test_schedule", "rt_test_walk_log",
    "rt_test_walk_log_read", "rt_test_obj_parallel_min", "rt_device_env_search",
    "rt_camera_rays", "rt_render_features", "rt_render_features_device", "rt_denoise_default_params", "rt_denoise",
    "rt_denoise_device",
    "rt_query", "rt_query_device", "rt_query_last_exact",
    "rt_render_gbuffer", "rt_render_gbuffer_device", "rt_gbuffer_last_exact",
    "rt_progress_begin", "rt_progress_advance", "rt_progress_resolve", "rt_progress_resolve_device",
    "rt_progress_info", "rt_progress_save", "rt_progress_load", "rt_progress_end",
    "rt_display_default_params", "rt_render_linear", "rt_render_linear_device", "rt_progress_resolve_linear",
    "rt_progress_resolve_linear_device", "rt_display", "rt_display_device", "rt_write_hdr",
    "rt_progress_noise_track", "rt_progress_noise", "rt_progress_noise_device",
    "rt_progress_advance_adaptive", "rt_progress_tile_counts",
    "rt_progress_noise_sigma", "rt_progress_noise_sigma_device", "rt_denoise_var_default_params", "rt_denoise_var",
    "rt_denoise_var_device",
    "rt_temporal_default_params", "rt_temporal_accumulate", "rt_temporal_accumulate_device",
    "rt_firefly_default_params", "rt_firefly", "rt_firefly_device",
    "rt_upscale_default_params", "rt_upscale", "rt_upscale_device",
    "rt_meter_default_params", "rt_meter", "rt_meter_device", "rt_meter_solve",
    "rt_bloom_default_params", "rt_bloom", "rt_bloom_device",
    "rt_dof_default_params", "rt_dof", "rt_dof_device",
    "rt_motion_default_params", "rt_motion_vectors", "rt_motion_vectors_device", "rt_motion_blur", "rt_motion_blur_device",
]

# return codes (include/rt_hip.h)
RT_OK, RT_ERR_ARG, RT_ERR_HIP, RT_ERR_STATE, RT_ERR_IO, RT_ERR_NODEV = 0, -1, -2, -3, -4, -5

P = ctypes.c_void_p
I = ctypes.c_int
L = ctypes.c_long
F = ctypes.c_float


class DenoiseParams(ctypes.Structure):
    """struct rt_denoise_params (include/rt_hip.h)."""
    _fields_ = [("passes", ctypes.c_int), ("sigma_color", F), ("sigma_normal", F), ("sigma_albedo", F),
                ("sigma_depth", F)]


class DenoiseVarParams(ctypes.Structure):
    """struct rt_denoise_var_params (include/rt_hip.h)."""
    _fields_ = [("passes", ctypes.c_int), ("sigma_color", F), ("sigma_normal", F), ("sigma_albedo", F),
                ("sigma_depth", F), ("var_floor", F)]


class TemporalParams(ctypes.Structure):
    """struct rt_temporal_params (include/rt_hip.h)."""
    _fields_ = [("depth_tol", F), ("normal_cos", F), ("min_weight", F), ("max_len", F)]


class FireflyParams(ctypes.Structure):
    """struct rt_firefly_params (include/rt_hip.h)."""
    _fields_ = [("radius", I), ("rank", I), ("gain", F), ("floor", F)]


METER_WORDS = 264  # struct rt_meter_hist: 256 bins, then the words named below
METER_STATS = ("counted", "under", "over", "nonpositive", "nonfinite", "max_bits", "min_bits", "reserved")


class MeterParams(ctypes.Structure):
    """struct rt_meter_params (include/rt_hip.h)."""
    _fields_ = [("low", F), ("high", F), ("key", F), ("min_exposure", F), ("max_exposure", F), ("tau_up", F),
                ("tau_down", F)]


class MeterResult(ctypes.Structure):
    """struct rt_meter_result (include/rt_hip.h)."""
    _fields_ = [("exposure", F), ("target", F), ("log2_mean", F), ("valid", I)]


class UpscaleParams(ctypes.Structure):
    """struct rt_upscale_params (include/rt_hip.h)."""
    _fields_ = [("sigma_normal", F), ("sigma_albedo", F), ("sigma_depth", F), ("min_weight", F)]


class BloomParams(ctypes.Structure):
    """struct rt_bloom_params (include/rt_hip.h)."""
    _fields_ = [("threshold", F), ("knee", F), ("intensity", F), ("levels", I)]


class DofParams(ctypes.Structure):
    """struct rt_dof_params (include/rt_hip.h)."""
    _fields_ = [("focus", F), ("coc_inf", F), ("max_radius", I)]


class MotionParams(ctypes.Structure):
    """struct rt_motion_params (include/rt_hip.h)."""
    _fields_ = [("shutter", F), ("depth_soft", F), ("max_radius", I)]


class DisplayParams(ctypes.Structure):
    """struct rt_display_params (include/rt_hip.h)."""
    _fields_ = [("exposure", F), ("gamma", F), ("flip_y", ctypes.c_int)]


class NoiseStats(ctypes.Structure):
    """struct rt_noise_stats (include/rt_hip.h)."""
    _fields_ = [("max_tile", F), ("tiles", I), ("tiles_over", I), ("nonfinite", I), ("samples_a", I), ("samples_b", I),
                ("passes", I)]


_SIGS = {
    "rt_create": (I, [I, ctypes.POINTER(P)]),
    "rt_create_multi": (I, [I, P, ctypes.POINTER(P)]),
    "rt_create_multi_loopback": (I, [I, P, ctypes.POINTER(P)]),
    "rt_test_create_multi_rccl": (I, [I, P, ctypes.POINTER(P)]),
    "rt_test_fail_device": (I, [P, I]),
    "rt_test_schedule": (I, [P, ctypes.c_char_p, ctypes.c_double]),
    "rt_test_walk_log": (I, [P, I, I, I]),
    "rt_test_walk_log_read": (L, [P, P, L]),
    "rt_test_obj_parallel_min": (I, [L]),
    "rt_device_env_search": (I, [P, I, P, I, P]),
    "rt_device_count": (I, [P]),
    "rt_set_materials": (I, [P, P, I]),
    "rt_destroy": (None, [P]),
    "rt_last_error": (ctypes.c_char_p, [P]),
    "rt_version": (I, []),
    "rt_build_id": (ctypes.c_char_p, []),
    "rt_set_scene": (I, [P, P, I, P, I, P, I, P, I, P, I]),
    "rt_build_bvh": (I, [P, I, I]),
    "rt_set_bvh_preorder": (I, [P, P, L]),
    "rt_bvh_dump": (L, [P, P, L]),
    "rt_bvh_info": (I, [P, P]),
    "rt_set_env": (I, [P, P, I, I, I, P]),
    "rt_set_camera": (I, [P, P, F]),
    "rt_render": (I, [P, I, I, I, I, P]),
    "rt_render_device": (I, [P, I, I, I, I, P, I, I, P]),
    "rt_render_pixels": (I, [P, I, I, I, I, P, I, P]),
    "rt_render_variants": (I, [P, I, I, I, I, I, P, I, I, I, P, P]),
    "rt_intersect": (I, [P, P, I, P]),
    "rt_query": (I, [P, I, P, L, P]),
    "rt_query_device": (I, [P, I, P, L, P, P]),
    "rt_query_last_exact": (L, [P]),
    "rt_set_stats": (I, [P, I]),
    "rt_set_intersect_mode": (I, [P, I]),
    "rt_get_stats": (I, [P, P, I]),
    "rt_last_kernel_ms": (ctypes.c_double, [P]),
    "rt_mesh_load": (I, [ctypes.c_char_p, ctypes.POINTER(P)]),
    "rt_mesh_counts": (I, [P, P, P, P]),
    "rt_mesh_copy": (I, [P, P, P, P, P]),
    "rt_mesh_free": (None, [P]),
    "rt_camera_preset": (I, [ctypes.c_char_p, P, P]),
    "rt_env_luminance_cdf": (I, [P, I, I, I, P, P]),
    "rt_octree_dump": (L, [P, I, I, I, P, L]),
    "rt_read_hdr": (I, [ctypes.c_char_p, I, P, P, P]),
    "rt_write_png": (I, [ctypes.c_char_p, P, I, I, I]),
    "rt_image_to_rgba8": (I, [P, L, P]),
    "rt_camera_rays": (I, [P, I, I, P]),
    "rt_render_features": (I, [P, I, I, P, P]),
    "rt_render_features_device": (I, [P, I, I, P, P, P]),
    "rt_render_gbuffer": (I, [P, I, I, I, P, P, P]),
    "rt_render_gbuffer_device": (I, [P, I, I, I, P, P, P, P]),
    "rt_gbuffer_last_exact": (L, [P]),
    "rt_denoise_default_params": (None, [ctypes.POINTER(DenoiseParams)]),
    "rt_denoise": (I, [P, I, I, P, P, P, ctypes.POINTER(DenoiseParams), F, P]),
    "rt_denoise_device": (I, [P, I, I, P, P, P, ctypes.POINTER(DenoiseParams), F, P, P]),
    "rt_progress_begin": (I, [P, I, I, I, I, P, I, I]),
    "rt_progress_advance": (I, [P, I, P]),
    "rt_progress_resolve": (I, [P, P]),
    "rt_progress_resolve_device": (I, [P, P, P]),
    "rt_progress_info": (I, [P, P]),
    "rt_progress_save": (L, [P, P, L]),
    "rt_progress_load": (I, [P, P, L]),
    "rt_progress_end": (None, [P]),
    "rt_display_default_params": (None, [ctypes.POINTER(DisplayParams)]),
    "rt_render_linear": (I, [P, I, I, I, I, P]),
    "rt_render_linear_device": (I, [P, I, I, I, I, P, I, I, P]),
    "rt_progress_resolve_linear": (I, [P, P]),
    "rt_progress_resolve_linear_device": (I, [P, P, P]),
    "rt_display": (I, [P, I, I, P, ctypes.POINTER(DisplayParams), P, P]),
    "rt_display_device": (I, [P, I, I, P, ctypes.POINTER(DisplayParams), P, P, P]),
    "rt_write_hdr": (I, [ctypes.c_char_p, P, I, I, I]),
    "rt_progress_noise_track": (I, [P]),
    "rt_progress_noise": (I, [P, F, ctypes.POINTER(NoiseStats), P, P]),
    "rt_progress_noise_device": (I, [P, F, P, P, P, P]),
    "rt_progress_advance_adaptive": (I, [P, I, F, P, P]),
    "rt_progress_tile_counts": (I, [P, P, P]),
    "rt_progress_noise_sigma": (I, [P, P]),
    "rt_progress_noise_sigma_device": (I, [P, P, P]),
    "rt_denoise_var_default_params": (None, [ctypes.POINTER(DenoiseVarParams)]),
    "rt_denoise_var": (I, [P, I, I, P, P, P, P, ctypes.POINTER(DenoiseVarParams), F, P, P]),
    "rt_denoise_var_device": (I, [P, I, I, P, P, P, P, ctypes.POINTER(DenoiseVarParams), F, P, P, P]),
    "rt_temporal_default_params": (None, [ctypes.POINTER(TemporalParams)]),
    "rt_temporal_accumulate": (I, [P, I, I, P, P, P, P, F, P, P, P, P, ctypes.POINTER(TemporalParams), P, P, P]),
    "rt_temporal_accumulate_device": (I, [P, I, I, P, P, P, P, F, P, P, P, P, ctypes.POINTER(TemporalParams), P, P, P, P]),
    "rt_firefly_default_params": (None, [ctypes.POINTER(FireflyParams)]),
    "rt_firefly": (I, [P, I, I, P, P, ctypes.POINTER(FireflyParams), P, P, P]),
    "rt_firefly_device": (I, [P, I, I, P, P, ctypes.POINTER(FireflyParams), P, P, P, P]),
    "rt_meter_default_params": (None, [ctypes.POINTER(MeterParams)]),
    "rt_meter": (I, [P, I, I, P, P]),
    "rt_meter_device": (I, [P, I, I, P, P, P]),
    "rt_meter_solve": (I, [P, ctypes.POINTER(MeterParams), F, F, ctypes.POINTER(MeterResult)]),
    "rt_upscale_default_params": (None, [ctypes.POINTER(UpscaleParams)]),
    "rt_upscale": (I, [P, I, I, I, I, P, P, P, P, P, P, ctypes.POINTER(UpscaleParams), P, P]),
    "rt_upscale_device": (I, [P, I, I, I, I, P, P, P, P, P, P, ctypes.POINTER(UpscaleParams), P, P, P]),
    "rt_bloom_default_params": (None, [ctypes.POINTER(BloomParams)]),
    "rt_bloom": (I, [P, I, I, P, ctypes.POINTER(BloomParams), P, P]),
    "rt_bloom_device": (I, [P, I, I, P, ctypes.POINTER(BloomParams), P, P, P]),
    "rt_dof_default_params": (None, [ctypes.POINTER(DofParams)]),
    "rt_dof": (I, [P, I, I, P, P, ctypes.POINTER(DofParams), P, P]),
    "rt_dof_device": (I, [P, I, I, P, P, ctypes.POINTER(DofParams), P, P, P]),
    "rt_motion_default_params": (None, [ctypes.POINTER(MotionParams)]),
    "rt_motion_vectors": (I, [P, I, I, P, P, F, P]),
    "rt_motion_vectors_device": (I, [P, I, I, P, P, F, P, P]),
    "rt_motion_blur": (I, [P, I, I, P, P, P, ctypes.POINTER(MotionParams), P, P]),
    "rt_motion_blur_device": (I, [P, I, I, P, P, P, ctypes.POINTER(MotionParams), P, P, P]),
    # product-only extras
    "rt_device_motion_kernel_ms": (I, [P, I, I, P, P, P, ctypes.POINTER(MotionParams), P, P, P, F, P, I, I, P]),
    "rt_device_dof_kernel_ms": (I, [P, I, I, P, P, ctypes.POINTER(DofParams), P, P, I, I, P]),
    "rt_device_bloom_kernel_ms": (I, [P, I, I, P, ctypes.POINTER(BloomParams), P, P, I, I, P]),
    "rt_device_meter_kernel_ms": (I, [P, I, I, P, P, I, I, P]),
    "rt_device_upscale_kernel_ms": (I, [P, I, I, I, I, P, P, P, P, P, P, P, P, I, I, P]),
    "rt_device_libm": (I, [I, I, P, P, P, I]),
    "rt_device_libm_digest": (I, [I, I, ctypes.c_uint32, I, P]),
    "rt_device_last_kernel_ms": (ctypes.c_double, [P]),
    "rt_device_kernel_timing": (I, [P, I, P, P]),
    "rt_device_set_lanes": (I, [P, I]),
    "rt_device_last_iterations": (I, [P]),
    "rt_device_exact_handovers": (I, [P, P, I]),
    "rt_device_queries": (I, [P, I, P, I, I, P, P, P]),
    "rt_device_query_trips": (I, [P, I, P, I, P]),
    "rt_device_denoise_pass_ms": (I, [P, I, P, I]),
    "rt_device_display_kernel_ms": (I, [P, I, I, P, P, P, P, I, P]),
    "rt_device_noise_kernel_ms": (I, [P, I, I, P, P, P, P, P, I, P]),
    "rt_device_adapt_kernel_ms": (I, [P, F, I, P, P]),
    "rt_device_denoise_var_pass_ms": (I, [P, I, P, I]),
    # hostsim-only extra
    "rt_hostsim_heap_order": (I, [P, I, P, P]),
    "rt_hostsim_fast_queries": (I, [P, P, I, P, P]),
    "rt_hostsim_leaf_hits": (I, [P, P, I, P]),
    "rt_hostsim_trip_cases": (I, [P, P, I, P]),
}

# rt_query modes (include/rt_hip.h)
QUERY_CLOSEST, QUERY_ANY, QUERY_EXACT = 0, 1, 0x100
# rt_render_gbuffer flags (include/rt_hip.h)
GBUFFER_EXACT = 0x100

STAT_NAMES = ["rays", "vol", "tri", "leaf", "mat", "env", "cdf", "heap_slow", "any_rays", "any_vol", "any_tri",
              "any_leaf", "verify", "fallback", "quad_visits", "wave_slots", "refills", "drain_slots", "drain_visits",
              "steps"]

_libs: dict = {}


class RtError(RuntimeError):
    pass


def lib(hostsim: bool = False):
    path = HOSTSIM if hostsim else PRODUCT
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RtError(f"{path} is not built: run `make` (or __graft_entry__.build()) first")
    L_ = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(L_, name, None)
        if fn is None:
            continue
        fn.restype = res
        fn.argtypes = args
    _libs[path] = L_
    return L_


def check(L_, rc: int, ctx=None, what: str = ""):
    if rc != 0:
        msg = L_.rt_last_error(ctx)
        raise RtError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
    return rc


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)
