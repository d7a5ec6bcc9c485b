"""The argument errors of the seven frame stages (rt_denoise, rt_denoise_var, rt_temporal_accumulate,
rt_firefly, rt_upscale, rt_meter, rt_display; include/rt_hip.h), both forms, on the hostsim build: one
valid call at 8 x 6 (upscale: 4 x 3 -> 8 x 6), then one call per single violation, enumerated from the
stage's argument list below, and a few calls that break two rules, which pin the order the rules are
applied in. A case's result is (return code, rt_last_error text), the text "" for RT_OK.

Every buffer of a call has a 4 KiB slot of one arena of 0.5f, far more than the frame's 768 bytes, so
a call whose "violation" is none for its stage (rt_meter tests no overlap, rt_display takes its input
as its float output) runs inside the arena. The frame-limit cases pass the small buffers: a stage
with that limit fails before it reads one, and a stage without the row limit (rt_meter, rt_display: no too_many_rows below) has no such case.
Misaligned pointers go to the device form only: the host forms of the hostsim build would read them.

Shared by tools/gen_golden_stage_errors.py, which records tests/golden/stage_errors.json, and
tests/test_stage_errors.py, which replays the calls against it.

Helpers only: no tests here."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from rt_amd import _capi
from rt_amd._capi import (DenoiseParams, DenoiseVarParams, DisplayParams, FireflyParams, TemporalParams,
                          UpscaleParams)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_errors.json")
FORMS = ("host", "device")
W, H, W_LO, H_LO = 8, 6, 4, 3
N, N_LO = W * H, W_LO * H_LO
SLOT = 4096
NAN, INF = float("nan"), float("inf")
VIEW = np.eye(4, dtype=np.float32)  # the camera of the context and prev_view: any invertible matrix
FOV = 2.4142137
PIXELS = dict(w=11586, h=11586)  # 134235396 > 134217727
ROWS = dict(w=1, h=262141)       # 4 * 65535 + 1


def _buf(name, role, required, align, count=N):
    """One buffer argument: count elements of `align` bytes (a float4, a float, a pixel's four bytes, a word)."""
    return dict(name=name, out=role == "out", required=required, align=align, bytes=count * align)


def _sig(*fields):
    return {f: 0.0 for f in fields}


# Per stage: fn (the host form; "_device" appended for the other), args in the C order after ctx (sizes, buffers,
# "params", scalars and "prev_view" by name), bufs, the params struct with one bad value per field, scalars
# {name: (valid, bad)}, pairs {case: overrides} for the rules over optional pointers, limits {case: overrides},
# extras {case: overrides} for a stage's own rules, orders: tuples of case names broken in one call, misaligned:
# False where the device form has no alignment rule.
STAGES = {
    "denoise": dict(
        fn="rt_denoise", sizes=("w", "h"),
        args=("w", "h", "rgba_in", "albedo", "normal_depth", "params", "blend", "rgba_out"),
        bufs=(_buf("rgba_in", "in", True, 16), _buf("albedo", "in", False, 16), _buf("normal_depth", "in", False, 16),
              _buf("rgba_out", "out", True, 16)),
        params=DenoiseParams, bad=dict(passes=0, **_sig("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth")),
        scalars=dict(blend=(0.75, NAN)),
        pairs=dict(albedo_alone=dict(normal_depth=None), normal_depth_alone=dict(albedo=None)),
        limits=dict(too_many_pixels=PIXELS, too_many_rows=ROWS),
        orders=(("ctx_null", "w_zero"), ("h_zero", "too_many_pixels"), ("rgba_out_null", "too_many_rows"),
                ("too_many_pixels", "too_many_rows"), ("too_many_rows", "rgba_out_is_rgba_in"),
                ("rgba_out_is_rgba_in", "albedo_alone"), ("albedo_alone", "params_passes_bad"),
                ("params_sigma_depth_bad", "blend_bad")),
        # (rt_denoise_device has no alignment rule: the hostsim build would read the misaligned float4)
        misaligned=False),
    "denoise_var": dict(
        fn="rt_denoise_var", sizes=("w", "h"),
        args=("w", "h", "rgba_in", "sigma", "albedo", "normal_depth", "params", "blend", "rgba_out", "sigma_out"),
        bufs=(_buf("rgba_in", "in", True, 16), _buf("sigma", "in", True, 4), _buf("albedo", "in", False, 16),
              _buf("normal_depth", "in", False, 16), _buf("rgba_out", "out", True, 16), _buf("sigma_out", "out", False, 4)),
        params=DenoiseVarParams,
        bad=dict(passes=0, **_sig("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth", "var_floor")),
        scalars=dict(blend=(0.75, NAN)),
        pairs=dict(albedo_alone=dict(normal_depth=None), normal_depth_alone=dict(albedo=None), no_sigma_out=dict(sigma_out=None)),
        limits=dict(too_many_pixels=PIXELS, too_many_rows=ROWS),
        orders=(("ctx_null", "w_zero"), ("sigma_null", "rgba_in_null"), ("sigma_null", "too_many_pixels"),
                ("sigma_null", "blend_bad"), ("sigma_null", "params_var_floor_bad"), ("params_var_floor_bad", "params_passes_bad"),
                ("params_var_floor_bad", "sigma_misaligned"), ("rgba_out_is_rgba_in", "sigma_out_misaligned"),
                ("too_many_rows", "albedo_alone"))),
    "temporal": dict(
        fn="rt_temporal_accumulate", sizes=("w", "h"),
        args=("w", "h", "rgba_in", "sigma_in", "normal_depth", "prev_view", "prev_fov_dist", "hist_rgba", "hist_sigma",
              "hist_len", "hist_normal_depth", "params", "rgba_out", "sigma_out", "len_out"),
        bufs=(_buf("rgba_in", "in", True, 16), _buf("sigma_in", "in", True, 4), _buf("normal_depth", "in", True, 16),
              _buf("hist_rgba", "in", False, 16), _buf("hist_sigma", "in", False, 4), _buf("hist_len", "in", False, 4),
              _buf("hist_normal_depth", "in", False, 16), _buf("rgba_out", "out", True, 16), _buf("sigma_out", "out", True, 4),
              _buf("len_out", "out", True, 4)),
        params=TemporalParams, bad=dict(depth_tol=-1.0, normal_cos=2.0, min_weight=1.0, max_len=0.5),
        scalars=dict(prev_fov_dist=(FOV, 0.0)),
        pairs=dict(no_history=dict(hist_rgba=None, hist_sigma=None, hist_len=None, hist_normal_depth=None),
                   no_hist_rgba=dict(hist_rgba=None), no_hist_sigma=dict(hist_sigma=None), no_hist_len=dict(hist_len=None),
                   no_hist_normal_depth=dict(hist_normal_depth=None),
                   hist_rgba_alone=dict(hist_sigma=None, hist_len=None, hist_normal_depth=None)),
        limits=dict(too_many_pixels=PIXELS, too_many_rows=ROWS),
        extras=dict(camera_not_set=dict(ctx="bare"), prev_view_null=dict(prev_view=None), prev_view_singular=dict(prev_view="zero"),
                    params_depth_tol_nan=dict(params=dict(depth_tol=NAN))),
        orders=(("ctx_null", "camera_not_set"), ("camera_not_set", "w_zero"), ("camera_not_set", "rgba_in_null"),
                ("prev_view_null", "too_many_pixels"), ("too_many_rows", "no_hist_len"), ("no_hist_len", "params_max_len_bad"),
                ("params_depth_tol_nan", "params_normal_cos_bad"), ("params_max_len_bad", "prev_fov_dist_bad"),
                ("prev_fov_dist_bad", "sigma_out_is_hist_len"), ("len_out_is_rgba_in", "sigma_out_is_rgba_out"),
                ("len_out_into_sigma_out", "sigma_out_is_hist_rgba"), ("rgba_out_into_rgba_in", "hist_sigma_misaligned"),
                ("len_out_misaligned", "prev_view_singular"))),
    "firefly": dict(
        fn="rt_firefly", sizes=("w", "h"),
        args=("w", "h", "rgba_in", "sigma_in", "params", "rgba_out", "sigma_out", "scale_out"),
        bufs=(_buf("rgba_in", "in", True, 16), _buf("sigma_in", "in", False, 4), _buf("rgba_out", "out", True, 16),
              _buf("sigma_out", "out", False, 4), _buf("scale_out", "out", False, 4)),
        params=FireflyParams, bad=dict(radius=3, rank=9, gain=-1.0, floor=NAN),
        pairs=dict(sigma_out_alone=dict(sigma_in=None), no_sigma=dict(sigma_in=None, sigma_out=None),
                   no_sigma_out=dict(sigma_out=None), no_scale_out=dict(scale_out=None)),
        limits=dict(too_many_pixels=PIXELS, too_many_rows=ROWS),
        orders=(("ctx_null", "w_zero"), ("h_negative", "rgba_in_null"), ("rgba_out_null", "sigma_out_alone"),
                ("sigma_out_alone", "too_many_pixels"), ("too_many_rows", "params_radius_bad"),
                ("params_rank_bad", "params_gain_bad"), ("params_floor_bad", "rgba_out_is_rgba_in"),
                ("scale_out_is_rgba_in", "sigma_out_is_rgba_out"), ("scale_out_into_sigma_out", "sigma_out_is_sigma_in"),
                ("scale_out_is_sigma_out", "rgba_in_misaligned"))),
    "upscale": dict(
        fn="rt_upscale", sizes=("w_lo", "h_lo", "w", "h"),
        args=("w_lo", "h_lo", "w", "h", "rgba_lo", "sigma_lo", "albedo_lo", "normal_depth_lo", "albedo_hi", "normal_depth_hi",
              "params", "rgba_out", "sigma_out"),
        bufs=(_buf("rgba_lo", "in", True, 16, N_LO), _buf("sigma_lo", "in", False, 4, N_LO), _buf("albedo_lo", "in", True, 16, N_LO),
              _buf("normal_depth_lo", "in", True, 16, N_LO), _buf("albedo_hi", "in", True, 16), _buf("normal_depth_hi", "in", True, 16),
              _buf("rgba_out", "out", True, 16), _buf("sigma_out", "out", False, 4)),
        params=UpscaleParams, bad=dict(min_weight=1.0, **_sig("sigma_normal", "sigma_albedo", "sigma_depth")),
        pairs=dict(sigma_out_alone=dict(sigma_lo=None), sigma_lo_alone=dict(sigma_out=None), no_sigma=dict(sigma_lo=None, sigma_out=None)),
        limits=dict(too_many_pixels=PIXELS, too_many_rows=dict(ROWS, w_lo=1)),
        extras=dict(low_frame_wider=dict(w_lo=W + 1), low_frame_taller=dict(h_lo=H + 1)),
        orders=(("ctx_null", "w_lo_zero"), ("h_zero", "low_frame_wider"), ("low_frame_taller", "rgba_lo_null"),
                ("rgba_out_null", "sigma_out_alone"), ("sigma_lo_alone", "too_many_pixels"), ("too_many_rows", "params_sigma_depth_bad"),
                ("params_sigma_normal_bad", "params_min_weight_bad"), ("params_min_weight_bad", "rgba_out_is_rgba_lo"),
                ("sigma_out_is_rgba_out", "sigma_out_is_sigma_lo"), ("sigma_out_is_rgba_out", "rgba_out_is_albedo_hi"),
                ("sigma_out_into_rgba_out", "normal_depth_hi_misaligned"))),
    "meter": dict(
        fn="rt_meter", sizes=("w", "h"), args=("w", "h", "linear", "hist"),
        bufs=(_buf("linear", "in", True, 16), _buf("hist", "out", True, 4, _capi.METER_WORDS)),
        limits=dict(too_many_pixels=PIXELS),
        orders=(("ctx_null", "w_zero"), ("h_negative", "hist_null"), ("linear_null", "too_many_pixels"),
                ("too_many_pixels", "hist_misaligned"), ("hist_is_linear", "linear_misaligned"))),
    "display": dict(
        fn="rt_display", sizes=("w", "h"), args=("w", "h", "linear", "params", "rgba_out", "rgba8_out"),
        bufs=(_buf("linear", "in", True, 16), _buf("rgba_out", "out", False, 16), _buf("rgba8_out", "out", False, 4)),
        params=DisplayParams, bad=dict(exposure=INF, gamma=0.0, flip_y=7),
        pairs=dict(no_outputs=dict(rgba_out=None, rgba8_out=None), no_rgba_out=dict(rgba_out=None), no_rgba8_out=dict(rgba8_out=None)),
        limits=dict(too_many_pixels=PIXELS),
        orders=(("ctx_null", "w_zero"), ("linear_null", "too_many_pixels"), ("too_many_pixels", "no_outputs"),
                ("no_outputs", "params_gamma_bad"), ("rgba8_out_is_linear", "rgba8_out_is_rgba_out"),
                ("rgba8_out_into_rgba_out", "rgba_out_into_linear"), ("rgba_out_into_linear", "linear_misaligned"),
                ("rgba8_out_misaligned", "params_exposure_bad"), ("params_exposure_bad", "params_gamma_bad"))),
}


def violations(stage: str) -> dict:
    """{case name: (overrides, device form only)} of the stage, "valid" first, in the order of the module docstring.
    An override: a size, a scalar, None for a pointer, ("at", buffer, byte offset) for a buffer, a dict of fields
    for params, "bare" (the context without a camera) or None for ctx, "zero" for a singular prev_view."""
    S = STAGES[stage]
    v = {"valid": ({}, False), "ctx_null": (dict(ctx=None), False)}
    for s in S["sizes"]:
        v[f"{s}_zero"], v[f"{s}_negative"] = (({s: 0}, False), ({s: -1}, False))
    for b in S["bufs"]:
        if b["required"]:
            v[f"{b['name']}_null"] = ({b["name"]: None}, False)
    for name, o in {**S.get("pairs", {}), **S["limits"], **S.get("extras", {})}.items():
        v[name] = (o, False)
    ins = [b["name"] for b in S["bufs"] if not b["out"]]
    outs = [b["name"] for b in S["bufs"] if b["out"]]
    for k, o in enumerate(outs):
        for other in ins + outs[:k]:
            v[f"{o}_is_{other}"] = ({o: ("at", other, 0)}, False)
            v[f"{o}_into_{other}"] = ({o: ("at", other, 16)}, False)
    for b in S["bufs"] if S.get("misaligned", True) else ():
        v[f"{b['name']}_misaligned"] = ({b["name"]: ("at", b["name"], 4 if b["align"] == 16 else 1)}, True)
    if "params" in S:
        v["params_null"] = (dict(params=None), False)
        for f, bad in S["bad"].items():
            v[f"params_{f}_bad"] = (dict(params={f: bad}), False)
    for name, (_, bad) in S.get("scalars", {}).items():
        v[f"{name}_bad"] = ({name: bad}, False)
    for pair in S["orders"]:
        o, dev = {}, False
        for name in pair:
            for key, val in v[name][0].items():
                o[key] = {**o[key], **val} if key == "params" and isinstance(o.get(key), dict) else val
            dev = dev or v[name][1]
        v["+".join(pair)] = (o, dev)
    return v


def case_keys() -> list:
    """"stage/form/case" of every call, in the order they are made."""
    return [f"{stage}/{form}/{name}" for stage in STAGES for form in FORMS
            for name, (_, dev) in violations(stage).items() if form == "device" or not dev]


class Calls:
    """The hostsim library, a context with a camera, a bare one, and the arena."""

    def __init__(self):
        self.L = _capi.lib(True)
        self.ctx, self.bare = ctypes.c_void_p(), ctypes.c_void_p()
        for h in (self.ctx, self.bare):
            _capi.check(self.L, self.L.rt_create(0, ctypes.byref(h)), None, "rt_create")
        _capi.check(self.L, self.L.rt_set_camera(self.ctx, _capi.ptr(VIEW), FOV), self.ctx, "rt_set_camera")
        slots = max(len(S["bufs"]) for S in STAGES.values())
        self.arena = np.full((slots + 1) * SLOT // 4, 0.5, np.float32)
        self.base = (self.arena.ctypes.data + SLOT - 1) // SLOT * SLOT
        self.zero = np.zeros(16, np.float32)

    def close(self):
        for h in (self.ctx, self.bare):
            self.L.rt_destroy(h)

    def build_id(self) -> str:
        return self.L.rt_build_id().decode()

    def run(self, stage: str, form: str, overrides: dict):
        """(return code, rt_last_error text) of one call."""
        S = STAGES[stage]
        self.arena[:] = 0.5
        addr = {b["name"]: self.base + k * SLOT for k, b in enumerate(S["bufs"])}
        ctx = {"cam": self.ctx, "bare": self.bare, None: None}[overrides.get("ctx", "cam")]
        args = [ctx]
        for a in S["args"]:
            o = overrides.get(a, "keep")
            if a in S["sizes"]:
                args.append({"w": W, "h": H, "w_lo": W_LO, "h_lo": H_LO}[a] if o == "keep" else o)
            elif a in addr:
                args.append(addr[a] if o == "keep" else None if o is None else addr[o[1]] + o[2])
            elif a == "params":
                p = S["params"]()
                getattr(self.L, S["fn"].replace("_accumulate", "") + "_default_params")(ctypes.byref(p))
                for f, val in ({} if o in ("keep", None) else o).items():
                    setattr(p, f, val)
                args.append(None if o is None else ctypes.byref(p))
            elif a == "prev_view":
                args.append(_capi.ptr(VIEW) if o == "keep" else None if o is None else _capi.ptr(self.zero))
            else:
                args.append(S["scalars"][a][0] if o == "keep" else o)
        if form == "device":
            args.append(None)  # stream
        rc = getattr(self.L, S["fn"] + ("_device" if form == "device" else ""))(*args)
        return [int(rc), (self.L.rt_last_error(ctx) or b"").decode() if rc else ""]


def run_all() -> dict:
    """{key: [return code, text]} over case_keys()."""
    c = Calls()
    got = {}
    for stage in STAGES:
        for form in FORMS:
            for name, (o, dev) in violations(stage).items():
                if form == "device" or not dev:
                    got[f"{stage}/{form}/{name}"] = c.run(stage, form, o)
    c.close()
    return got
