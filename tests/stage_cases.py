"""The host and the device form of each stage that has both (include/rt_hip.h): features, denoise,
display, query, progressive resolve, progress noise, denoise_var, temporal accumulation, firefly
rejection, metering, guided upscale. One call of each form on a Cornell context, a 16 x 12 frame
(the upscale: from 8 x 6) or 64 rays; a progression of two passes of one sample, so that both halves
of a tracked one hold a sample. Firefly takes a sigma and asks for all three outputs, temporal takes a
history and the upscale a sigma: every region of those stages' staging buffers is in use. Shared by tests/test_stage_call.py (hostsim: the two forms' outputs) and
tests/test_stage_call_gpu.py (gfx950: the outputs and the rt_last_kernel_ms convention, which the
backend keeps in one place, rt_backend_hip.h StagedCall).

Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import display_cases as dc
import dnv_cases as dnv
import firefly_cases as fc
import meter_cases as mc
import noise_cases as nc
import progress_cases as pc
import temporal_cases as tc
import upscale_cases as uc
from session_cases import _vp, assert_bits

from rt_amd import _capi

STAGES = ("features", "denoise", "display", "query", "resolve", "noise", "denoise_var", "temporal", "firefly", "meter",
          "upscale")
W, H, RAYS = 16, 12, 64
W_LO, H_LO = 8, 6


def _progression(s, tracked: bool):
    pc.begin(s, total=2, w=W, h=H)
    if tracked:
        nc.track(s)
    pc.advance(s, 1)
    pc.advance(s, 1)


def _both(s, fn: str, device: bool, *args) -> list:
    """fn(ctx, *args), or fn_device(ctx, *args, NULL stream), and its outputs. An array among args is an input and
    a (shape, dtype) pair an output, filled with fives first: host pointers, or device buffers (s.array) for the
    device form. Anything else is passed as it is."""
    outs, held, call = [], [], []
    for a in args:
        if isinstance(a, (tuple, np.ndarray)):
            is_out = isinstance(a, tuple)
            a = np.full(a[0], 5, a[1]) if is_out else np.ascontiguousarray(a)
            d = s.array(a) if device else a
            (outs if is_out else held).append(d)
            call.append(_vp(d.ptr) if device else _capi.ptr(a))
        else:
            call.append(a)
    name = fn + "_device" if device else fn
    s.ok(getattr(s.L, name)(s.ctx, *call, *([None] if device else [])), name)
    return [o.get() if device else o for o in outs]


def prepare(s, stage: str):
    """What both forms of the stage read: made once, before the first of them runs."""
    if stage == "denoise_var":
        return dnv.inputs(W, H)
    if stage == "temporal":
        case = tc.inputs("shift", W, H)
        s.set_camera(case["cur"].as17())
        return (case,)
    if stage == "firefly":
        return fc.inputs(W, H)
    if stage == "meter":
        return (mc.frame("noise", W, H),)
    if stage == "upscale":
        return (uc.inputs(W_LO, H_LO, W, H),)
    if stage == "denoise":
        alb, nd = s.features(W, H)
        return dc.shape_buffer(W, H), alb, nd
    if stage == "display":
        return (dc.shape_buffer(W, H),)
    if stage == "query":
        return (s.rays(RAYS),)
    if stage in ("resolve", "noise"):
        _progression(s, tracked=stage == "noise")
    return ()


def call(s, stage: str, device: bool, inputs) -> list:
    """The stage's outputs as a list of arrays, through its host or its device form."""
    if stage == "features":
        return list(s.features(W, H, device))
    if stage == "denoise":
        return [s.denoise(*inputs, 3, 0.75, device)]
    if stage == "display":
        return list(dc.display(s, inputs[0], device=device))
    if stage == "query":
        run = s.query_device if device else s.query
        return [run(inputs[0]), run(inputs[0], any_hit=True)]
    if stage == "resolve":
        return [pc.resolve(s, device), dc.resolve_linear(s, device)]
    frame, plane = ((H, W, 4), np.float32), ((H, W), np.float32)
    if stage == "denoise_var":
        rgba, sigma, alb, nd = inputs
        return _both(s, "rt_denoise_var", device, W, H, rgba, sigma, alb, nd, ctypes.byref(dnv.params(passes=3)),
                     ctypes.c_float(0.75), frame, plane)
    if stage == "temporal":
        c = inputs[0]
        view = np.ascontiguousarray(c["prev"].view_matrix, np.float32)  # (a host pointer in both forms)
        return _both(s, "rt_temporal_accumulate", device, W, H, c["rgba"], c["sigma"], c["nd"], _capi.ptr(view),
                     ctypes.c_float(c["prev"].fov_dist), *c["hist"], ctypes.byref(tc.params()), frame, plane, plane)
    if stage == "firefly":
        return _both(s, "rt_firefly", device, W, H, *inputs, ctypes.byref(fc.params()), frame, plane, plane)
    if stage == "meter":
        return _both(s, "rt_meter", device, W, H, inputs[0], ((mc.WORDS,), np.uint32))
    if stage == "upscale":
        c = inputs[0]
        return _both(s, "rt_upscale", device, W_LO, H_LO, W, H, c["rgba"], c["sigma"], c["alb_lo"], c["nd_lo"], c["alb_hi"],
                     c["nd_hi"], ctypes.byref(uc.params()), frame, plane)
    px, tl, st = nc.noise(s, device=device)
    words = [st[k] for k in nc.STAT_KEYS if k != "max_tile"]
    return [px, tl, np.asarray(words, np.int32), np.asarray([st["max_tile"]], np.float32)]


def case_forms(hostsim: bool, stage: str):
    """Both forms give the same words. gfx950 besides: the host form leaves rt_last_kernel_ms >= 0; the
    device form leaves it -1.0 until rt_device_last_kernel_ms is read after a synchronize (the download
    of the outputs waits for the device), and that read is >= 0 and is what rt_last_kernel_ms then says."""
    s = pc.session(hostsim, "cornell")
    inputs = prepare(s, stage)
    ms = lambda: float(s.L.rt_last_kernel_ms(s.ctx))  # noqa: E731
    host = call(s, stage, False, inputs)
    if not hostsim:
        assert ms() >= 0.0, s.where(f"{stage}: rt_last_kernel_ms after the host form is {ms()}")
    dev = call(s, stage, True, inputs)
    if not hostsim:
        assert ms() == -1.0, s.where(f"{stage}: rt_last_kernel_ms after the device form is {ms()}")
        read = float(s.L.rt_device_last_kernel_ms(s.ctx))
        assert read >= 0.0 and ms() == read, s.where(f"{stage}: rt_device_last_kernel_ms {read}, then {ms()}")
    assert len(host) == len(dev)
    for i, (a, b) in enumerate(zip(host, dev)):
        assert_bits(b, a, s.where(f"{stage}: output {i} of the device form vs the host form"))
    s.close()
