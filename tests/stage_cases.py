"""The host and the device form of each stage that has both (include/rt_hip.h): features, denoise,
display, query, progressive resolve, progress noise. One call of each form on a Cornell context, a
16 x 12 frame or 64 rays; a progression of two passes of one sample, so that both halves of a tracked
one hold a sample. Shared by tests/test_stage_call.py (hostsim: the two forms' outputs) and
tests/test_stage_call_gpu.py (gfx950: the outputs and the rt_last_kernel_ms convention, which the
backend keeps in one place, rt_backend_hip.h StagedCall).

Helpers only: no tests here."""
from __future__ import annotations

import numpy as np

import display_cases as dc
import noise_cases as nc
import progress_cases as pc
from session_cases import assert_bits

STAGES = ("features", "denoise", "display", "query", "resolve", "noise")
W, H, RAYS = 16, 12, 64


def _progression(s, tracked: bool):
    pc.begin(s, total=2, w=W, h=H)
    if tracked:
        nc.track(s)
    pc.advance(s, 1)
    pc.advance(s, 1)


def prepare(s, stage: str):
    """What both forms of the stage read: made once, before the first of them runs."""
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
