"""The gfx950 kernels of the firefly rejection stage (k_firefly_lds and k_firefly_direct, rt_firefly.hip) against the
hostsim build of the same code, bit for bit with NaN matching NaN on all three outputs: the synthetic cases of
firefly_cases.py under both forced ff_variant values and the product's dispatch, the device form on a stream of its
own, and the chain behind a tracked progression."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import firefly_cases as fc
import noise_cases as nc
import rt_amd
import session_cases as sc
from firefly_cases import clamp, inputs, params
from stage_gpu import Stream, both_chains, forced_variant, post_chain

NAMES = ("colour", "sigma_out", "scale_out")
GAIN, FLOOR = 1.0, 0.01  # (gain 1 clamps a third of the noisy frame: the scaling path runs in every wave)
# fc.SHAPES: (1, 1) one live thread, no neighbour; (5, 3) every neighbourhood clipped; (37, 29) partial blocks on both
# axes; (130, 67) more than two blocks across. At radius 2 the 288 halo entries take the fill loop's second round.


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("rank", [1, 2, 8])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_gpu_kernel_equals_hostsim(w, h, radius, rank, variant):
    want = fc.host_result(w, h, radius, rank, GAIN, FLOOR)
    with forced_variant(fc.ctx, "ff_variant", variant):
        got = clamp(*inputs(w, h), params(radius, rank, GAIN, FLOOR), hostsim=False)
    for g, x, name in zip(got, want, NAMES):
        nc.assert_bits(g, x, f"{w}x{h} radius {radius} rank {rank} variant {variant}: {name}")


@pytest.mark.gpu
def test_gpu_device_pointers_own_stream_and_scratch_reuse():
    L, ctx = fc.ctx(False)
    st = Stream()
    try:
        for (w, h) in [(130, 67), (37, 29)]:  # larger, then smaller: the context's scratch is reused
            rgba, sigma = inputs(w, h)
            clamp(rgba, sigma, params(2, 2, GAIN, FLOOR), hostsim=False)  # (the host form: it sizes the staging buffer)
            for radius in (1, 2):
                want = fc.host_result(w, h, radius, 2, GAIN, FLOOR)
                d_in, d_sg = st.upload(rgba), st.upload(sigma)
                outs = [st.upload(np.zeros(s, np.float32)) for s in ((h, w, 4), (h, w), (h, w))]
                p = params(radius, 2, GAIN, FLOOR)
                rt_amd.check(L, L.rt_firefly_device(ctx, w, h, d_in.ptr, d_sg.ptr, ctypes.byref(p), outs[0].ptr, outs[1].ptr,
                                                    outs[2].ptr, st.ptr), ctx, "rt_firefly_device")
                for b, x, name in zip(outs, want, NAMES):
                    nc.assert_bits(st.download(b, x.shape), x, f"{w}x{h} radius {radius}: {name}")
                nc.assert_bits(st.download(d_in, rgba.shape), rgba, f"{w}x{h}: rgba_in changed")
                nc.assert_bits(st.download(d_sg, sigma.shape), sigma, f"{w}x{h}: sigma_in changed")
    finally:
        st.close()


def _clamp(C, frame):
    C.call("rt_firefly_device", C.w, C.h, C.p(frame), C.p("sigma"), None, C.f4("clamped"), C.f1("clamped sigma"), C.f1("scale"))
    return "clamped"


def _features(C, frame):
    C.call("rt_render_features_device", C.w, C.h, C.f4("albedo"), C.f4("normal_depth"))


def _accumulate(C, frame):
    cam = sc.camera_of("cornell")  # (the session's camera: with no history only its validity counts)
    view = np.ascontiguousarray(cam[:16])
    C.call("rt_temporal_accumulate_device", C.w, C.h, C.p(frame), C.p("clamped sigma"), C.p("normal_depth"), rt_amd.ptr(view),
           ctypes.c_float(float(cam[16])), None, None, None, None, None, C.f4("accumulated"), C.f1("accumulated sigma"),
           C.f1("length"))
    return "accumulated"


def _filter(C, frame):
    C.call("rt_denoise_var_device", C.w, C.h, C.p(frame), C.p("accumulated sigma"), C.p("albedo"), C.p("normal_depth"), None,
           ctypes.c_float(1.0), C.f4("filtered"), C.f1("sigma_out"))


def _chain(hostsim: bool, stream):
    """Cornell 40x30: a tracked [2, 2] progression, then the linear resolve, the noise figure, the firefly stage at its
    defaults, the feature pass, temporal accumulation without a history and the variance-guided filter, device forms
    on one stream; (linear, sigma, clamped, clamped sigma, scale, accumulated, filtered)."""
    got = post_chain(hostsim, stream, [_clamp, _features, _accumulate, _filter], sigma=True, display=False)
    return tuple(got[k] for k in ("linear", "sigma", "clamped", "clamped sigma", "scale", "accumulated", "filtered"))


@pytest.mark.gpu
def test_gpu_chain_with_the_firefly_stage_equals_hostsim():
    want, got = both_chains(_chain)
    assert (want[4] < 1).any() and (want[4] == 1).any(), "the frame has clamped and untouched pixels"
    for name, g, w in zip(("linear frame", "sigma", "clamped", "clamped sigma", "scale", "accumulated", "filtered"), got, want):
        nc.assert_bits(g, w, f"chain: {name}")
