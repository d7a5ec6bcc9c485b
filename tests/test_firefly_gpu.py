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
import progress_cases as pc
import rt_amd
import session_cases as sc
from firefly_cases import clamp, inputs, params
from test_dnv_gpu import _Stream

NAMES = ("colour", "sigma_out", "scale_out")
GAIN, FLOOR = 1.0, 0.01  # (gain 1 clamps a third of the noisy frame: the scaling path runs in every wave)
# fc.SHAPES: (1, 1) one live thread, no neighbour; (5, 3) every neighbourhood clipped; (37, 29) partial blocks on both
# axes; (130, 67) more than two blocks across. At radius 2 the 288 halo entries take the fill loop's second round.


def _gpu_variant(v):
    L, h = fc.ctx(False)
    rt_amd.check(L, L.rt_test_schedule(h, b"ff_variant", float(v)), h, "rt_test_schedule")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("rank", [1, 2, 8])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_gpu_kernel_equals_hostsim(w, h, radius, rank, variant):
    want = fc.host_result(w, h, radius, rank, GAIN, FLOOR)
    _gpu_variant(variant)
    try:
        got = clamp(*inputs(w, h), params(radius, rank, GAIN, FLOOR), hostsim=False)
    finally:
        _gpu_variant(0)
    for g, x, name in zip(got, want, NAMES):
        nc.assert_bits(g, x, f"{w}x{h} radius {radius} rank {rank} variant {variant}: {name}")


@pytest.mark.gpu
def test_gpu_device_pointers_own_stream_and_scratch_reuse():
    L, ctx = fc.ctx(False)
    st = _Stream()
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


def _chain(hostsim: bool, stream):
    """Cornell 40x30: a tracked [2, 2] progression, then the linear resolve, the noise figure, the firefly stage at its
    defaults, the feature pass, temporal accumulation without a history and the variance-guided filter, device forms
    on one stream; (linear, sigma, clamped, clamped sigma, scale, accumulated, filtered)."""
    s = pc.session(hostsim, "cornell")
    pc.begin(s, total=4)
    nc.track(s)
    pc.advance(s, 2)
    pc.advance(s, 2)
    W, H = pc.W, pc.H
    vp = ctypes.c_void_p
    q = vp(stream) if stream else None
    c4, c1 = (H, W, 4), (H, W)
    bufs = [s.array(np.full(shape, -3.0, np.float32)) for shape in (c4, c1, c4, c1, c1, c4, c4, c4, c1, c1, c4, c1)]
    lin, sg, ff, ff_s, ff_f, alb, nd, acc, acc_s, acc_l, out, left = bufs
    s.ok(s.L.rt_progress_resolve_linear_device(s.ctx, vp(lin.ptr), q), "rt_progress_resolve_linear_device")
    s.ok(s.L.rt_progress_noise_sigma_device(s.ctx, vp(sg.ptr), q), "rt_progress_noise_sigma_device")
    s.ok(s.L.rt_firefly_device(s.ctx, W, H, vp(lin.ptr), vp(sg.ptr), None, vp(ff.ptr), vp(ff_s.ptr), vp(ff_f.ptr), q),
         "rt_firefly_device")
    s.ok(s.L.rt_render_features_device(s.ctx, W, H, vp(alb.ptr), vp(nd.ptr), q), "rt_render_features_device")
    cam = sc.camera_of("cornell")  # (the session's camera: with no history only its validity counts)
    view = np.ascontiguousarray(cam[:16])
    s.ok(s.L.rt_temporal_accumulate_device(s.ctx, W, H, vp(ff.ptr), vp(ff_s.ptr), vp(nd.ptr), rt_amd.ptr(view),
                                           ctypes.c_float(float(cam[16])), None, None, None, None, None, vp(acc.ptr),
                                           vp(acc_s.ptr), vp(acc_l.ptr), q), "rt_temporal_accumulate_device")
    s.ok(s.L.rt_denoise_var_device(s.ctx, W, H, vp(acc.ptr), vp(acc_s.ptr), vp(alb.ptr), vp(nd.ptr), None, ctypes.c_float(1.0),
                                   vp(out.ptr), vp(left.ptr), q), "rt_denoise_var_device")
    got = tuple(b.get() for b in (lin, sg, ff, ff_s, ff_f, acc, out))  # (the download waits for the device)
    s.close()
    return got


@pytest.mark.gpu
def test_gpu_chain_with_the_firefly_stage_equals_hostsim():
    want = _chain(True, None)
    st = _Stream()
    try:
        got = _chain(False, st.ptr)
    finally:
        st.close()
    assert (want[4] < 1).any() and (want[4] == 1).any(), "the frame has clamped and untouched pixels"
    for name, g, w in zip(("linear frame", "sigma", "clamped", "clamped sigma", "scale", "accumulated", "filtered"), got, want):
        nc.assert_bits(g, w, f"chain: {name}")
