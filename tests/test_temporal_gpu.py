"""The gfx950 kernel of temporal accumulation (k_temporal, rt_temporal.hip) against the hostsim build of the
same code, bit for bit with NaN matching NaN: the synthetic cases of temporal_cases.py under the four cameras,
with and without history; the device form on a stream of its own; the chain behind two tracked progressions
under a moved camera."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import noise_cases as nc
import progress_cases as pc
import rt_amd
import session_cases as sc
import temporal_cases as tc
from stage_gpu import Stream
from temporal_cases import accumulate, inputs, params

NAMES = ("colour", "sigma_out", "len_out")
# tc.SHAPES: (1, 1) one live thread; (5, 3) every tap clipped somewhere; (37, 29) partial blocks on both axes;
# (130, 67) more than two blocks across


@pytest.mark.gpu
@pytest.mark.parametrize("history", [True, False])
@pytest.mark.parametrize("kind", tc.CAMERAS)
@pytest.mark.parametrize("w,h", tc.SHAPES)
def test_gpu_kernel_equals_hostsim(w, h, kind, history):
    want = tc.host_result(kind, w, h, history)
    got = accumulate(inputs(kind, w, h), params(), hostsim=False, history=history)
    for g, x, name in zip(got, want, NAMES):
        nc.assert_bits(g, x, f"{w}x{h} {kind} history {history}: {name}")


@pytest.mark.gpu
def test_gpu_device_pointers_own_stream_and_scratch_reuse():
    st = Stream()
    try:
        for (w, h) in [(130, 67), (37, 29)]:  # larger, then smaller: the context's scratch is reused
            for kind in ("shift", "turn"):
                case = inputs(kind, w, h)
                L, ctx = tc.ctx(False, case["cur"])
                want = tc.host_result(kind, w, h)
                ins = [case["rgba"], case["sigma"], case["nd"], *case["hist"]]
                d = [st.upload(a) for a in ins]
                outs = [st.upload(np.zeros(s, np.float32)) for s in ((h, w, 4), (h, w), (h, w))]
                p = params()
                rt_amd.check(L, L.rt_temporal_accumulate_device(
                    ctx, w, h, d[0].ptr, d[1].ptr, d[2].ptr, rt_amd.ptr(case["prev"].view_matrix),
                    ctypes.c_float(case["prev"].fov_dist), d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, ctypes.byref(p),
                    outs[0].ptr, outs[1].ptr, outs[2].ptr, st.ptr), ctx, "rt_temporal_accumulate_device")
                for b, x, name in zip(outs, want, NAMES):
                    nc.assert_bits(st.download(b, x.shape), x, f"{w}x{h} {kind}: {name}")
                for b, a in zip(d, ins):
                    nc.assert_bits(st.download(b, a.shape), a, f"{w}x{h} {kind}: an input changed")
    finally:
        st.close()


def _chain(hostsim: bool, stream):
    """Cornell 40x30, two frames, the camera moved between them: per frame a tracked [2, 2] progression of a
    declared total of 6 + k, the linear resolve, the noise figure, the feature pass, temporal accumulation against
    the frame before and the variance-guided filter, device forms on one stream. Returns the second frame's
    (linear, accumulated, sigma, len, filtered)."""
    s = pc.session(hostsim, "cornell")
    W, H = pc.W, pc.H
    vp = ctypes.c_void_p
    q = vp(stream) if stream else None
    shapes = ((H, W, 4), (H, W), (H, W, 4), (H, W, 4), (H, W, 4), (H, W), (H, W), (H, W, 4), (H, W))
    prev = None
    for k in range(2):
        cam = sc.camera_of("cornell").copy()
        cam[3] += np.float32(0.05 * k)
        cam[7] += np.float32(0.02 * k)
        s.set_camera(cam)
        pc.begin(s, total=6 + k)
        nc.track(s)
        pc.advance(s, 2)
        pc.advance(s, 2)
        lin, sg, alb, nd, acc, acc_s, acc_l, out, left = [s.array(np.full(sh, -3.0, np.float32)) for sh in shapes]
        s.ok(s.L.rt_progress_resolve_linear_device(s.ctx, vp(lin.ptr), q), "rt_progress_resolve_linear_device")
        s.ok(s.L.rt_progress_noise_sigma_device(s.ctx, vp(sg.ptr), q), "rt_progress_noise_sigma_device")
        s.ok(s.L.rt_render_features_device(s.ctx, W, H, vp(alb.ptr), vp(nd.ptr), q), "rt_render_features_device")
        hist = [None] * 4 if prev is None else [vp(b.ptr) for b in prev[1]]
        view = np.ascontiguousarray((cam if prev is None else prev[0])[:16])
        s.ok(s.L.rt_temporal_accumulate_device(s.ctx, W, H, vp(lin.ptr), vp(sg.ptr), vp(nd.ptr), rt_amd.ptr(view),
                                               ctypes.c_float(float(cam[16])), *hist, None, vp(acc.ptr), vp(acc_s.ptr),
                                               vp(acc_l.ptr), q), "rt_temporal_accumulate_device")
        s.ok(s.L.rt_denoise_var_device(s.ctx, W, H, vp(acc.ptr), vp(acc_s.ptr), vp(alb.ptr), vp(nd.ptr), None,
                                       ctypes.c_float(1.0), vp(out.ptr), vp(left.ptr), q), "rt_denoise_var_device")
        got = tuple(b.get() for b in (lin, acc, acc_s, acc_l, out))  # (the download waits for the device)
        prev = (cam, (acc, acc_s, acc_l, nd))
    s.close()
    return got


@pytest.mark.gpu
def test_gpu_two_frame_chain_equals_hostsim():
    want = _chain(True, None)
    st = Stream()
    try:
        got = _chain(False, st.ptr)
    finally:
        st.close()
    assert (want[3] == 2.0).any(), "the second frame found history"
    for name, g, w in zip(("linear frame", "accumulated", "sigma", "len", "filtered"), got, want):
        nc.assert_bits(g, w, f"chain: {name}")
    assert (got[1][..., :3] != got[0][..., :3]).any(), "the second frame's output differs from its input"
