"""The gfx950 kernels of the motion stages (k_motion_vectors, k_motion_tilemax, k_mblur_lds and k_mblur_direct,
rt_motion.hip) against the hostsim build of the same code, bit for bit with NaN matching NaN on every output: the
synthetic cases of motion_cases.py under both forced motion_variant values and the product's dispatch, the tie within a
tile and the still tile beside a moving one (the tile records' effect), the vectors of temporal_cases.py's cameras, the
device forms on a stream of their own, and the chain from a tracked progression to the displayed frame."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import meter_cases as mc_meter
import motion_cases as mc
import noise_cases as nc
import progress_cases as pc
import rt_amd
import temporal_cases as tc
from motion_cases import blur, field, inputs, params
from test_dnv_gpu import _Stream

NAMES = ("rgba_out", "reach_out")
# mc.SHAPES: (1, 1) one live thread and an empty footprint; (5, 3) the streak longer than the image, negative offsets at
# every border; (37, 29) partial motion tiles on both axes; (130, 67) nine tiles across with a partial last tile; (70, 45)
# a full interior tile with all eight neighbours. mc.RADII: the footprint is at most 18 x 16, 24 x 16 and 48 x 16 entries
# along an axis, 40 x 38 near the diagonal.


def _gpu_variant(v):
    L, h = mc.ctx(False)
    rt_amd.check(L, L.rt_test_schedule(h, b"motion_variant", float(v)), h, "rt_test_schedule")


def _gpu_blur(variant, *args):
    _gpu_variant(variant)
    try:
        return blur(*args, hostsim=False)
    finally:
        _gpu_variant(0)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("kind", mc.FIELDS)
@pytest.mark.parametrize("max_radius", mc.RADII)
@pytest.mark.parametrize("w,h", mc.SHAPES)
def test_gpu_kernels_equal_hostsim(w, h, max_radius, kind, variant):
    want = mc.host_result(w, h, max_radius, kind)
    got = _gpu_blur(variant, *inputs(w, h), field(kind, w, h, max_radius), params(max_radius=max_radius))
    for g, x, name in zip(got, want, NAMES):
        nc.assert_bits(g, x, f"{w}x{h} max_radius {max_radius} {kind} variant {variant}: {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("case", ["tie_case", "border_case"])
def test_gpu_tile_records_equal_hostsim(case, variant):
    """The first of two equal reaches sets the line; a still tile takes its moving neighbour's line."""
    args = getattr(mc, case)()
    want = blur(*args)
    assert not np.array_equal(want[0], args[0]), "the case blurs something"
    got = _gpu_blur(variant, *args)
    for g, x, name in zip(got, want, NAMES):
        nc.assert_bits(g, x, f"{case}, variant {variant}: {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", tc.CAMERAS)
@pytest.mark.parametrize("w,h", tc.SHAPES)
def test_gpu_vectors_equal_hostsim(w, h, kind):
    cur, prev = tc.cameras(kind, w, h)
    nd = tc.normal_depth(cur, w, h)
    if w * h > 4:
        nd.reshape(-1, 4)[2 * w * h // 3, 1] = np.nan
    nc.assert_bits(mc.vectors(cur, prev, nd, hostsim=False), mc.vectors(cur, prev, nd), f"{kind} {w}x{h}: the vectors")


@pytest.mark.gpu
def test_gpu_device_pointers_own_stream():
    cur, prev = tc.cameras("turn", 130, 67)
    L, ctx = tc.ctx(False, cur)
    st = _Stream()
    try:
        for (w, h) in [(130, 67), (37, 29)]:  # larger, then smaller
            rgba, nd = inputs(w, h)
            d_in, d_nd = st.upload(rgba), st.upload(nd)
            for R in (16, 4):
                m = field("random", w, h, R)
                want = mc.host_result(w, h, R, "random")
                d_m = st.upload(m)
                d_out, d_reach = st.upload(np.zeros((h, w, 4), np.float32)), st.upload(np.zeros((h, w), np.float32))
                p = params(max_radius=R)
                rt_amd.check(L, L.rt_motion_blur_device(ctx, w, h, d_in.ptr, d_nd.ptr, d_m.ptr, ctypes.byref(p), d_out.ptr, d_reach.ptr,
                                                        st.ptr), ctx, "rt_motion_blur_device")
                for b, x, name in zip((d_out, d_reach), want, NAMES):
                    nc.assert_bits(st.download(b, x.shape), x, f"{w}x{h} max_radius {R}: {name}")
                nc.assert_bits(st.download(d_m, m.shape), m, f"{w}x{h}: the motion changed")
            # without the reach
            out = st.upload(np.zeros((h, w, 4), np.float32))
            rt_amd.check(L, L.rt_motion_blur_device(ctx, w, h, d_in.ptr, d_nd.ptr, d_m.ptr, ctypes.byref(p), out.ptr, None, st.ptr), ctx,
                         "rt_motion_blur_device")
            nc.assert_bits(st.download(out, rgba.shape), mc.host_result(w, h, 4, "random")[0], f"{w}x{h}: reach_out NULL")
            nc.assert_bits(st.download(d_in, rgba.shape), rgba, f"{w}x{h}: the input changed")
            nc.assert_bits(st.download(d_nd, nd.shape), nd, f"{w}x{h}: the guide changed")
            # the vectors
            cur, prev = tc.cameras("turn", w, h)
            tc.ctx(False, cur)
            guide = tc.normal_depth(cur, w, h)
            d_g, d_v = st.upload(guide), st.upload(np.zeros((h, w, 2), np.float32))
            rt_amd.check(L, L.rt_motion_vectors_device(ctx, w, h, d_g.ptr, rt_amd.ptr(prev.view_matrix), ctypes.c_float(prev.fov_dist),
                                                       d_v.ptr, st.ptr), ctx, "rt_motion_vectors_device")
            nc.assert_bits(st.download(d_v, (h, w, 2)), mc.vectors(cur, prev, guide), f"{w}x{h}: the vectors")
            nc.assert_bits(st.download(d_g, guide.shape), guide, f"{w}x{h}: the vectors' guide changed")
    finally:
        st.close()


def _chain(hostsim: bool, stream):
    """Cornell 40x30 under the Cornell camera, the previous frame's camera that preset moved three steps
    (temporal_cases.moved_camera): a tracked [2, 2] progression, the linear resolve, rt_render_features, rt_motion_vectors,
    rt_dof focused by rt_amd.focus_at at the centre pixel, rt_motion_blur, rt_bloom, the histogram of the bloomed frame,
    the solve at the defaults and rt_display with that exposure, device forms on one stream; every buffer on the way."""
    s = pc.session(hostsim, "cornell")
    pc.begin(s, total=4)
    nc.track(s)
    pc.advance(s, 2)
    pc.advance(s, 2)
    W, H = pc.W, pc.H
    vp = ctypes.c_void_p
    q = vp(stream) if stream else None
    prev = tc.moved_camera(3, step=0.15)
    lin, alb, nd, lens, shut, out, layer = (s.array(np.full((H, W, 4), -3.0, np.float32)) for _ in range(7))
    mv = s.array(np.full((H, W, 2), -3.0, np.float32))
    reach = s.array(np.full((H, W), -3.0, np.float32))
    hist = s.array(np.full(mc_meter.WORDS, 0xDEADBEEF, np.uint32))
    out8 = s.array(np.zeros((H, W, 4), np.uint8))
    s.ok(s.L.rt_progress_resolve_linear_device(s.ctx, vp(lin.ptr), q), "rt_progress_resolve_linear_device")
    s.ok(s.L.rt_render_features_device(s.ctx, W, H, vp(alb.ptr), vp(nd.ptr), q), "rt_render_features_device")
    s.ok(s.L.rt_motion_vectors_device(s.ctx, W, H, vp(nd.ptr), rt_amd.ptr(prev.view_matrix), ctypes.c_float(prev.fov_dist), vp(mv.ptr),
                                      q), "rt_motion_vectors_device")
    guide = nd.get()  # (the download waits for the device)
    dp = rt_amd.DofParams(rt_amd.focus_at(guide, W // 2, H // 2), 6.0, 8)
    s.ok(s.L.rt_dof_device(s.ctx, W, H, vp(lin.ptr), vp(nd.ptr), ctypes.byref(dp), vp(lens.ptr), None, q), "rt_dof_device")
    mp = rt_amd.MotionParams(1.0, 0.05, 8)
    s.ok(s.L.rt_motion_blur_device(s.ctx, W, H, vp(lens.ptr), vp(nd.ptr), vp(mv.ptr), ctypes.byref(mp), vp(shut.ptr), vp(reach.ptr), q),
         "rt_motion_blur_device")
    s.ok(s.L.rt_bloom_device(s.ctx, W, H, vp(shut.ptr), None, vp(out.ptr), vp(layer.ptr), q), "rt_bloom_device")
    s.ok(s.L.rt_meter_device(s.ctx, W, H, vp(out.ptr), vp(hist.ptr), q), "rt_meter_device")
    words = hist.get()
    r = rt_amd.meter_solve(words, hostsim=hostsim)
    d = rt_amd.DisplayParams(r["exposure"], 2.2, 0)
    s.ok(s.L.rt_display_device(s.ctx, W, H, vp(out.ptr), ctypes.byref(d), None, vp(out8.ptr), q), "rt_display_device")
    got = (lin.get(), guide, mv.get(), lens.get(), shut.get(), reach.get(), out.get(), words, r["exposure"], out8.get())
    s.close()
    return got


@pytest.mark.gpu
def test_gpu_chain_with_the_motion_stages_equals_hostsim():
    want = _chain(True, None)
    st = _Stream()
    try:
        got = _chain(False, st.ptr)
    finally:
        st.close()
    for i, name in ((0, "linear frame"), (1, "normal_depth"), (2, "motion vectors"), (3, "lens frame"), (4, "shutter frame"),
                    (5, "reach"), (6, "bloomed frame")):
        nc.assert_bits(got[i], want[i], "chain: " + name)
    mc_meter.assert_words(got[7], want[7], "chain: histogram")
    assert got[8] == want[8], "chain: exposure"
    assert np.array_equal(got[9], want[9]), "chain: the 8-bit frame"
    assert want[5].max() > 1.0, "something moved"
    assert not np.array_equal(want[4], want[3]), "the shutter changed the frame"
