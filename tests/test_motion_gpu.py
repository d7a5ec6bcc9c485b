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
import rt_amd
import temporal_cases as tc
from motion_cases import blur, field, inputs, params
from stage_gpu import Stream, both_chains, forced_variant, post_chain

NAMES = ("rgba_out", "reach_out")
# mc.SHAPES: (1, 1) one live thread and an empty footprint; (5, 3) the streak longer than the image, negative offsets at
# every border; (37, 29) partial motion tiles on both axes; (130, 67) nine tiles across with a partial last tile; (70, 45)
# a full interior tile with all eight neighbours. mc.RADII: the footprint is at most 18 x 16, 24 x 16 and 48 x 16 entries
# along an axis, 40 x 38 near the diagonal.


def _gpu_blur(variant, *args):
    with forced_variant(mc.ctx, "motion_variant", variant):
        return blur(*args, hostsim=False)


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
    st = Stream()
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


def _vectors(C, frame):
    prev = tc.moved_camera(3, step=0.15)
    C.call("rt_motion_vectors_device", C.w, C.h, C.p("normal_depth"), rt_amd.ptr(prev.view_matrix), ctypes.c_float(prev.fov_dist),
           C.new("motion", (C.h, C.w, 2)))


def _lens(C, frame):
    dp = rt_amd.DofParams(rt_amd.focus_at(C.get("normal_depth"), C.w // 2, C.h // 2), 6.0, 8)
    C.call("rt_dof_device", C.w, C.h, C.p(frame), C.p("normal_depth"), ctypes.byref(dp), C.f4("lens"), None)
    return "lens"


def _shutter(C, frame):
    mp = rt_amd.MotionParams(1.0, 0.05, 8)
    C.call("rt_motion_blur_device", C.w, C.h, C.p(frame), C.p("normal_depth"), C.p("motion"), ctypes.byref(mp), C.f4("shutter"),
           C.f1("reach"))
    return "shutter"


def _chain(hostsim: bool, stream):
    """Cornell 40x30 under the Cornell camera, the previous frame's camera that preset moved three steps
    (temporal_cases.moved_camera): a tracked [2, 2] progression, the linear resolve, rt_render_features, rt_motion_vectors,
    rt_dof focused by rt_amd.focus_at at the centre pixel, rt_motion_blur, rt_bloom, the histogram of the bloomed frame,
    the solve at the defaults and rt_display with that exposure, device forms on one stream; every buffer on the way."""
    got = post_chain(hostsim, stream, [_vectors, _lens, _shutter], features=True, bloom=True)
    return tuple(got[k] for k in ("linear", "normal_depth", "motion", "lens", "shutter", "reach", "bloomed", "histogram", "exposure",
                                  "out8"))


@pytest.mark.gpu
def test_gpu_chain_with_the_motion_stages_equals_hostsim():
    want, got = both_chains(_chain)
    for i, name in ((0, "linear frame"), (1, "normal_depth"), (2, "motion vectors"), (3, "lens frame"), (4, "shutter frame"),
                    (5, "reach"), (6, "bloomed frame")):
        nc.assert_bits(got[i], want[i], "chain: " + name)
    mc_meter.assert_words(got[7], want[7], "chain: histogram")
    assert got[8] == want[8], "chain: exposure"
    assert np.array_equal(got[9], want[9]), "chain: the 8-bit frame"
    assert want[5].max() > 1.0, "something moved"
    assert not np.array_equal(want[4], want[3]), "the shutter changed the frame"
