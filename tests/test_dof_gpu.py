"""The gfx950 kernels of the depth-of-field stage (k_dof_lds and k_dof_direct, rt_dof.hip) against the hostsim build of
the same code, bit for bit with NaN matching NaN on both outputs: the synthetic cases of dof_cases.py under both forced
dof_variant values and the product's dispatch, the case whose in-focus tile is reached by its neighbours' blur, the
device form on a stream of its own, and the chain from a tracked progression to the displayed frame."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import dof_cases as dc
import meter_cases as mc
import noise_cases as nc
import rt_amd
from dof_cases import dof, inputs, params
from stage_gpu import Stream, both_chains, forced_variant, post_chain

NAMES = ("rgba_out", "coc_out")
# dc.SHAPES: (1, 1) one live thread, every other entry of the footprint outside the image; (5, 3) the window larger than
# the image; (37, 29) two 32 x 16 tiles each way, partial on both axes; (130, 67) five tiles across, partial 64 x 4 blocks
# of the direct kernel; (70, 45) three tiles each way. dc.RADII: the footprint is 34 x 18, 40 x 24 and 56 x 40 entries.


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("max_radius", dc.RADII)
@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_gpu_kernels_equal_hostsim(w, h, max_radius, variant):
    want = dc.host_result(w, h, max_radius)
    with forced_variant(dc.ctx, "dof_variant", variant):
        got = dof(*inputs(w, h), params(max_radius=max_radius), hostsim=False)
    for g, x, name in zip(got, want, NAMES):
        nc.assert_bits(g, x, f"{w}x{h} max_radius {max_radius} variant {variant}: {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_gpu_blur_reaches_into_a_tile_that_is_in_focus(variant):
    """A window bound taken from the tile's own pixels (r = 0: one tap) would return the tile's input."""
    rgba, nd, p = dc.tile_case()
    want = dof(rgba, nd, p)
    assert np.all(want[1][16:32, 32:64] == 0.0) and np.all(want[1][:16] == 12.0)
    inner = want[0][16:32, 32:64, :3]
    assert not np.array_equal(inner, rgba[16:32, 32:64, :3]), "the blur reaches into the in-focus tile"
    with forced_variant(dc.ctx, "dof_variant", variant):
        got = dof(rgba, nd, p, hostsim=False)
    for g, x, name in zip(got, want, NAMES):
        nc.assert_bits(g, x, f"in-focus tile, variant {variant}: {name}")


@pytest.mark.gpu
def test_gpu_device_pointers_own_stream():
    L, ctx = dc.ctx(False)
    st = Stream()
    try:
        for (w, h) in [(130, 67), (37, 29)]:  # larger, then smaller
            rgba, nd = inputs(w, h)
            d_in, d_nd = st.upload(rgba), st.upload(nd)
            for R in (12, 4):
                want = dc.host_result(w, h, R)
                d_out, d_coc = st.upload(np.zeros((h, w, 4), np.float32)), st.upload(np.zeros((h, w), np.float32))
                p = params(max_radius=R)
                rt_amd.check(L, L.rt_dof_device(ctx, w, h, d_in.ptr, d_nd.ptr, ctypes.byref(p), d_out.ptr, d_coc.ptr, st.ptr), ctx,
                             "rt_dof_device")
                for b, x, name in zip((d_out, d_coc), want, NAMES):
                    nc.assert_bits(st.download(b, x.shape), x, f"{w}x{h} max_radius {R}: {name}")
            # without the radius
            out = st.upload(np.zeros((h, w, 4), np.float32))
            rt_amd.check(L, L.rt_dof_device(ctx, w, h, d_in.ptr, d_nd.ptr, ctypes.byref(p), out.ptr, None, st.ptr), ctx, "rt_dof_device")
            nc.assert_bits(st.download(out, rgba.shape), dc.host_result(w, h, 4)[0], f"{w}x{h}: coc_out NULL")
            nc.assert_bits(st.download(d_in, rgba.shape), rgba, f"{w}x{h}: the input changed")
            nc.assert_bits(st.download(d_nd, nd.shape), nd, f"{w}x{h}: the guide changed")
    finally:
        st.close()


def _lens(C, frame):
    C.values["focus"] = rt_amd.focus_at(C.get("normal_depth"), C.w // 2, C.h // 2)
    p = rt_amd.DofParams(C.values["focus"], 6.0, 8)
    C.call("rt_dof_device", C.w, C.h, C.p(frame), C.p("normal_depth"), ctypes.byref(p), C.f4("blurred"), C.f1("coc"))
    return "blurred"


def _chain(hostsim: bool, stream):
    """Cornell 40x30: a tracked [2, 2] progression, the linear resolve, rt_render_features, rt_dof focused by
    rt_amd.focus_at at the centre pixel, rt_bloom, the histogram of the bloomed frame, the solve at the defaults and
    rt_display with that exposure, device forms on one stream; every buffer on the way."""
    got = post_chain(hostsim, stream, [_lens], features=True, bloom=True)
    return tuple(got[k] for k in ("linear", "normal_depth", "focus", "blurred", "coc", "bloomed", "layer", "histogram", "exposure",
                                  "out8"))


@pytest.mark.gpu
def test_gpu_chain_with_the_dof_stage_equals_hostsim():
    want, got = both_chains(_chain)
    nc.assert_bits(got[0], want[0], "chain: linear frame")
    nc.assert_bits(got[1], want[1], "chain: normal_depth")
    assert got[2] == want[2], "chain: the focus"
    nc.assert_bits(got[3], want[3], "chain: blurred frame")
    nc.assert_bits(got[4], want[4], "chain: radius")
    nc.assert_bits(got[5], want[5], "chain: bloomed frame")
    nc.assert_bits(got[6], want[6], "chain: layer")
    mc.assert_words(got[7], want[7], "chain: histogram")
    assert got[8] == want[8], "chain: exposure"
    assert np.array_equal(got[9], want[9]), "chain: the 8-bit frame"
    assert want[4][want[4].shape[0] // 2, want[4].shape[1] // 2] == 0.0 and want[4].max() > 1.0, "the centre is in focus, something is not"
    assert not np.array_equal(want[3], want[0]), "the lens changed the frame"
