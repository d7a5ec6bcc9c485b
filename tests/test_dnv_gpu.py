"""The gfx950 kernels of the variance-guided filter and of the absolute noise figure (rt_dnv.hip) against
the hostsim build of the same code, bit for bit with NaN matching NaN: k_dnv_direct and every k_dnv_lds
instantiation under both forced dn_variant values and the product's dispatch, the device forms on a stream
of their own, the chain behind a tracked progression, and an adaptive state with unequal tile counts."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import dnv_cases as dv
import noise_cases as nc
import rt_amd
from dnv_cases import denoise_var, inputs, params
from stage_gpu import Stream, both_chains, forced_variant, post_chain

# (w, h, passes): one live thread; every tap row, column and the 3x3 clipped; partial tiles on both axes at steps
# 1, 2 and 4 (every k_dnv_lds instantiation under dn_variant 2, the 32x8 one included); more than two tiles across
# and steps 8 and 16 on the direct kernel. Every shape carries sigma_map()'s NaN and +inf entries.
SHAPES = [(1, 1, 3), (5, 3, 3), (37, 29, 3), (130, 67, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("guides", [True, False])
@pytest.mark.parametrize("w,h,passes", SHAPES)
def test_gpu_filter_equals_hostsim(w, h, passes, guides, variant):
    rgba, sigma, alb, nd = inputs(w, h)
    want = dv.host_result(w, h, passes, guides, 0.75)
    with forced_variant(dv.ctx, "dn_variant", variant):
        got = denoise_var(rgba, sigma, alb if guides else None, nd if guides else None, params(passes), 0.75, hostsim=False)
    nc.assert_bits(got[0], want[0], f"{w}x{h} passes {passes} guides {guides} variant {variant}: colour")
    nc.assert_bits(got[1], want[1], f"{w}x{h} passes {passes} guides {guides} variant {variant}: sigma_out")


@pytest.mark.gpu
def test_gpu_device_pointers_own_stream_and_scratch_reuse():
    L, h = dv.ctx(False)
    st = Stream()
    try:
        for (w, hh) in [(130, 67), (37, 29)]:  # larger, then smaller: the context's scratch is reused
            rgba, sigma, alb, nd = inputs(w, hh)
            want = dv.host_result(w, hh, 4, True, 0.75)
            d_in, d_sg, d_alb, d_nd = (st.upload(a) for a in (rgba, sigma, alb, nd))
            d_out, d_left = st.upload(np.zeros_like(rgba)), st.upload(np.zeros_like(sigma))
            p = params(4)
            rt_amd.check(L, L.rt_denoise_var_device(h, w, hh, d_in.ptr, d_sg.ptr, d_alb.ptr, d_nd.ptr, ctypes.byref(p),
                                                    ctypes.c_float(0.75), d_out.ptr, d_left.ptr, st.ptr), h,
                         "rt_denoise_var_device")
            nc.assert_bits(st.download(d_out, rgba.shape), want[0], f"{w}x{hh}: colour")
            nc.assert_bits(st.download(d_left, sigma.shape), want[1], f"{w}x{hh}: sigma_out")
            nc.assert_bits(st.download(d_in, rgba.shape), rgba, f"{w}x{hh}: the input is untouched")
    finally:
        st.close()


def _filter(C, frame):
    C.call("rt_denoise_var_device", C.w, C.h, C.p(frame), C.p("sigma"), C.p("albedo"), C.p("normal_depth"), None, ctypes.c_float(1.0),
           C.f4("filtered"), C.f1("sigma_out"))


def _chain(hostsim: bool, stream):
    """Cornell 40x30: a tracked [2, 2] progression, then the linear resolve, the noise figure, the feature pass
    and the filter, device forms on one stream; (linear, sigma, rgba_out, sigma_out)."""
    got = post_chain(hostsim, stream, [_filter], sigma=True, features=True, display=False)
    return tuple(got[k] for k in ("linear", "sigma", "filtered", "sigma_out"))


@pytest.mark.gpu
def test_gpu_progression_sigma_features_filter_chain_equals_hostsim():
    want, got = both_chains(_chain)
    assert np.isfinite(want[1]).all() and (want[1] > 0).any()
    for name, g, w in zip(("linear frame", "sigma", "filtered", "sigma_out"), got, want):
        nc.assert_bits(g, w, f"chain: {name}")
    assert (got[2][..., :3] != got[0][..., :3]).any(), "the filter changed the frame"


@pytest.mark.gpu
def test_gpu_noise_sigma_with_unequal_tile_counts_equals_hostsim():
    want = dv.case_sigma_uneven(True)
    dv.case_sigma_uneven(False, want=want)
