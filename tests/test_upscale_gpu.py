"""The gfx950 kernels of the guided upscale stage (k_upscale_direct and k_upscale_lds, rt_upscale.hip) against the
hostsim build of the same code, bit for bit with NaN matching NaN on both outputs: the synthetic cases of
upscale_cases.py under both forced up_variant values and the product's dispatch, the device form on a stream of its
own, and the chain from a tracked progression at 32x32 to the displayed 64x64 frame."""
from __future__ import annotations

import numpy as np
import pytest

import meter_cases as mc
import noise_cases as nc
import rt_amd
import upscale_cases as uc
from upscale_cases import inputs, upscale
from stage_gpu import Stream, both_chains, forced_variant, post_chain

f32 = np.float32
# uc.PAIRS: (1,1)->(1,1) one live thread; (1,1)->(3,2) every tap but one outside the frame; (5,3)->(10,6) a ratio of 2
# with every footprint clipped; (37,29)->(130,67) and (65,17)->(130,67) three blocks across and 17 down, partial on
# both axes, footprints of 22 x 5 and 35 x 5 low pixels at uneven ratios; the identity's footprint is the widest, 67 x 7;
# (33,1)->(257,1) five blocks of one row at a ratio of 7.8.


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("sigma", [True, False])
@pytest.mark.parametrize("pair", uc.PAIRS)
def test_gpu_kernel_equals_hostsim(pair, sigma, variant):
    want = uc.host_result(pair, sigma)
    with forced_variant(uc.ctx, "up_variant", variant):
        got = upscale(inputs(*pair), None, sigma, hostsim=False)
    nc.assert_bits(got[0], want[0], f"{pair} sigma {sigma} variant {variant}: colour")
    if sigma:
        nc.assert_bits(got[1], want[1], f"{pair} sigma {sigma} variant {variant}: sigma_out")
    else:
        assert got[1] is None


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2])
def test_gpu_device_pointers_own_stream_into_garbage(variant):
    L, ctx = uc.ctx(False)
    st = Stream()
    try:
        with forced_variant(uc.ctx, "up_variant", variant):
            for pair in [(37, 29, 130, 67), (5, 3, 10, 6)]:  # larger, then smaller: the context's scratch is reused
                case = inputs(*pair)
                w_lo, h_lo, w, h = pair
                upscale(case, None, True, hostsim=False)  # (the host form: it sizes the staging buffer)
                want = uc.host_result(pair)
                d = {k: st.upload(v) for k, v in case.items()}
                d_out, d_sout = st.upload(np.full((h, w, 4), np.nan, f32)), st.upload(np.full((h, w), -7.0, f32))
                rt_amd.check(L, L.rt_upscale_device(ctx, w_lo, h_lo, w, h, d["rgba"].ptr, d["sigma"].ptr, d["alb_lo"].ptr,
                                                    d["nd_lo"].ptr, d["alb_hi"].ptr, d["nd_hi"].ptr, None, d_out.ptr, d_sout.ptr,
                                                    st.ptr), ctx, "rt_upscale_device")
                nc.assert_bits(st.download(d_out, (h, w, 4)), want[0], f"{pair}: colour")
                nc.assert_bits(st.download(d_sout, (h, w)), want[1], f"{pair}: sigma_out")
                for k, v in case.items():
                    nc.assert_bits(st.download(d[k], v.shape), v, f"{pair}: {k} changed")
            assert L.rt_last_kernel_ms(ctx) == -1.0, "the device form does not wait"
    finally:
        st.close()


LO, HI = 32, 64


def _upscale(C, frame):
    C.call("rt_render_features_device", HI, HI, C.f4("albedo_hi", HI, HI), C.f4("normal_depth_hi", HI, HI))
    C.call("rt_upscale_device", LO, LO, HI, HI, C.p(frame), C.p("sigma"), C.p("albedo"), C.p("normal_depth"), C.p("albedo_hi"),
           C.p("normal_depth_hi"), None, C.f4("upscaled", HI, HI), C.f1("upscaled sigma", HI, HI))
    return "upscaled"


def _chain(hostsim: bool, stream):
    """Cornell: a tracked [2, 2] progression at 32x32, the linear resolve, the noise figure, the guides at 32x32 and at
    64x64, the upscale, the histogram, the solve at the defaults and rt_display with that exposure, device forms on one
    stream; (linear, sigma, upscaled, upscaled sigma, histogram, 8-bit frame)."""
    got = post_chain(hostsim, stream, [_upscale], size=(LO, LO), sigma=True, features=True)
    return tuple(got[k] for k in ("linear", "sigma", "upscaled", "upscaled sigma", "histogram", "out8"))


@pytest.mark.gpu
def test_gpu_chain_to_the_displayed_frame_equals_hostsim():
    want, got = both_chains(_chain)
    for name, g, w in zip(("linear frame", "sigma", "upscaled", "upscaled sigma"), got, want):
        nc.assert_bits(g, w, f"chain: {name}")
    mc.assert_words(got[4], want[4], "chain: histogram")
    assert np.array_equal(got[5], want[5]), "chain: the 8-bit frame"
    assert want[5][..., :3].min() < 64 and want[5][..., :3].max() > 128, "the frame is neither black nor white"
