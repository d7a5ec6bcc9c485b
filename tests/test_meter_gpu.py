"""The gfx950 kernels of the metering stage (k_meter_lds and k_meter_direct, rt_meter.hip) against the hostsim build
of the same code, word for word: the synthetic frames of meter_cases.py under both forced mt_variant values and the
product's dispatch, forced block counts, the device form on a stream of its own, and the chain behind a tracked
progression up to the displayed 8-bit frame."""
from __future__ import annotations

import numpy as np
import pytest

import meter_cases as mc
import noise_cases as nc
import rt_amd
from meter_cases import frame, meter
from stage_gpu import Stream, both_chains, forced_variant, post_chain

u32 = np.uint32
# mc.SHAPES: (1, 1) one live thread; (5, 3) part of a wave; (37, 29) and (130, 67) several blocks, the last one
# partial, so its waves ballot with idle lanes; (64, 4) one block exactly; (257, 1) a block and one pixel.


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("w,h", mc.SHAPES)
def test_gpu_kernel_equals_hostsim(w, h, kind, variant):
    want = mc.host_result(kind, w, h)
    with forced_variant(mc.ctx, "mt_variant", variant):
        got = meter(frame(kind, w, h), hostsim=False)
    mc.assert_words(got, want, f"{kind} {w}x{h} variant {variant}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("w,h", [(130, 67), (37, 29)])
def test_gpu_forced_block_counts(w, h, kind, blocks, variant):
    """One block walks the frame in 35 (5) grid-stride rounds; three blocks do not divide the 35 (5) rounds evenly,
    and the last round has idle threads."""
    want = mc.host_result(kind, w, h)
    with forced_variant(mc.ctx, "mt_variant", variant, mt_blocks=blocks):
        got = meter(frame(kind, w, h), hostsim=False)
    mc.assert_words(got, want, f"{kind} {w}x{h} variant {variant} blocks {blocks}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2])
def test_gpu_constant_frame_counts_every_lane(variant):
    """Every lane of every wave hits one bin: the count must be exactly 130 * 67 = 8710."""
    with forced_variant(mc.ctx, "mt_variant", variant):
        got = meter(frame("constant", 130, 67), hostsim=False)
    assert int(got[:256].max()) == 8710 and int(got[:256].sum()) == 8710 and int(got[mc.COUNTED]) == 8710
    mc.assert_words(got, mc.host_result("constant", 130, 67), f"constant 130x67 variant {variant}")


@pytest.mark.gpu
def test_gpu_device_pointers_own_stream_no_carry_over():
    L, ctx = mc.ctx(False)
    st = Stream()
    try:
        d_hist = st.upload(np.full(mc.WORDS, 0xDEADBEEF, u32))  # (garbage: the call clears it)
        # larger, then smaller: the staging of the host form is reused; the same d_hist twice in a row
        for (w, h, kind) in [(130, 67, "noise"), (37, 29, "specials"), (37, 29, "black"), (130, 67, "constant")]:
            rgba = frame(kind, w, h)
            meter(rgba, hostsim=False)  # (the host form: it sizes the staging buffer)
            d_in = st.upload(rgba)
            rt_amd.check(L, L.rt_meter_device(ctx, w, h, d_in.ptr, d_hist.ptr, st.ptr), ctx, "rt_meter_device")
            mc.assert_words(st.download(d_hist, (mc.WORDS,), u32), mc.host_result(kind, w, h), f"{kind} {w}x{h}: device form")
            nc.assert_bits(st.download(d_in, rgba.shape), rgba, f"{kind} {w}x{h}: the input changed")
        assert L.rt_last_kernel_ms(ctx) == -1.0, "the device form does not wait"
    finally:
        st.close()


def _chain(hostsim: bool, stream):
    """Cornell 40x30: a tracked [2, 2] progression, the linear resolve, the histogram, the solve at the defaults and
    rt_display with that exposure, device forms on one stream; (linear, histogram, exposure, 8-bit frame)."""
    got = post_chain(hostsim, stream)
    return tuple(got[k] for k in ("linear", "histogram", "exposure", "out8"))


@pytest.mark.gpu
def test_gpu_chain_to_the_displayed_frame_equals_hostsim():
    want, got = both_chains(_chain)
    nc.assert_bits(got[0], want[0], "chain: linear frame")
    mc.assert_words(got[1], want[1], "chain: histogram")
    assert got[2] == want[2] and want[2] != 1.5, "chain: exposure"
    assert np.array_equal(got[3], want[3]), "chain: the 8-bit frame"
    assert want[3][..., :3].min() < 64 and want[3][..., :3].max() > 128, "the frame is neither black nor white"
