"""The gfx950 kernels of the bloom stage (k_bloom_reduce_lds, k_bloom_reduce_direct, k_bloom_expand and
k_bloom_composite, rt_bloom.hip) against the hostsim build of the same code, bit for bit with NaN matching NaN on both
outputs: the synthetic cases of bloom_cases.py under both forced bloom_variant values and the product's dispatch, the
device form on a stream of its own, and the chain from a tracked progression to the displayed frame."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import bloom_cases as bc
import meter_cases as mc
import noise_cases as nc
import rt_amd
from bloom_cases import bloom, inputs, params
from stage_gpu import Stream, both_chains, forced_variant, post_chain

NAMES = ("rgba_out", "layer_out")
# bc.SHAPES: (1, 1) every level one texel, one live thread; (5, 3) every tap clamped; (37, 29) odd at every level, a
# partial reduce tile on both axes; (130, 67) partial 64 x 4 blocks at level 0 and partial 32 x 8 tiles at level 1
# (65 x 34); (263, 41) five tiles across at level 1 (132 x 21). Levels 8 takes every shape down to 1 x 1.


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("levels", bc.LEVELS)
@pytest.mark.parametrize("w,h", bc.SHAPES)
def test_gpu_kernels_equal_hostsim(w, h, levels, variant):
    want = bc.host_result(w, h, levels)
    with forced_variant(bc.ctx, "bloom_variant", variant):
        got = bloom(inputs(w, h), params(levels=levels), hostsim=False)
    for g, x, name in zip(got, want, NAMES):
        nc.assert_bits(g, x, f"{w}x{h} levels {levels} variant {variant}: {name}")


@pytest.mark.gpu
def test_gpu_device_pointers_own_stream_and_scratch_reuse():
    L, ctx = bc.ctx(False)
    st = Stream()
    try:
        for (w, h) in [(263, 41), (37, 29)]:  # larger, then smaller: the context's pyramid is reused
            rgba = inputs(w, h)
            for levels in (8, 3):
                want = bc.host_result(w, h, levels)
                d_in = st.upload(rgba)
                outs = [st.upload(np.zeros((h, w, 4), np.float32)) for _ in range(2)]
                p = params(levels=levels)
                rt_amd.check(L, L.rt_bloom_device(ctx, w, h, d_in.ptr, ctypes.byref(p), outs[0].ptr, outs[1].ptr, st.ptr), ctx,
                             "rt_bloom_device")
                for b, x, name in zip(outs, want, NAMES):
                    nc.assert_bits(st.download(b, x.shape), x, f"{w}x{h} levels {levels}: {name}")
                nc.assert_bits(st.download(d_in, rgba.shape), rgba, f"{w}x{h}: the input changed")
            # without a layer
            out = st.upload(np.zeros((h, w, 4), np.float32))
            rt_amd.check(L, L.rt_bloom_device(ctx, w, h, d_in.ptr, ctypes.byref(p), out.ptr, None, st.ptr), ctx, "rt_bloom_device")
            nc.assert_bits(st.download(out, rgba.shape), bc.host_result(w, h, 3)[0], f"{w}x{h}: layer_out NULL")
    finally:
        st.close()


def _lum32(rgba):
    f = np.float32
    with np.errstate(all="ignore"):
        return (f(0.2126) * rgba[..., 0] + f(0.7152) * rgba[..., 1]) + f(0.0722) * rgba[..., 2]


def _params(C, frame):
    lum = _lum32(C.get(frame))
    thr = C.values["threshold"] = float(np.float32(np.percentile(lum[np.isfinite(lum)], 90)))
    return rt_amd.BloomParams(thr, 0.5 * thr, 0.2, 5)


def _chain(hostsim: bool, stream):
    """Cornell 40x30: a tracked [2, 2] progression, the linear resolve, rt_bloom with the 90th percentile of the frame's
    own luminance as its threshold, the histogram of the bloomed frame, the solve at the defaults and rt_display with
    that exposure, device forms on one stream; (linear, threshold, bloomed, layer, histogram, exposure, 8-bit frame)."""
    got = post_chain(hostsim, stream, bloom=_params)
    return tuple(got[k] for k in ("linear", "threshold", "bloomed", "layer", "histogram", "exposure", "out8"))


@pytest.mark.gpu
def test_gpu_chain_with_the_bloom_stage_equals_hostsim():
    want, got = both_chains(_chain)
    nc.assert_bits(got[0], want[0], "chain: linear frame")
    assert got[1] == want[1], "chain: the threshold"
    nc.assert_bits(got[2], want[2], "chain: bloomed frame")
    nc.assert_bits(got[3], want[3], "chain: layer")
    mc.assert_words(got[4], want[4], "chain: histogram")
    assert got[5] == want[5], "chain: exposure"
    assert np.array_equal(got[6], want[6]), "chain: the 8-bit frame"
    lum = _lum32(want[0])
    above, below = lum > np.float32(want[1]), lum < np.float32(want[1])
    assert above.any(), "some pixels are above the threshold"
    assert (_lum32(want[2])[below] > lum[below]).any(), "some pixel below the threshold got brighter"
