"""The measurement hooks of the gfx950 library (rt_device_{display,noise,adapt,meter,upscale,bloom,dof,motion}_kernel_ms),
which the bench tools time the stages' kernels with: two rounds of each at 37 x 29 and 130 x 67 (partial tiles on both axes,
more than one block), starting with either kernel where the hook takes `first`. Every slot of out_ms a hook writes is
finite and above 0 and no slot beyond them is touched; the buffers left behind are the hostsim result bit for bit,
whichever kernel of the stage ran last, since both equal the CPU build. This pins the layout and the validating product
call, not the times.
The noise hook's maps and stat words are those of the hostsim build on the same injected state; the adaptive hook's list
sizes are those of the hostsim build's tile map of the same progression, which it leaves as it was."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import adapt_cases as ac
import bloom_cases as bc
import display_cases as dsp
import dof_cases as dc
import meter_cases as mt
import motion_cases as mc
import noise_cases as nc
import progress_cases as pc
import rt_amd
import temporal_cases as tc
import upscale_cases as uc

pytestmark = pytest.mark.gpu

REPS = 2
SIZES = [(37, 29), (130, 67)]
FIRSTS = [0, 1]
GUARD = -7.0  # (what the slots behind a hook's own hold before and after)
f32 = np.float32


def _dev(a):
    from hip_mem import DeviceBuffer
    a = np.ascontiguousarray(a)
    b = DeviceBuffer(a.nbytes)
    b.upload(a)
    return b


def _out(shape, dtype=f32, fill=-3):
    return _dev(np.full(shape, fill, dtype))


def _ms(rows):
    return np.full((rows + 1, REPS), GUARD, np.float64)


def _check_ms(ms, what, zero_rows=()):
    assert (ms[-1] == GUARD).all(), f"{what}: wrote past its slots"
    for k, row in enumerate(ms[:-1]):
        if k in zero_rows:
            assert (row == 0.0).all(), f"{what}: row {k} is {row}, not 0"
        else:
            assert np.isfinite(row).all() and (row > 0.0).all(), f"{what}: row {k} is {row}"


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_dof_hook(w, h, first):
    L, ctx = dc.ctx(False)
    rgba, nd = dc.inputs(w, h)
    want = dc.host_result(w, h, 4)
    d_in, d_nd, d_out, d_coc = _dev(rgba), _dev(nd), _out((h, w, 4)), _out((h, w))
    p, ms = dc.params(max_radius=4), _ms(2)
    rt_amd.check(L, L.rt_device_dof_kernel_ms(ctx, w, h, d_in.ptr, d_nd.ptr, ctypes.byref(p), d_out.ptr, d_coc.ptr, REPS, first,
                                              rt_amd.ptr(ms)), ctx, "rt_device_dof_kernel_ms")
    _check_ms(ms, f"dof {w}x{h} first {first}")
    nc.assert_bits(d_out.download((h, w, 4), f32), want[0], f"dof {w}x{h} first {first}: rgba_out")
    nc.assert_bits(d_coc.download((h, w), f32), want[1], f"dof {w}x{h} first {first}: coc_out")


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_motion_hook(w, h, first):
    """Without d_vec_out the vectors' row is exactly 0; with it (the context then has a camera) it is timed and the
    vectors are hostsim's."""
    rgba, nd = mc.inputs(w, h)
    m = mc.field("random", w, h, 4)
    want = mc.host_result(w, h, 4, "random")
    cur, prev = tc.cameras("turn", w, h)
    guide = tc.normal_depth(cur, w, h)
    want_vec = mc.vectors(cur, prev, guide)
    L, ctx = tc.ctx(False, cur)
    d_in, d_nd, d_m, d_g = _dev(rgba), _dev(nd), _dev(m), _dev(guide)
    p = mc.params(max_radius=4)
    for vec in (False, True):
        d_out, d_reach, d_vec, ms = _out((h, w, 4)), _out((h, w)), _out((h, w, 2)), _ms(4)
        what = f"motion {w}x{h} first {first} vectors {vec}"
        # (the vectors read the guide they are given: the blur's own record when there are none)
        rt_amd.check(L, L.rt_device_motion_kernel_ms(ctx, w, h, d_in.ptr, d_nd.ptr, d_m.ptr, ctypes.byref(p), d_out.ptr, d_reach.ptr,
                                                     rt_amd.ptr(prev.view_matrix), prev.fov_dist, d_vec.ptr if vec else None, REPS,
                                                     first, rt_amd.ptr(ms)), ctx, "rt_device_motion_kernel_ms")
        _check_ms(ms, what, zero_rows=() if vec else (3,))
        nc.assert_bits(d_out.download((h, w, 4), f32), want[0], what + ": rgba_out")
        nc.assert_bits(d_reach.download((h, w), f32), want[1], what + ": reach_out")
    # the vectors of the guide record the cameras belong to, through the hook's own launch
    d_out, d_reach, d_vec, ms = _out((h, w, 4)), _out((h, w)), _out((h, w, 2)), _ms(4)
    rt_amd.check(L, L.rt_device_motion_kernel_ms(ctx, w, h, d_in.ptr, d_g.ptr, d_m.ptr, ctypes.byref(p), d_out.ptr, d_reach.ptr,
                                                 rt_amd.ptr(prev.view_matrix), prev.fov_dist, d_vec.ptr, REPS, first,
                                                 rt_amd.ptr(ms)), ctx, "rt_device_motion_kernel_ms")
    _check_ms(ms, f"motion {w}x{h} first {first}, the cameras' guide")
    nc.assert_bits(d_vec.download((h, w, 2), f32), want_vec, f"motion {w}x{h} first {first}: the vectors")


@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_bloom_hook(w, h, lds):
    """The bloom hook takes the reduce kernel instead of `first` and lays its slots out by round: 2 * levels a round."""
    L, ctx = bc.ctx(False)
    rgba = bc.inputs(w, h)
    want = bc.host_result(w, h, 3)
    d_in, d_out, d_layer = _dev(rgba), _out((h, w, 4)), _out((h, w, 4))
    p = bc.params(levels=3)
    ms = np.full(REPS * 6 + 2, GUARD, np.float64)
    rt_amd.check(L, L.rt_device_bloom_kernel_ms(ctx, w, h, d_in.ptr, ctypes.byref(p), d_out.ptr, d_layer.ptr, lds, REPS,
                                                rt_amd.ptr(ms)), ctx, "rt_device_bloom_kernel_ms")
    assert (ms[REPS * 6:] == GUARD).all(), "wrote past its slots"
    assert np.isfinite(ms[:REPS * 6]).all() and (ms[:REPS * 6] > 0.0).all(), ms
    nc.assert_bits(d_out.download((h, w, 4), f32), want[0], f"bloom {w}x{h} lds {lds}: rgba_out")
    nc.assert_bits(d_layer.download((h, w, 4), f32), want[1], f"bloom {w}x{h} lds {lds}: layer_out")


@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_meter_hook(w, h):
    """(no `first`: the direct kernel, then the LDS one, the histogram cleared in front of each)"""
    L, ctx = mt.ctx(False)
    d_in = _dev(mt.frame("noise", w, h))
    d_hist = _dev(np.full(mt.WORDS, 0xDEADBEEF, np.uint32))
    for blocks in (0, 3):
        ms = _ms(2)
        rt_amd.check(L, L.rt_device_meter_kernel_ms(ctx, w, h, d_in.ptr, d_hist.ptr, blocks, REPS, rt_amd.ptr(ms)), ctx,
                     "rt_device_meter_kernel_ms")
        _check_ms(ms, f"meter {w}x{h} blocks {blocks}")
        mt.assert_words(d_hist.download((mt.WORDS,), np.uint32), mt.host_result("noise", w, h), f"meter {w}x{h} blocks {blocks}")


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("pair", [(37, 29, 130, 67), (130, 67, 130, 67)])
def test_gpu_upscale_hook(pair, first):
    L, ctx = uc.ctx(False)
    w_lo, h_lo, w, h = pair
    case = uc.inputs(*pair)
    want = uc.host_result(pair)
    d = {k: _dev(v) for k, v in case.items()}
    d_out, d_sout, ms = _out((h, w, 4)), _out((h, w)), _ms(2)
    rt_amd.check(L, L.rt_device_upscale_kernel_ms(ctx, w_lo, h_lo, w, h, d["rgba"].ptr, d["sigma"].ptr, d["alb_lo"].ptr,
                                                  d["nd_lo"].ptr, d["alb_hi"].ptr, d["nd_hi"].ptr, d_out.ptr, d_sout.ptr, REPS,
                                                  first, rt_amd.ptr(ms)), ctx, "rt_device_upscale_kernel_ms")
    _check_ms(ms, f"upscale {pair} first {first}")
    nc.assert_bits(d_out.download((h, w, 4), f32), want[0], f"upscale {pair} first {first}: colour")
    nc.assert_bits(d_sout.download((h, w), f32), want[1], f"upscale {pair} first {first}: sigma_out")


@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_display_hook(w, h):
    """The last of the six launches writes both outputs at exposure 1.5 and gamma 2.2, rows in order."""
    lin = dsp.shape_buffer(w, h)
    host = dsp.unbound(True)
    want, want8 = dsp.display(host, lin, exposure=1.5, gamma=2.2)
    host.close()
    s = dsp.unbound(False)
    d_in, d_state, d_out, d_8 = _dev(lin), _dev(np.zeros_like(lin)), _out((h, w, 4)), _out((h, w, 4), np.uint8, 77)
    ms = _ms(6)
    s.ok(s.L.rt_device_display_kernel_ms(s.ctx, w, h, d_in.ptr, d_state.ptr, d_out.ptr, d_8.ptr, REPS, rt_amd.ptr(ms)),
         "rt_device_display_kernel_ms")
    _check_ms(ms, f"display {w}x{h}")
    nc.assert_bits(d_out.download((h, w, 4), f32), want, f"display {w}x{h}: rgba_out")
    assert np.array_equal(d_8.download((h, w, 4), np.uint8), want8), f"display {w}x{h}: rgba8_out"
    nc.assert_bits(d_in.download((h, w, 4), f32), lin, f"display {w}x{h}: the input changed")
    s.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_noise_hook(w, h):
    """The hook folds the state out of the half buffer in its first round and in again in its second, then estimates with
    n_a = n_b = 2 at threshold 0.05 after 2 passes: on sums that are small whole numbers both folds are exact, so the half
    buffer is the input again and the maps and stat words left behind are those of the hostsim build on that state."""
    rng = np.random.default_rng([nc.SEED, w, h])
    base = np.zeros((h, w, 4), f32)
    state = (2 * rng.integers(1, 32, (h, w, 4))).astype(f32)
    half = state / f32(2.0)  # (the A passes' mean is the frame's: no error), but for half of the right half's pixels
    half[:, w // 2:, :3] += (rng.random((h, w - w // 2, 1)) < 0.5).astype(f32)
    half[..., 3] = 0.0  # (the fold leaves 0 there)
    host = pc.session(True, "cornell")
    assert pc.load_rc(host, nc.pack_v2(base, state, half, total=6, done=4, passes=2, n_a=2)) == 0, host.error()
    want = nc.noise(host, 0.05)
    host.close()
    assert 0 < want[2]["tiles_over"] < want[2]["tiles"] and want[2]["nonfinite"] == 0, "the threshold splits the tiles"
    s = dsp.unbound(False)
    th, tw = (h + 7) // 8, (w + 7) // 8
    d_state, d_half, d_px, d_tl, d_st = _dev(state), _dev(half), _out((h, w)), _out((th, tw)), _out(8, np.int32)
    ms = _ms(3)
    s.ok(s.L.rt_device_noise_kernel_ms(s.ctx, w, h, d_state.ptr, d_half.ptr, d_px.ptr, d_tl.ptr, d_st.ptr, REPS, rt_amd.ptr(ms)),
         "rt_device_noise_kernel_ms")
    _check_ms(ms, f"noise {w}x{h}")
    nc.assert_bits(d_half.download((h, w, 4), f32), half, f"noise {w}x{h}: the half buffer after two folds")
    nc.assert_bits(d_state.download((h, w, 4), f32), state, f"noise {w}x{h}: the state changed")
    st = d_st.download((8,), np.int32)
    assert int(st[7]) == 0, "the eighth stat word"
    stats = dict(tiles=int(st[0]), tiles_over=int(st[1]), nonfinite=int(st[2]), max_tile=st[3:4].view(f32)[0], samples_a=int(st[4]),
                 samples_b=int(st[5]), passes=int(st[6]))
    nc.assert_noise((d_px.download((h, w), f32), d_tl.download((th, tw), f32), stats), want, f"noise {w}x{h}")
    s.close()


def _adaptive(hostsim, w, h):
    """Cornell at w x h, 8 samples: two tracked passes of 2, then an adaptive one of 2 at threshold 0."""
    s = pc.session(hostsim, "cornell")
    pc.begin(s, total=8, w=w, h=h)
    nc.track(s)
    pc.advance(s, 2)
    pc.advance(s, 2)
    ac.advance(s, 2, 0.0)
    return s


@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_adapt_hook(w, h):
    """On an adaptive progression the hook selects with no samples to add, so it lists the tiles whose error is above the
    threshold: out_active is the count of those tiles and of their pixels in the hostsim build's tile map of the same
    progression, at threshold 0 and at the map's median (about half the tiles). The progression is left as it was."""
    host = _adaptive(True, w, h)
    _, tile_err, _ = nc.noise(host, 0.0)
    host.close()
    s = _adaptive(False, w, h)
    counts, frame = ac.counts(s), dsp.resolve_linear(s)
    for thr in (0.0, float(np.median(tile_err))):
        listed = tile_err > f32(thr)
        want = [int(listed.sum()), int(ac.tile_counts_px(h, w)[listed].sum())]
        assert 0 < want[0] and (thr == 0.0 or want[0] < listed.size), "the threshold splits the tiles"
        ms, act = _ms(4), np.full(2, -7, np.int32)
        s.ok(s.L.rt_device_adapt_kernel_ms(s.ctx, ctypes.c_float(thr), REPS, rt_amd.ptr(ms), rt_amd.ptr(act)),
             "rt_device_adapt_kernel_ms")
        _check_ms(ms, f"adapt {w}x{h} threshold {thr}")
        assert act.tolist() == want, f"adapt {w}x{h} threshold {thr}: listed tiles and pixels"
    after = ac.counts(s)
    assert (after[0] == counts[0]).all() and (after[1] == counts[1]).all(), "the tile counts changed"
    nc.assert_bits(dsp.resolve_linear(s), frame, "the progression's frame changed")
    s.close()
