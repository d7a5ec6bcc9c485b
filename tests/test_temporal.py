"""Temporal accumulation on the hostsim build (rt_temporal_accumulate; include/rt_hip.h): against
temporal_cases.model(), a float64 restatement of the header comment; the exact properties and argument
errors; a static camera's running mean; the quality figure of DESIGN.md §15; the Python interface."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import dnv_cases as dv
import noise_cases as nc
import rt_amd
import temporal_cases as tc
from rt_amd import ptr
from temporal_cases import accumulate, inputs, params

f32 = np.float32


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("kind", tc.CAMERAS)
@pytest.mark.parametrize("w,h", tc.SHAPES)
def test_hostsim_matches_float64_model(w, h, kind):
    case = inputs(kind, w, h)
    got = tc.host_result(kind, w, h)
    want = tc.model(case["cur"], case["prev"], case["rgba"], case["sigma"], case["nd"], case["hist"], params())
    near = want[3]
    ec, es, el = tc.model_errors(got, want, near)
    print(f"temporal model {w}x{h} {kind}: left out {near.mean():.4f} colour {ec:.3e} sigma_out {es:.3e} len_out {el:.3e} "
          f"carried {(got[2] == 1).mean():.3f}")
    assert near.mean() <= tc.NEAR_CAP
    assert ec <= tc.COLOR_TOL and es <= tc.SIGMA_TOL and el <= tc.LEN_TOL
    assert np.all(got[0][..., 3] == 1.0)
    if kind == "away":
        assert np.all(got[2] == 1.0), "ratio <= 0 everywhere: no pixel has history"
    elif (w, h) != (1, 1):
        assert (got[2] > 1.0).any() and (got[2] == 1.0).any(), "the case has accumulated and carried pixels"


def test_turn_pushes_a_third_of_the_history_out():
    case = inputs("turn", 130, 67, faults=False)
    ln = accumulate(case, params())[2]
    out = (ln == 1.0).mean()
    print(f"turn 130x67 without faults: {out:.3f} of the pixels carried")
    assert 0.25 <= out <= 0.45


# ------------------------------------------------------------------ exact properties
def _carried(case):
    """What step 2 gives, in numpy float32: {rgb_in, 1} and sqrt(dnv_variance(sigma_in))."""
    with np.errstate(all="ignore"):
        v = case["sigma"] * case["sigma"]
    want_s = np.sqrt(np.where(np.isnan(v), f32(0), np.minimum(v, f32(tc.VMAX))).astype(f32))
    want = case["rgba"].copy()
    want[..., 3] = 1.0
    return want, want_s


@pytest.mark.parametrize("w,h", tc.SHAPES)
def test_null_history_carries_every_pixel_bitwise(w, h):
    case = inputs("shift", w, h)
    out, s, ln = tc.host_result("shift", w, h, history=False)
    want, want_s = _carried(case)
    nc.assert_bits(out, want, "rgba_out is rgba_in with alpha 1")
    nc.assert_bits(s, want_s, "sigma_out is sqrt(dnv_variance(sigma_in))")
    assert np.all(ln == 1.0)


@pytest.mark.parametrize("kind", ["same", "shift"])
def test_non_finite_colour_is_carried_whatever_the_history(kind):
    case = inputs(kind, 37, 29)
    n = 37 * 29
    bad = [divmod(n // 3, 37), divmod(n // 3 + 1, 37)]
    assert all(not np.isfinite(case["rgba"][y, x, :3]).all() for y, x in bad)
    first = tc.host_result(kind, 37, 29, history=False)
    with_h = tc.host_result(kind, 37, 29)
    other = inputs(kind, 37, 29, seed=6)
    other_h = accumulate(dict(case, hist=other["hist"]), params())
    for y, x in bad:
        for a, b, c in zip(first, with_h, other_h):
            nc.assert_bits(b[y, x], a[y, x], f"pixel ({x}, {y}) with history")
            nc.assert_bits(c[y, x], a[y, x], f"pixel ({x}, {y}) with another history")
    assert (with_h[0] != first[0]).any()


def test_inputs_are_untouched():
    case = inputs("shift", 37, 29)
    keep = [case[k].copy() for k in ("rgba", "sigma", "nd")] + [a.copy() for a in case["hist"]]
    accumulate(case, params())
    for a, b in zip([case[k] for k in ("rgba", "sigma", "nd")] + list(case["hist"]), keep):
        nc.assert_bits(a, b, "an input changed")


def test_argument_errors():
    case = inputs("shift", 5, 3)
    L, h = tc.ctx(True, case["cur"])
    ARG, STATE = rt_amd.RT_ERR_ARG, rt_amd.RT_ERR_STATE

    def rc(p=None, **over):
        r = accumulate(case, p if p is not None else params(), code=True, **over)
        assert r == 0 or L.rt_last_error(h)
        return r

    assert rc() == 0
    assert accumulate(case, None, code=True) == 0, "params NULL"
    assert accumulate(case, None, code=True, history=False) == 0, "history NULL"
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            v = [0.05, 0.9, 0.1, 32.0]
            v[k] = bad
            assert rc(params(*v)) == ARG, (bad, k)
    assert rc(params(depth_tol=-0.01)) == ARG and b"depth_tol" in L.rt_last_error(h)
    assert rc(params(depth_tol=0.0)) == 0
    for v in (-1.5, 1.01):
        assert rc(params(normal_cos=v)) == ARG and b"normal_cos" in L.rt_last_error(h)
    assert rc(params(normal_cos=-1.0)) == 0 and rc(params(normal_cos=1.0)) == 0
    for v in (-0.1, 1.0, 2.0):
        assert rc(params(min_weight=v)) == ARG and b"min_weight" in L.rt_last_error(h)
    assert rc(params(min_weight=0.0)) == 0
    assert rc(params(max_len=0.5)) == ARG and b"max_len" in L.rt_last_error(h)
    assert rc(params(max_len=1.0)) == 0
    for v in (0.0, np.nan, np.inf):
        assert rc(prev_fov=v) == ARG and b"prev_fov_dist" in L.rt_last_error(h)
    hist = case["hist"]
    for k in range(4):
        some = list(hist)
        some[k] = None
        assert rc(hist=some) == ARG and b"history" in L.rt_last_error(h)
        assert rc(hist=[a if i == k else None for i, a in enumerate(hist)]) == ARG
    # an output that aliases an input, by pointer and by overlap
    assert rc(out=case["rgba"]) == ARG and b"overlaps" in L.rt_last_error(h)
    assert rc(out=hist[0]) == ARG
    assert rc(out=case["nd"]) == ARG
    assert rc(sigma_out=case["sigma"]) == ARG
    assert rc(sigma_out=hist[1]) == ARG
    assert rc(len_out=hist[2]) == ARG
    both = np.zeros((2, 3, 5), f32)
    assert rc(sigma_out=both[0], len_out=both[0]) == ARG and b"outputs" in L.rt_last_error(h)
    assert rc(sigma_out=both[0], len_out=both[1]) == 0
    big = np.zeros(16 * 15 + 8, np.uint8)
    assert rc(rgba=big[:240].view(f32).reshape(3, 5, 4), out=big[8:248].view(f32).reshape(3, 5, 4)) == ARG
    # singular and non-finite matrices
    sing = case["prev"].view_matrix.copy()
    sing[2] = sing[1]
    assert rc(prev_view=sing) == ARG and b"singular" in L.rt_last_error(h)
    nan = case["prev"].view_matrix.copy()
    nan[1, 2] = np.nan
    assert rc(prev_view=nan) == ARG
    assert rc(prev_view=np.zeros((4, 4), f32)) == ARG
    assert rc(rgba=None) == ARG and rc(sigma=None) == ARG and rc(nd=None) == ARG
    assert rc(out=None) == ARG and rc(sigma_out=None) == ARG and rc(len_out=None) == ARG and rc(prev_view=None) == ARG
    # rt_denoise's frame-size limits
    tall4, tall1 = np.zeros((262141, 1, 4), f32), np.zeros((262141, 1), f32)
    p = params()
    assert L.rt_temporal_accumulate(h, 1, 262141, ptr(tall4), ptr(tall1), ptr(tall4), ptr(case["prev"].view_matrix),
                                    ctypes.c_float(tc.FOV), None, None, None, None, ctypes.byref(p), ptr(tall4.copy()),
                                    ptr(tall1.copy()), ptr(tall1.copy())) == ARG
    assert b"262140" in L.rt_last_error(h)
    assert L.rt_temporal_accumulate(h, 1 << 14, 1 << 13, ptr(tall4), ptr(tall1), ptr(tall4), ptr(case["prev"].view_matrix),
                                    ctypes.c_float(tc.FOV), None, None, None, None, ctypes.byref(p), ptr(tall4.copy()),
                                    ptr(tall1.copy()), ptr(tall1.copy())) == ARG
    assert b"too many pixels" in L.rt_last_error(h)
    assert L.rt_temporal_accumulate(h, 0, 3, ptr(tall4), ptr(tall1), ptr(tall4), ptr(case["prev"].view_matrix),
                                    ctypes.c_float(tc.FOV), None, None, None, None, ctypes.byref(p), ptr(tall4.copy()),
                                    ptr(tall1.copy()), ptr(tall1.copy())) == ARG
    # the device form's alignment rules
    odd4 = np.zeros(16 * 15 + 16, np.uint8)[4:]
    odd1 = np.zeros(4 * 15 + 8, np.uint8)[1:]
    o4, o1, o2 = np.zeros((3, 5, 4), f32), np.zeros((3, 5), f32), np.zeros((3, 5), f32)

    def dev(rgba=case["rgba"], sigma=case["sigma"], hs=hist[1], so=o1):
        return L.rt_temporal_accumulate_device(h, 5, 3, ptr(rgba), ptr(sigma), ptr(case["nd"]), ptr(case["prev"].view_matrix),
                                               ctypes.c_float(tc.FOV), ptr(hist[0]), ptr(hs), ptr(hist[2]), ptr(hist[3]),
                                               ctypes.byref(p), ptr(o4), ptr(so), ptr(o2), None)

    assert dev() == 0, L.rt_last_error(h)
    for kw in (dict(rgba=odd4), dict(sigma=odd1), dict(hs=odd1), dict(so=odd1)):
        assert dev(**kw) == ARG and b"aligned" in L.rt_last_error(h), kw
    assert L.rt_temporal_accumulate(None, 5, 3, ptr(case["rgba"]), ptr(case["sigma"]), ptr(case["nd"]),
                                    ptr(case["prev"].view_matrix), ctypes.c_float(tc.FOV), None, None, None, None, None,
                                    ptr(o4), ptr(o1), ptr(o2)) == ARG
    # no camera: RT_ERR_STATE, on a context of its own
    bare = ctypes.c_void_p()
    rt_amd.check(L, L.rt_create(0, ctypes.byref(bare)), None, "rt_create")
    assert L.rt_temporal_accumulate(bare, 5, 3, ptr(case["rgba"]), ptr(case["sigma"]), ptr(case["nd"]),
                                    ptr(case["prev"].view_matrix), ctypes.c_float(tc.FOV), None, None, None, None, None,
                                    ptr(o4), ptr(o1), ptr(o2)) == STATE
    assert b"camera" in L.rt_last_error(bare)
    L.rt_destroy(bare)
    d = rt_amd.temporal_default_params(hostsim=True)
    assert (round(d.depth_tol, 6), round(d.normal_cos, 6), round(d.min_weight, 6), d.max_len) == (0.05, 0.9, 0.1, 32.0)


def test_multi_device_context_runs_the_stage():
    m = nc.Session(True, name="temporal-multi", devices=[0, 1])
    case = inputs("shift", 37, 29)
    m.set_camera(case["cur"].as17())
    out, s, ln = (np.empty((29, 37, 4), f32), np.empty((29, 37), f32), np.empty((29, 37), f32))
    p = params()
    m.ok(m.L.rt_temporal_accumulate(m.ctx, 37, 29, ptr(case["rgba"]), ptr(case["sigma"]), ptr(case["nd"]),
                                    ptr(case["prev"].view_matrix), ctypes.c_float(tc.FOV), *(ptr(a) for a in case["hist"]),
                                    ctypes.byref(p), ptr(out), ptr(s), ptr(ln)), "rt_temporal_accumulate")
    for g, w, name in zip((out, s, ln), tc.host_result("shift", 37, 29), ("colour", "sigma_out", "len_out")):
        nc.assert_bits(g, w, f"multi-device context: {name}")
    m.close()


# ------------------------------------------------------------------ a static camera
@pytest.mark.parametrize("max_len", [32.0, 4.0])
def test_static_camera_is_the_running_mean(max_len):
    """K = 6 frames of independent noise (standard deviation 0.25) over a constant image: len_out = min(k, max_len),
    the colour is the running mean (an exponential one once the cap holds) and sigma_out its standard deviation."""
    w, h, K, sd = 37, 29, 6, 0.25
    case = inputs("same", w, h, faults=False)
    rng = np.random.default_rng(11)
    const = np.asarray([0.25, 0.5, 0.75], np.float64)
    sigma = np.full((h, w), sd, f32)
    hist, mean, var = None, None, None
    for k in range(1, K + 1):
        frame = np.ones((h, w, 4), f32)
        frame[..., :3] = (const + sd * rng.standard_normal((h, w, 3))).astype(f32)
        got = accumulate(dict(case, rgba=frame, sigma=sigma, hist=hist or (None,) * 4), params(max_len=max_len))
        n = min(k, max_len)
        a = 1.0 / n
        mean = frame[..., :3].astype(np.float64) if k == 1 else mean + a * (frame[..., :3] - mean)
        var = float(f32(sd)) ** 2 if k == 1 else (1 - a) ** 2 * var + a * a * float(f32(sd)) ** 2
        assert np.abs(got[2] - n).max() <= 2e-6 * n, f"frame {k}: len_out"
        assert np.abs(got[0][..., :3] - mean).max() <= tc.COLOR_TOL, f"frame {k}: colour"
        assert np.abs(got[1] - np.sqrt(var)).max() <= tc.SIGMA_TOL, f"frame {k}: sigma_out"
        if max_len >= K:
            assert abs(np.sqrt(var) - sd / np.sqrt(k)) < 1e-12
        hist = (got[0], got[1], got[2], case["nd"])
    assert np.abs(got[0][..., :3] - const).mean() < np.abs(frame[..., :3] - const).mean()


# ------------------------------------------------------------------ quality
def test_quality_accumulated_frames_filter_closer_to_converged(cameras, manifest):
    """Cornell 64x64, 8 bounces: 8 frames of 4 samples by the seeding recipe (frame k declares 64 + k samples and
    renders two passes of 2), the camera moved 0.02 along x and 0.01 along y per frame, pushed through
    TemporalHistory at the default parameters; rt_denoise_var of the last accumulated frame against rt_denoise_var
    of the last frame alone, both as RMSE against a 256-sample linear render at the last camera. Measured on the
    hostsim build: the last frame 4.528, accumulated 1.607; filtered alone 2.026, temporal 1.427;
    mean history length 7.53, 2.2 % of the pixels carried."""
    W = H = 64
    frames, samples, n0 = 8, 4, 64
    rk, fb = dv.cornell_kernel(cameras, manifest, True, W, H, 256, 8)
    hist = rt_amd.TemporalHistory()
    for k in range(frames):
        rk.set_camera(tc.moved_camera(k))
        lin, sigma = tc.recipe_frame(rk, k, n0, samples, W, H)
        acc, acc_sigma, length = hist.push(rk, lin, sigma)
    with np.errstate(all="ignore"):
        temporal = rk.denoise_var(acc, acc_sigma)
        alone = rk.denoise_var(lin, sigma)
    rk.render_linear()
    ref = fb.pixels[..., :3].astype(np.float64)
    r_in, r_acc = dv.rmse(lin.pixels, ref), dv.rmse(acc.pixels, ref)
    r_alone, r_temporal = dv.rmse(alone.pixels, ref), dv.rmse(temporal.pixels, ref)
    print(f"temporal quality: rmse last frame {r_in:.5f} accumulated {r_acc:.5f}; denoise_var alone {r_alone:.5f} "
          f"temporal {r_temporal:.5f}; mean len {length.mean():.2f} carried {(length == 1).mean():.3f}")
    assert r_temporal < r_alone


# ------------------------------------------------------------------ the Python interface
def test_python_interface_equals_the_c_abi(cameras, manifest):
    rk, _ = dv.cornell_kernel(cameras, manifest, True, 24, 20, 4, 3)
    hist = rt_amd.TemporalHistory(params={"max_len": 8.0})
    outs = []
    for k in range(2):
        rk.set_camera(tc.moved_camera(k, 0.05))
        lin, sigma = tc.recipe_frame(rk, k, 8, 4, 24, 20)
        nd = rk.features()[1]
        outs.append((lin, sigma, nd, hist.push(rk, lin, sigma)))
    (l0, s0, nd0, first), (l1, s1, nd1, second) = outs
    nc.assert_bits(first[0].pixels[..., :3], l0.pixels[..., :3], "the first push carries the frame")
    assert np.all(first[2] == 1.0) and np.all(second[2] <= 2.0) and (second[2] == 2.0).any()
    case = dict(cur=tc.moved_camera(1, 0.05), prev=tc.moved_camera(0, 0.05), rgba=l1.pixels, sigma=s1, nd=nd1,
                hist=(first[0].pixels, first[1], first[2], nd0))
    L, h = tc.ctx(True, case["cur"])
    want = accumulate(case, params(max_len=8.0))
    for g, w, name in zip((second[0].pixels, second[1], second[2]), want, ("colour", "sigma", "length")):
        nc.assert_bits(g, w, f"TemporalHistory.push vs the C ABI: {name}")
    again = rk.temporal_accumulate(l1, s1, nd1, tc.moved_camera(0, 0.05), (first[0], first[1], first[2], nd0),
                                   rt_amd.TemporalParams(0.05, 0.9, 0.1, 8.0))
    nc.assert_bits(again[0].pixels, want[0], "RenderKernel.temporal_accumulate")
    with pytest.raises(TypeError):
        rk.temporal_accumulate(l1, s1, nd1, tc.moved_camera(0), params={"length": 3})
    with pytest.raises(rt_amd.RtError):
        rk.temporal_accumulate(l1, s1, nd1, tc.moved_camera(0), params={"max_len": 0.0})
    hist.reset()
    assert hist.rgba is None and np.all(hist.push(rk, l1, s1)[2] == 1.0)
