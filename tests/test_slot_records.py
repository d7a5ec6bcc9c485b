"""The packed slot records of the wavefront (rt_wave.h): one closest-hit record per slot (HitRec:
the continuation's and the camera ray's answers, each half written with one 8-byte store), one
flags word per slot (ResFlag: the two occlusion answers and the heavy mark, a byte each) and the
pending bounce's three candidates side by side (PendRec). A layout change only: every frame is
the goldens' and the oracle's, bit for bit, whoever writes or reads the records.

Frames: the emissive Cornell box (the light kinds LSH / BL and r_bl_k), cfg1, a crop of the cfg2
dragon pixel list; 67x33 (2211 slots, no multiple of 64: the carve offsets) and 40x1 (one row) on
the emissive box against the oracle. On the GPU each once more under the schedules that change the
records' writers and readers: the heavy class on (every walk marks its slot) and off, the camera
ray traced ahead never / always / where the last sample ended, the fast lane, a few percent of the
queries through the exact walks (their octet roles write both kinds of result), one lane and the
default count, a progressive render in two passes."""
from __future__ import annotations

import numpy as np
import pytest

import rt_cases

import rt_amd

EMISSIVE = "cornell32_128"  # cornell_pbr.obj: emissive triangles, so LSH / BL rays and their results
CFG1 = "cfg1_cornell12"
DRAGON = "cfg2_dragon"
N_DRAGON_CPU = 48   # pixels of the golden list rendered by the CPU build (64 spp x 8 bounces each)
N_DRAGON_GPU = 300  # ... by the GPU build: more than one block, no multiple of 64
SIZES = [(67, 33), (40, 1)]
# Frames of a few thousand slots enter the tail kernel at once (the plan's tail_max), so the schedules that are
# about k_trace's and k_step's writers and readers switch it off (tail_paths 0): the wavefront then runs to the end.
# (heavy_calls 1: every walk takes at least one quad_visit call, so every answered query marks its slot)
SCHEDULES = {
    "wave_only": dict(tail_paths=0),
    "tail_only": dict(tail_paths=1, tail_enter=1000),
    "heavy_on": dict(heavy_calls=1, tail_paths=0), "heavy_off": dict(heavy_calls=0, tail_paths=0),
    "spec_cam0": dict(spec_cam=0, tail_paths=0), "spec_cam1": dict(spec_cam=1, tail_paths=0),
    "spec_cam2": dict(spec_cam=2, tail_paths=0),
    "fallback": dict(force_fallback=29, tail_paths=0),  # ~3.4 % of the queries skip the search-BVH walk
    "fallback_heavy_tail": dict(force_fallback=29, heavy_calls=1, tail_paths=1, tail_enter=1000),
    "one_lane": dict(lanes=1),
}
_oracle: dict = {}
_default: dict = {}


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def case(name: str, manifest, n_px: int = 0) -> dict:
    e = rt_cases.golden_case(name, manifest)
    if n_px:
        e["px"], e["expected"] = e["px"][:n_px], e["expected"][:n_px]
    return e


def oracle_frame(cameras, manifest, W: int, H: int, spp: int = 3, nb: int = 4) -> np.ndarray:
    """The emissive box at W x H from the CPU restatement oracle: computed once, read-only."""
    key = (W, H, spp, nb)
    if key not in _oracle:
        e = dict(case(EMISSIVE, manifest), W=W, H=H, spp=spp, bounces=nb, px=None)
        fb = np.array(rt_cases.run_oracle(e, cameras))
        fb.setflags(write=False)
        _oracle[key] = fb
    return _oracle[key]


def sized_frame(cameras, manifest, hostsim: bool, W: int, H: int, spp: int = 3, nb: int = 4, schedule=None) -> np.ndarray:
    rk, fb = rt_cases.make_kernel(case(EMISSIVE, manifest), cameras, hostsim=hostsim, W=W, H=H, spp=spp, bounces=nb)
    if schedule:
        rk.test_schedule(**schedule)
    rk.render()
    return fb.pixels.copy()


def two_passes(cameras, manifest, hostsim: bool, W: int, H: int, spp: int = 4, nb: int = 4):
    """(the frame resolved after passes of spp - 1 and 1 samples, the one-shot frame of the same context)."""
    rk, fb = rt_cases.make_kernel(case(EMISSIVE, manifest), cameras, hostsim=hostsim, W=W, H=H, spp=spp, bounces=nb)
    rk.progress_begin()
    assert rk.progress_advance(spp - 1) == spp - 1 and rk.progress_advance(1) == spp
    got = rk.progress_resolve(rt_amd.Image(W, H)).pixels.copy()  # (not into the bound image: the render below adds to that)
    rk.progress_end()
    rk.render()
    return got, fb.pixels.copy()


# ------------------------------------------------------------------ the CPU build of the same header
@pytest.mark.parametrize("name,n_px", [(EMISSIVE, 0), (CFG1, 0), (DRAGON, N_DRAGON_CPU)])
def test_hostsim_goldens_bitwise(name, n_px, manifest, cameras):
    e = case(name, manifest, n_px)
    got = rt_cases.run_case(e, cameras, hostsim=True)
    np.testing.assert_array_equal(bits(got), bits(e["expected"]))


@pytest.mark.parametrize("W,H", SIZES)
def test_hostsim_sizes_bitwise_vs_oracle(W, H, manifest, cameras):
    want = oracle_frame(cameras, manifest, W, H)
    np.testing.assert_array_equal(bits(sized_frame(cameras, manifest, True, W, H)), bits(want))
    np.testing.assert_array_equal(bits(sized_frame(cameras, manifest, True, W, H, schedule=dict(force_fallback=29, spec_cam=2))),
                                  bits(want))


def test_hostsim_two_passes_equal_one_shot(manifest, cameras):
    got, want = two_passes(cameras, manifest, True, 67, 33)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(want), bits(oracle_frame(cameras, manifest, 67, 33, spp=4)))


# ------------------------------------------------------------------ gfx950
def gpu_default(name: str, manifest, cameras) -> np.ndarray:
    """The default schedule's frame of a golden case on the GPU: rendered once, held to the golden."""
    if name not in _default:
        e = case(name, manifest, N_DRAGON_GPU if name == DRAGON else 0)
        got = np.array(rt_cases.run_case(e, cameras, hostsim=False))
        assert np.isfinite(got[..., :3]).any() and got[..., :3].any()
        np.testing.assert_array_equal(bits(got), bits(e["expected"]), err_msg=f"{name}: default schedule vs the golden")
        got.setflags(write=False)
        _default[name] = got
    return _default[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [EMISSIVE, CFG1, DRAGON])
def test_gpu_goldens_bitwise(name, manifest, cameras):
    gpu_default(name, manifest, cameras)


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("name", [EMISSIVE, CFG1, DRAGON])
def test_gpu_schedules_equal_default_frame(name, schedule, manifest, cameras):
    want = gpu_default(name, manifest, cameras)
    e = case(name, manifest, N_DRAGON_GPU if name == DRAGON else 0)
    rk, fb = rt_cases.make_kernel(e, cameras, hostsim=False)
    rk.test_schedule(**SCHEDULES[schedule])
    rk.exact_handovers(reset=True)
    if e.get("px") is None:
        rk.render()
        got = fb.pixels
    else:
        rk.ray_trace_pixels(e["px"])
        got = fb.pixels[e["px"][:, 1], e["px"][:, 0]]
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{name} under {schedule}")
    if schedule == "fallback":  # (k_trace did hand a share of the queries to the exact walks)
        samples = (e["px"].shape[0] if e.get("px") is not None else e["W"] * e["H"]) * e["spp"]
        assert rk.exact_handovers() >= samples // 100, f"{name} under {schedule}: {rk.exact_handovers()} hand-overs"


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_gpu_sizes_bitwise_vs_oracle(W, H, manifest, cameras):
    want = oracle_frame(cameras, manifest, W, H)
    for schedule in (None, SCHEDULES["wave_only"], SCHEDULES["fallback"], SCHEDULES["fallback_heavy_tail"], SCHEDULES["heavy_on"]):
        got = sized_frame(cameras, manifest, False, W, H, schedule=schedule)
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{W}x{H} under {schedule}")


@pytest.mark.gpu
def test_gpu_fast_lane_equals_default_frame(manifest, cameras):
    """64x36 x 32 spp on the dragon, the lane's own tail kernel held back to its last ~60 paths (tail_enter), the fast
    lane from the first iteration on or from iteration 32 on: its tail kernel steps the paths it was handed (k_hand's
    mark in r_park, cleared by k_tail_fast) beside the lane's own kernels."""
    frames = {}
    for what, schedule in (("default", None), ("fast", dict(fast_k=64, fast_spp=0.0, tail_enter=0.01)),
                           ("fast_wave", dict(fast_k=64, fast_spp=1.0, tail_enter=0.01, heavy_calls=1)), ("off", dict(fast_k=0, tail_paths=0))):
        e = dict(case(DRAGON, manifest), px=None)
        rk, fb = rt_cases.make_kernel(e, cameras, hostsim=False, W=64, H=36, spp=32, bounces=8)
        if schedule:
            rk.test_schedule(**schedule)
        rk.render()
        frames[what] = fb.pixels.copy()
    assert np.isfinite(frames["default"][..., :3]).any() and frames["default"][..., :3].any()
    for what in ("fast", "fast_wave", "off"):
        np.testing.assert_array_equal(bits(frames[what]), bits(frames["default"]), err_msg=f"fast lane {what}")


@pytest.mark.gpu
def test_gpu_lane_counts_equal(manifest, cameras):
    """512x384 (3 x 65536 slots: the default plan runs three lanes, rows interleaved) against one lane, set
    through rt_device_set_lanes and through the schedule."""
    frames = {}
    for what in ("default", "set_lanes", "schedule"):
        rk, fb = rt_cases.make_kernel(case(CFG1, manifest), cameras, hostsim=False, W=512, H=384, spp=1, bounces=3)
        if what == "set_lanes":
            rk.set_lanes(1)
        elif what == "schedule":
            rk.test_schedule(lanes=1)
        rk.render()
        frames[what] = fb.pixels.copy()
    assert np.isfinite(frames["default"][..., :3]).any() and frames["default"][..., :3].any()
    for what in ("set_lanes", "schedule"):
        np.testing.assert_array_equal(bits(frames[what]), bits(frames["default"]), err_msg=what)


@pytest.mark.gpu
def test_gpu_two_passes_equal_one_shot(manifest, cameras):
    got, want = two_passes(cameras, manifest, False, 67, 33)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(want), bits(oracle_frame(cameras, manifest, 67, 33, spp=4)))
