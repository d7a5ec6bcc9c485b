"""The batched ray queries (rt_query, include/rt_hip.h) on the hostsim build: closest and
any-hit answers against rt_intersect and the reference-written fixtures, the routing between
the search-BVH walks and the exact walk (rt_query_last_exact), degenerate rays and the
argument checks. tests/test_query_gpu.py repeats the comparisons on the gfx950 library."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import query_cases as qc

import rt_amd
from rt_amd import _capi


@pytest.mark.parametrize("name", list(qc.FIXTURES))
def test_query_equals_intersect_and_reference(name):
    routed = qc.check_fixture(name, hostsim=True)
    if name == "brute_rays_dragon_tie_prone.npz":
        assert routed > 0, "the tie-prone rays must exercise the fallback to the exact walk"


@pytest.mark.parametrize("scene", ["cornell", "dragon"])
def test_far_origins_are_counted(scene):
    """Every origin outside the near box takes the exact walk, in either mode."""
    name = f"far_rays_{scene}.npz"
    rays = qc.fixture_rays(name)
    _, outside = qc.near_masks(scene, rays[:, 0:3].astype(np.float64))
    assert outside.sum() >= 1024
    rk = qc.kernel(scene, hostsim=True)
    for mode in ("closest", "any"):
        # (the far origins alone: the count is then exactly theirs)
        rk.query(rays[outside], mode)
        assert rk.query_last_exact() == int(outside.sum()), mode
        rk.query(rays, mode)
        assert rk.query_last_exact() >= int(outside.sum()), mode


@pytest.mark.parametrize("scene", ["cornell", "dragon"])
def test_inbox_rays_mostly_settle(scene):
    """Origins inside the scene's box: at most 10 % of the queries need the exact walk (the cap
    tests/test_far_origin.py applies to near rays), and the answers are rt_intersect's."""
    rays = qc.inbox_rays(scene)
    n = rays.shape[0]
    assert n == 4096
    rk = qc.kernel(scene, hostsim=True)
    want = rk.intersect(rays)
    for mode, w in (("closest", want), ("any", want[:, 0])):
        np.testing.assert_array_equal(rk.query(rays, mode), w, err_msg=mode)
        e = rk.query_last_exact()
        print(f"in-box {scene} {mode}: exact walks {e} of {n}")
        assert e <= n // 10, (mode, e)


@pytest.mark.parametrize("scene", ["cornell", "dragon"])
def test_degenerate_rays(scene):
    rays = qc.degenerate_rays(scene)
    rk = qc.kernel(scene, hostsim=True)
    want = rk.intersect(rays)
    assert want[-1, 0] == 1  # (the ordinary ray hits)
    for exact in (False, True):
        np.testing.assert_array_equal(rk.query(rays, "closest", exact=exact), want)
        np.testing.assert_array_equal(rk.query(rays, "any", exact=exact), want[:, 0])


def test_n_zero_and_one():
    rk = qc.kernel("cornell", hostsim=True)
    rays = qc.inbox_rays("cornell")
    for mode, cols in (("closest", (0, 11)), ("any", (0,))):
        rk.query(rays[:64], mode, exact=True)
        assert rk.query_last_exact() == 64
        out = rk.query(rays[:0], mode)
        assert out.shape == cols and out.dtype == np.int32
        assert rk.query_last_exact() == 0
    # n == 0 needs no buffers at all
    assert rk.L.rt_query(rk.ctx, _capi.QUERY_CLOSEST, None, 0, None) == rt_amd.RT_OK
    assert rk.L.rt_query_device(rk.ctx, _capi.QUERY_ANY, None, 0, None, None) == rt_amd.RT_OK
    want = rk.intersect(rays[:1])
    np.testing.assert_array_equal(rk.query(rays[:1], "closest"), want)
    np.testing.assert_array_equal(rk.query(rays[:1], "any"), want[:, 0])


def test_argument_errors():
    rk = qc.kernel("cornell", hostsim=True)
    L = rk.L
    rays = qc.inbox_rays("cornell")[:4]
    out = np.zeros((4, 11), np.int32)
    p, po = _capi.ptr(rays), _capi.ptr(out)
    bad = [
        ("unknown mode", (2, p, 4, po)),
        ("unknown mode", (_capi.QUERY_EXACT | 7, p, 4, po)),
        ("negative", (_capi.QUERY_CLOSEST, p, -1, po)),
        ("2^27", (_capi.QUERY_ANY, p, 1 << 27, po)),
        ("NULL", (_capi.QUERY_CLOSEST, None, 4, po)),
        ("NULL", (_capi.QUERY_CLOSEST, p, 4, None)),
    ]
    for word, args in bad:
        for fn, extra in ((L.rt_query, ()), (L.rt_query_device, (None,))):
            assert fn(rk.ctx, *args, *extra) == rt_amd.RT_ERR_ARG, (word, args)
            assert word in L.rt_last_error(rk.ctx).decode(), (word, L.rt_last_error(rk.ctx))
    with pytest.raises(ValueError):
        rk.query(rays, "nearest")
    assert L.rt_query_last_exact(None) == rt_amd.RT_ERR_ARG
    # the schedule key of the gfx950 kernel variants exists in either build
    rk.test_schedule(rq_variant=2)
    rk.test_schedule(rq_variant=0)


def test_state_error_before_scene():
    L = _capi.lib(hostsim=True)
    h = ctypes.c_void_p()
    assert L.rt_create(0, ctypes.byref(h)) == 0
    try:
        rays = np.zeros((1, 6), np.float32)
        out = np.zeros((1, 11), np.int32)
        assert L.rt_query(h, _capi.QUERY_CLOSEST, _capi.ptr(rays), 1, _capi.ptr(out)) == rt_amd.RT_ERR_STATE
        assert L.rt_query_device(h, _capi.QUERY_ANY, _capi.ptr(rays), 1, _capi.ptr(out), None) == rt_amd.RT_ERR_STATE
        assert b"scene/BVH" in L.rt_last_error(h)
        assert L.rt_query_last_exact(h) == 0
    finally:
        L.rt_destroy(h)
