"""The geometry zoo on the gfx950 library (tests/zoo_cases.py): k_intersect, the quad and row
walks (rt_device_queries), the three rt_query kernel variants, the wavefront render under three
schedules (k_trace's quads, k_step's octet exact walk, k_tail's inline exact walk) and the
feature pass, bit for bit against the CPU oracle, with the one-slab leaf verification and with
the full ancestor-chain loop (rt_test_schedule "chain_full"). tests/test_zoo.py pins the oracle
on the same scenes to the reference and to a float64 check."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import zoo_cases as zc
from test_gpu_parity import assert_parity

from rt_amd import _capi

pytestmark = pytest.mark.gpu

DEFAULT = (32, 8)
# (scene, octree setting, chain_full)
CASES = ([(s, DEFAULT, 0) for s in zc.SCENES] +
         [(s, st, 0) for s in ("fan", "flat", "dup") for st in ((3, 2), (12, 1))] +
         [(s, DEFAULT, 1) for s in ("fan", "grid", "soup")])
IDS = [f"{s}-{st[0]}-{st[1]}" + ("-chain_full" if cf else "") for s, st, cf in CASES]
SCHEDULES = [{}, dict(lanes=1, tail_paths=0), dict(lanes=3, tail_paths=1, tail_enter=1000)]


@pytest.fixture(autouse=True)
def _product_schedule():
    yield
    for key, rk in zc._kernels.items():
        if not key[1]:
            rk.test_schedule(reset=1)


def _want(name, setting):
    """The oracle's answers as rt_intersect's records: the hostsim build's, once they are seen to
    be the oracle's on found .. normal (the record's last two words are rt_intersect's own)."""
    host = zc.kernel(name, True, setting).intersect(zc.rays(name))
    np.testing.assert_array_equal(host[:, :9], zc.oracle_intersect(name, setting)[:, :9])
    return host


@pytest.mark.parametrize("name,setting,chain_full", CASES, ids=IDS)
def test_gpu_intersect_equals_oracle(name, setting, chain_full):
    rk = zc.kernel(name, False, setting)
    rk.test_schedule(chain_full=chain_full)
    assert rk.bvh_dump() == zc.oracle(name, setting).octree_dump()
    np.testing.assert_array_equal(rk.intersect(zc.rays(name))[:, :9], zc.oracle_intersect(name, setting)[:, :9])


@pytest.mark.parametrize("name", ["soup", "dup", "fan"])
def test_gpu_brute_intersect_equals_oracle(name):
    rb = zc.kernel(name, False, brute=True)
    np.testing.assert_array_equal(rb.intersect(zc.rays(name))[:, :9], zc.oracle_intersect(name, brute=True)[:, :9])


def _device_queries(rk, mode, rays):
    n = rays.shape[0]
    rays8 = np.zeros((n, 8), np.float32)
    rays8[:, 0:3], rays8[:, 4:7] = rays[:, 0:3], rays[:, 3:6]
    t, k, ms = np.zeros(n, np.float32), np.zeros(n, np.int32), ctypes.c_double()
    rc = _capi.lib().rt_device_queries(rk.ctx, mode, _capi.ptr(rays8), n, 1, _capi.ptr(t), _capi.ptr(k), ctypes.byref(ms))
    assert rc == 0, _capi.lib().rt_last_error(rk.ctx)
    return t, k


def _hostsim_fast(name, setting, chain_full):
    """The hostsim build's verdict per ray (rt_hostsim_fast_queries): t, or -2 for the exact walk."""
    rh = zc.kernel(name, True, setting)
    rays = zc.rays(name)
    t, k = np.zeros(rays.shape[0], np.float32), np.zeros(rays.shape[0], np.int32)
    try:
        rh.test_schedule(chain_full=chain_full)
        assert _capi.lib(True).rt_hostsim_fast_queries(rh.ctx, _capi.ptr(rays), rays.shape[0], _capi.ptr(t), _capi.ptr(k)) == 0
    finally:
        rh.test_schedule(chain_full=0)
    return t, k


@pytest.mark.parametrize("name,setting,chain_full", CASES, ids=IDS)
def test_gpu_quad_and_row_walks_equal_oracle(name, setting, chain_full):
    """rt_device_queries modes 4 / 8 (closest, quads / rows) and 5 / 9 (occlusion): every answer a
    walk settles is the oracle's, bit for bit; rows and quads hand over the same queries, and they
    are the queries the hostsim build's one-lane walk hands over."""
    rays = zc.rays(name)
    rk = zc.kernel(name, False, setting)
    rk.test_schedule(chain_full=chain_full)
    want = zc.oracle_intersect(name, setting)
    want_t = np.where(want[:, 0] == 1, want[:, 2].view(np.float32), np.float32(-1.0)).astype(np.float32)
    want_k = np.where(want[:, 0] == 1, want[:, 1], -1)
    verdicts = []
    for mode, what in ((4, "quad"), (8, "row")):
        t, k = _device_queries(rk, mode, rays)
        ok = t != -2.0
        assert ok.any(), f"{what} closest settles nothing"
        np.testing.assert_array_equal(t[ok].view(np.uint32), want_t[ok].view(np.uint32), err_msg=f"{what} closest t")
        np.testing.assert_array_equal(k[ok], want_k[ok], err_msg=f"{what} closest prim")
        verdicts.append(ok)
    np.testing.assert_array_equal(verdicts[0], verdicts[1], err_msg="hand-overs, rows vs quads")
    host_t, _ = _hostsim_fast(name, setting, chain_full)
    host_ok = host_t != -2.0
    print(f"{name} {setting} chain_full={chain_full}: closest hand-overs quads {(~verdicts[0]).sum()}, "
          f"hostsim {(~host_ok).sum()}, only quads {(~verdicts[0] & host_ok).sum()}, only hostsim {(verdicts[0] & ~host_ok).sum()}")
    np.testing.assert_array_equal(verdicts[0], host_ok, err_msg="hand-overs, quads vs hostsim")
    flags = []
    for mode, what in ((5, "quad"), (9, "row")):
        a, _ = _device_queries(rk, mode, rays)
        ok = a != -2.0  # (-2: the bounded stack overflowed, the exact walk answers)
        print(f"{name} {setting}: {what} occlusion hand-overs {(~ok).sum()}")
        np.testing.assert_array_equal(a[ok], want[ok, 0].astype(np.float32), err_msg=f"{what} occlusion")
        flags.append(a)
    np.testing.assert_array_equal(flags[0], flags[1], err_msg="occlusion, rows vs quads")


@pytest.mark.parametrize("name,setting,chain_full", CASES, ids=IDS)
def test_gpu_rt_query_equals_oracle(name, setting, chain_full):
    """rt_query_device, each kernel variant, closest and any, on HIP allocations; the exact-walk count
    of each call is the hostsim build's for the same call."""
    from hip_mem import DeviceBuffer
    rays = zc.rays(name)
    n = rays.shape[0]
    want = _want(name, setting)
    rk, rh = zc.kernel(name, False, setting), zc.kernel(name, True, setting)
    rk.test_schedule(chain_full=chain_full)
    host_exact = {}
    try:
        rh.test_schedule(chain_full=chain_full)
        for mode in ("closest", "any"):
            rh.query(rays, mode)
            host_exact[mode] = rh.query_last_exact()
    finally:
        rh.test_schedule(chain_full=0)
    d_rays = DeviceBuffer(rays.nbytes)
    d_rays.upload(rays)
    for v in (0, 1, 2):
        rk.test_schedule(rq_variant=v)
        for mode, words, w in (("closest", 11, want), ("any", 1, want[:, 0])):
            d_out = DeviceBuffer(n * words * 4)
            d_out.upload(np.full(n * words, 0x5A5A5A5A, np.int32))
            rk.query_device(d_rays.ptr, n, d_out.ptr, mode=mode)
            got = d_out.download((n * words,), np.int32).reshape(w.shape)
            np.testing.assert_array_equal(got, w, err_msg=f"{mode}, variant {v}")
            e = rk.query_last_exact()
            print(f"{name} {setting} chain_full={chain_full} {mode} variant {v}: exact walks {e}, hostsim {host_exact[mode]}")
            assert e == host_exact[mode], (mode, v)


@pytest.mark.parametrize("name", zc.SCENES)
def test_gpu_frame_equals_oracle(name):
    """40x30 x 2 spp x 4 bounces under the product's schedule, one lane without a tail kernel
    (k_step's octet exact walk takes every hand-over) and an early tail (k_tail's inline one)."""
    rk = zc.kernel(name, False, frame=True)
    want = zc.oracle_frame(name)
    for chain_full in (0, 1) if name in ("fan", "grid", "soup") else (0,):
        for sch in SCHEDULES:
            rk.test_schedule(reset=1)
            rk.test_schedule(chain_full=chain_full, **sch)
            assert_parity(zc.render(rk), want, min_bitwise=1.0)
    if name == "flat":
        rk.test_schedule(reset=1)
        rk.set_stats(True)
        try:
            assert_parity(zc.render(rk), want, min_bitwise=1.0)
            assert rk.stats()["fallback"] > 0
        finally:
            rk.set_stats(False)


@pytest.mark.parametrize("name", ["dup", "fan"])
def test_gpu_brute_frame_equals_oracle(name):
    rb = zc.kernel(name, False, brute=True, frame=True)
    assert_parity(zc.render(rb), zc.oracle_frame(name, brute=True), min_bitwise=1.0)


@pytest.mark.parametrize("name", ["fan", "flat"])
def test_gpu_features_equal_hostsim(name):
    got = zc.kernel(name, False, frame=True).features()
    want = zc.kernel(name, True, frame=True).features()
    assert (want[1][..., 3] > 0).any()
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32))


def test_gpu_chain_full_walks_the_chain():
    """The hook reaches the device's view: the same frame from more slab tests (one per ancestor)."""
    from test_zoo import verify_counts
    (f0, v0), (f1, v1) = verify_counts(zc.kernel("fan", False, frame=True))
    np.testing.assert_array_equal(f0.view(np.uint32), f1.view(np.uint32))
    assert 0 < v0 < v1, (v0, v1)
