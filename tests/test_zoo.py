"""The geometry zoo on the CPU (tests/zoo_cases.py): the oracle against the reference's own
answers (tests/golden/zoo_*.npz, tools/gen_golden_zoo.py) and against a float64
Moller-Trumbore; the hostsim build of the device code (the exact octree walk, the search-BVH
walks of rt_fast.h behind rt_query, the wavefront render) against the oracle, bit for bit, on
every scene at every octree setting, with the one-slab leaf verification and with the full
ancestor-chain loop (rt_test_schedule "chain_full"); and the proof that each degenerate scene
reaches its hazard."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import pytest

import golden_io as gio
import zoo_cases as zc
from conftest import load_golden
from test_gpu_parity import assert_parity
from test_oracle_pinned import _hits_to_i32

import rt_amd

CASES = [(s, st) for s in zc.SCENES for st in zc.SETTINGS]
IDS = [f"{s}-{st[0]}-{st[1]}" for s, st in CASES]

with open(os.path.join(gio.GOLDEN, "zoo_manifest.json")) as _f:
    MANIFEST = json.load(_f)


def test_scenes_hold_their_hazards():
    """What the generator promises, read back from its arrays."""
    for name in zc.SCENES:
        t = zc.triangles(name)
        assert t.dtype == np.float32 and t.shape[0] <= 6144 and np.isfinite(t).all()
        r = zc.rays(name)
        assert r.shape == (zc.N_RAYS, 6) and np.isfinite(r).all()
        d = r[:, 3:6]
        axis = ((d == 0).sum(1) == 2)
        assert axis.mean() > 0.08 and np.signbit(d[axis]).any() and (d[axis] == 1).any() and (d[axis] == -1).any()

    def a(n):
        t = zc.triangles(n).astype(np.float64).reshape(-1, 3, 3)
        return np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1) / 2

    assert (a("slivers") == 0).sum() >= 2 * (2000 // 7) and (a("slivers") > 0).any() and a("slivers").max() < 1e-6
    assert (a("flat") > 0).all() and (zc.triangles("flat")[:, 1::3] == 0).all()
    lo, hi = zc.box("flat")
    assert hi[1] - lo[1] == 0.0
    assert np.unique(zc.triangles("dup"), axis=0).shape[0] == 2000  # 3 equal copies + 1 rewound
    assert np.abs(zc.triangles("offset")).max() > 8192 and np.abs(zc.triangles("tiny")).max() < 2e-3
    assert a("mix").max() / a("mix").min() > 1e10
    assert (zc.triangles("fan")[:, 0:3] == np.float32([0, 1, 0])).all()
    g = zc.triangles("grid") * 8
    assert (g == np.round(g)).all()


@pytest.mark.parametrize("name", zc.SCENES)
def test_parse_obj_round_trip(name, tmp_path):
    """%.9g vertices parse back to the generator's float32 bits; the material tables to materials()."""
    P = rt_amd.parse_obj(zc.write_obj(name, str(tmp_path)))
    mats, mi, em = zc.materials(name)
    np.testing.assert_array_equal(P.triangles.view(np.uint32), zc.triangles(name).view(np.uint32))
    np.testing.assert_array_equal(P.material_indices, mi)
    np.testing.assert_array_equal(P.emissive_triangle_indices, em)
    np.testing.assert_array_equal(P.materials.view(np.uint32), mats.view(np.uint32))


# ------------------------------------------------------------- the oracle and the hostsim library, pinned
def _pinned(name, key):
    if key in MANIFEST["scenes"][name]["unavailable"]:
        pytest.fail(f"{name}: no reference fixture for {key}")  # (none today: the reference took every scene)
    return load_golden(f"zoo_{name}.npz")[key]


def _check_hits(got, ref, what):
    """found and prim everywhere; t, point and normal where found (as tests/test_oracle_pinned.py)."""
    ref = _hits_to_i32(ref)
    np.testing.assert_array_equal(got[:, :2], ref[:, :2], err_msg=what)
    hit = ref[:, 0] == 1
    np.testing.assert_array_equal(got[hit, 2:9], ref[hit, 2:9], err_msg=what)


@pytest.mark.parametrize("name", zc.SCENES)
def test_pinned_to_the_reference(name):
    """The reference's octree, BVH::intersect, intersect_scene and frame: the oracle equals them bit
    for bit, and so does the hostsim library."""
    n = MANIFEST["n_pin"]
    rays = zc.rays(name)[:n]
    rk, rb = zc.kernel(name, True), zc.kernel(name, True, brute=True)
    sha = MANIFEST["scenes"][name]["octree_sha256"]
    assert hashlib.sha256(zc.oracle(name).octree_dump()).hexdigest() == sha
    assert hashlib.sha256(rk.bvh_dump()).hexdigest() == sha
    _check_hits(zc.oracle_intersect(name)[:n], _pinned(name, "bvh"), f"{name}: oracle, octree walk")
    _check_hits(rk.intersect(rays), _pinned(name, "bvh"), f"{name}: hostsim, octree walk")
    _check_hits(zc.oracle_intersect(name, brute=True)[:n], _pinned(name, "brute"), f"{name}: oracle, brute")
    _check_hits(rb.intersect(rays), _pinned(name, "brute"), f"{name}: hostsim, brute")
    np.testing.assert_array_equal(_pinned(name, "camera").view(np.uint32), zc.camera(name).view(np.uint32))
    want = _pinned(name, "rgba")
    assert gio.compare_rgb(zc.oracle_frame(name), want)["bitwise_fraction"] == 1.0
    assert_parity(zc.render(zc.kernel(name, True, frame=True)), want, min_bitwise=1.0)


# ------------------------------------------------------------- hostsim against the oracle, every setting
@pytest.mark.parametrize("name,setting", CASES, ids=IDS)
def test_hostsim_equals_oracle(name, setting):
    rays = zc.rays(name)
    rk = zc.kernel(name, True, setting)
    assert rk.bvh_dump() == zc.oracle(name, setting).octree_dump()
    want = zc.oracle_intersect(name, setting)
    got = rk.intersect(rays)
    np.testing.assert_array_equal(got[:, :9], want[:, :9], err_msg="rt_intersect vs the oracle")
    counts = []
    try:
        for chain_full in (0, 1):
            rk.test_schedule(chain_full=chain_full)
            np.testing.assert_array_equal(rk.intersect(rays), got, err_msg=f"rt_intersect, chain_full={chain_full}")
            np.testing.assert_array_equal(rk.query(rays, "closest"), got, err_msg=f"closest, chain_full={chain_full}")
            counts.append(rk.query_last_exact())
            np.testing.assert_array_equal(rk.query(rays, "any"), got[:, 0], err_msg=f"any, chain_full={chain_full}")
    finally:
        rk.test_schedule(chain_full=0)
    print(f"{name} {setting}: exact walks {counts[0]} of {rays.shape[0]} (chain_full: {counts[1]})")
    # every ancestor passes where the leaf does (rt_fast.h chain_ok): the loop rejects nothing more
    assert counts[0] == counts[1]
    if name in ("flat", "fan", "grid"):
        assert counts[0] >= 0.05 * rays.shape[0]
    if name in ("fan", "dup", "grid"):
        assert (zc.leaf_hits(name, setting)[:, 0] >= 3).any()


@pytest.mark.parametrize("name", zc.SCENES)
def test_hostsim_brute_equals_oracle(name):
    """USE_BVH 0: the triangle loop in buffer order (first of equal t)."""
    rays = zc.rays(name)
    rb = zc.kernel(name, True, brute=True)
    want = zc.oracle_intersect(name, brute=True)
    got = rb.intersect(rays)
    np.testing.assert_array_equal(got[:, :9], want[:, :9])
    np.testing.assert_array_equal(rb.query(rays, "closest"), got)
    assert rb.query_last_exact() == rays.shape[0]
    np.testing.assert_array_equal(rb.query(rays, "any"), got[:, 0])


@pytest.mark.parametrize("name,setting", CASES, ids=IDS)
def test_hostsim_frame_equals_oracle(name, setting):
    rk = zc.kernel(name, True, setting, frame=True)
    want = zc.oracle_frame(name, setting)
    assert_parity(zc.render(rk), want, min_bitwise=1.0)
    try:
        rk.test_schedule(chain_full=1)
        assert_parity(zc.render(rk), want, min_bitwise=1.0)
    finally:
        rk.test_schedule(chain_full=0)


def test_frames_see_their_scenes():
    """No frame is sky alone: the cameras look at the geometry."""
    import rt_cases
    from oracle_bindings import OracleScene
    F = zc.FRAME
    empty = OracleScene(np.zeros((0, 9), np.float32), np.zeros(0, np.int32), zc.materials("soup")[0],
                        np.zeros(0, np.int32), env=rt_cases.sky(F["sky"]))
    sky_only, _ = empty.render(zc.camera("soup"), F["W"], F["H"], F["spp"], F["bounces"])
    for name in ("soup", "mix", "offset", "dup", "flat", "grid", "fan"):
        diff = (zc.oracle_frame(name)[..., :3] != sky_only[..., :3]).any(-1).mean()
        assert diff > 0.1, (name, diff)


# ------------------------------------------------------------- the independent float64 check
_f64: dict = {}


def f64(name):
    if name not in _f64:
        _f64[name] = zc.mt64(zc.triangles(name), zc.rays(name))
    return _f64[name]


def check_against_f64(name, got, what):
    found, prim, t, un = f64(name)
    hit = un & (found == 1)
    np.testing.assert_array_equal(got[un, 0], found[un], err_msg=f"{name}: {what}: found")
    np.testing.assert_array_equal(got[hit, 1], prim[hit], err_msg=f"{name}: {what}: prim")
    gt = got[hit, 2].view(np.float32).astype(np.float64)
    rel = np.abs(gt - t[hit]) / t[hit]
    print(f"{name}: {what}: {un.mean():.3f} unambiguous, {hit.sum()} hits, t within {rel.max() if hit.any() else 0:.2e}")
    assert (rel <= zc.T_REL).all()


@pytest.mark.parametrize("name", ["soup", "mix", "offset", "tiny"])
def test_brute_force_equals_float64(name):
    """A float64 Moller-Trumbore over all triangles knows nothing of the oracle's code: on the rays
    whose answer does not hang on a rounding (zoo_cases.mt64), found and prim are equal and t agrees
    to 1e-5; at least half of every set is such a ray."""
    un = f64(name)[3]
    assert un.mean() >= 0.5, un.mean()
    assert (f64(name)[0][un] == 1).sum() >= 200
    check_against_f64(name, zc.oracle_intersect(name, brute=True), "oracle")
    check_against_f64(name, zc.kernel(name, True, brute=True).intersect(zc.rays(name)), "hostsim")


def verify_counts(rk):
    """(frame, slab tests of the leaf verification) of a stats render, per chain_full 0 and 1."""
    out = []
    rk.set_stats(True)
    try:
        for chain_full in (0, 1):
            rk.test_schedule(chain_full=chain_full)
            out.append((zc.render(rk), rk.stats()["verify"]))
    finally:
        rk.test_schedule(chain_full=0)
        rk.set_stats(False)
    return out


def test_chain_full_walks_the_chain():
    """The hook reaches the walks: the same frame from more slab tests (one per ancestor)."""
    (f0, v0), (f1, v1) = verify_counts(zc.kernel("fan", True, frame=True))
    np.testing.assert_array_equal(f0.view(np.uint32), f1.view(np.uint32))
    assert 0 < v0 < v1, (v0, v1)
