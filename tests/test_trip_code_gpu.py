"""The per-trip code of the search-BVH walks (rt_quad.h quad_visit and pop_within, rt_row.h row_visit,
trace_stream's trip loop) on the gfx950 library, on the inputs of tests/trip_cases.py (tests/test_trip_code.py
shows on the CPU build which cases they produce: every push count, tied keys, stack depths 0, capacity - 1,
capacity and one beyond).

Held to tests/golden/trip_code_parent.npz, recorded with the build before the branch-free push / pop
(tools/gen_golden_trip.py): the set of queries each probe walk leaves to the exact walk (quads and rows,
closest-hit and occlusion) and the quad walks' visit counts per query (quad_visit calls, child boxes, leaf
triangles) are the same, ray for ray; every settled answer is the exact walk's. Then two whole renders
against the CPU build, bit for bit (refill, drain to rows and k_tail in one frame)."""
from __future__ import annotations

import numpy as np
import pytest

import rt_cases
import trip_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tc.MESHES)
def test_handovers_equal_the_recorded_ones(name):
    """Modes 4 / 5 (quads, closest / occlusion) and 8 / 9 (rows): the -2 set is the recorded build's."""
    r, g = tc.rays(name), tc.golden()
    rk = tc.kernel(name, hostsim=False)
    for mode in (4, 5, 8, 9):
        t, _ = tc.device_queries(rk, mode, r)
        print(f"{name}: mode {mode} hands over {(t == -2.0).sum()} of {t.size} (recorded {g[f'{name}_handover_{mode}'].sum()})")
        np.testing.assert_array_equal(t == -2.0, g[f"{name}_handover_{mode}"], err_msg=f"{name}: mode {mode} hand-overs")


@pytest.mark.parametrize("name", tc.MESHES)
def test_visit_counts_equal_the_recorded_ones(name):
    """Same nodes in the same order: calls, child boxes and leaf triangles per query, closest and occlusion."""
    r, g = tc.rays(name), tc.golden()
    rk = tc.kernel(name, hostsim=False)
    for any_ in (0, 1):
        got = tc.device_trips(rk, any_, r)
        assert got[:, 0].sum() > 0
        np.testing.assert_array_equal(got, g[f"{name}_trips_{any_}"], err_msg=f"{name}: visit counts, any = {any_}")


@pytest.mark.parametrize("name", tc.MESHES)
def test_settled_answers_equal_exact_walk(name):
    """Hit triangle and t bits of every query a walk settles; an occlusion walk's flag."""
    r, want = tc.rays(name), tc.exact(name)
    rk = tc.kernel(name, hostsim=False)
    want_t = np.where(want[:, 0] == 1, want[:, 2].view(np.float32), np.float32(-1.0)).astype(np.float32)
    want_k = np.where(want[:, 0] == 1, want[:, 1], -1)
    for mode in (4, 8):
        t, k = tc.device_queries(rk, mode, r)
        ok = t != -2.0
        np.testing.assert_array_equal(t[ok].view(np.uint32), want_t[ok].view(np.uint32), err_msg=f"{name}: mode {mode} t")
        np.testing.assert_array_equal(k[ok], want_k[ok], err_msg=f"{name}: mode {mode} k")
    for mode in (5, 9):
        a, _ = tc.device_queries(rk, mode, r)
        ok = a != -2.0
        np.testing.assert_array_equal(a[ok], want[ok, 0].astype(np.float32), err_msg=f"{name}: mode {mode} occlusion")


def test_overflowing_rays_are_handed_over():
    """The rays whose stack the CPU walk finds one entry beyond the capacity come back as -2 from the quads."""
    c = tc.cases("chain")
    t, _ = tc.device_queries(tc.kernel("chain", hostsim=False), 4, tc.rays("chain"))
    assert (c[:, 8] == 1).any() and (t[c[:, 8] == 1] == -2.0).all()


@pytest.mark.parametrize("case,W,H", [("cfg1_cornell12", 64, 64), ("cfg2_dragon", 96, 54)])
def test_frame_bitwise_vs_cpu_build(case, W, H, manifest, cameras):
    """A whole render, 4 spp x 8 bounces: k_trace's refills, its drain's rows and k_tail in one frame."""
    e = rt_cases.golden_case(case, manifest)
    e["px"] = None
    frames = []
    for hostsim in (True, False):
        rk, fb = rt_cases.make_kernel(e, cameras, hostsim=hostsim, W=W, H=H, spp=4, bounces=8)
        rk.render()
        frames.append(fb.pixels.copy())
    assert np.isfinite(frames[1][..., :3]).any() and frames[1][..., :3].any()
    np.testing.assert_array_equal(frames[1].view(np.uint32), frames[0].view(np.uint32))
