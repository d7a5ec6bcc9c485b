"""The inputs of tests/test_trip_code_gpu.py really produce the cases they are for, checked on the CPU
build: rt_hostsim_trip_cases walks each ray through the search BVH one item per trip, as a quad does
(rt_fast.h fast_closest_u with counters, a stack of the quads' capacity), and counts per ray the inner
trips by children hit, the trips with tied keys, the deepest stack, pops on an empty stack and overflow."""
from __future__ import annotations

import numpy as np
import pytest

import trip_cases as tc


def test_grid_has_every_push_count_and_tied_keys():
    """(a) inner trips with 0, 1, 2, 3 and 4 children hit all occur; (b) rays in the symmetry planes meet
    trips whose hit children have equal keys, and some of them hit."""
    c, want = tc.cases("grid"), tc.exact("grid")
    hist = c[:, :5].sum(0)
    print("grid: trips by children hit", hist.tolist(), "rays with tied trips", int((c[:, 5] > 0).sum()))
    assert (hist > 0).all(), hist
    tied = c[:, 5] > 0
    assert tied.sum() >= 64 and (tied & (want[:, 0] == 1)).sum() >= 32
    assert (c[:, 8] == 0).all()


def test_chain_reaches_the_stack_boundaries():
    """(c) depth 0 with a pop on an empty stack, depths CAP - 1 and CAP without overflow, and overflow."""
    c = tc.cases("chain")
    ok = c[:, 8] == 0
    print("chain: deepest stacks", np.bincount(c[ok, 6], minlength=tc.CAP + 1)[-4:].tolist(), "overflows", int((~ok).sum()))
    assert ((c[:, 6] == 0) & (c[:, 7] > 0) & ok).any()
    assert (c[ok, 6] == tc.CAP - 1).any() and (c[ok, 6] == tc.CAP).any()
    assert (~ok).any() and (c[~ok, 6] == tc.CAP + 1).any()  # (one entry beyond the capacity)
    assert (c[ok, 6] <= tc.CAP).all()


def test_strip_pushes_three_per_trip_for_long():
    """The strip keeps four children open trip after trip (long runs of three pushes, long pops)."""
    c = tc.cases("strip")
    assert c[:, 4].sum() >= 10000 and c[:, 6].max() >= 12 and (c[:, 8] == 0).all()


@pytest.mark.parametrize("name", tc.MESHES)
def test_golden_is_of_these_inputs(name):
    """The recorded hand-overs and visit counts belong to these meshes and rays."""
    g = tc.golden()
    assert str(g[f"{name}_digest"]) == tc.rays_digest(name)
    n = tc.rays(name).shape[0]
    for m in (4, 5, 8, 9):
        assert g[f"{name}_handover_{m}"].shape == (n,)
    for a in (0, 1):
        assert g[f"{name}_trips_{a}"].shape == (n, 3)


def test_golden_hands_over_the_overflowing_rays():
    """The rays the CPU walk finds overflowing are among those the recorded quad walk left to the exact walk."""
    c, g = tc.cases("chain"), tc.golden()
    assert g["chain_handover_4"][c[:, 8] == 1].all()
