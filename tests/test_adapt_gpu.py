"""Adaptive progressions on gfx950: the cases of tests/adapt_cases.py through the product library. What can fail
for a real reason here: k_adapt_select's block scan across its 1,024-tile steps and its ascending order,
k_adapt_gather's ballot ranks on partial tiles, the tile kernel's per-tile counts, a WavePass over a pixel list
under every wave plan, and the order of gather, pass, scatter, resolves and queries on a stream. The chain cases
also compare every pass with the hostsim build, word for word."""
from __future__ import annotations

import pytest

import adapt_cases as ac

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", ["zero", "median", "above"])
@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_selection_by_injected_state(shape, which):
    ac.case_select(False, shape, which)


@pytest.mark.parametrize("scene,step,off,stride", [("cornell", 2, 0, 1), ("fan", 2, 0, 1), ("cornell", 1, 0, 1),
                                                   ("cornell", 2, 1, 3)], ids=["cornell", "fan", "step1", "shard"])
def test_gpu_chain_identity_vs_hostsim(scene, step, off, stride):
    ac.case_chain(False, scene, step, off, stride, against_hostsim=True)


@pytest.mark.parametrize("name", [k for k in ac.SCHEDULES if k != "default"])
def test_gpu_chain_identity_under_a_wave_plan(name):
    ac.case_chain(False, "cornell", 2, schedule=ac.SCHEDULES[name], against_hostsim=True)


def test_gpu_checkpoint():
    ac.case_checkpoint(False)


def test_gpu_errors_and_state():
    ac.case_errors(False)


def test_gpu_python_render_kernel():
    ac.case_python(False)
