"""Linear radiance and the display stage on gfx950: the cases of tests/display_cases.py through the
product library. What can fail for a real reason here: a tone-map launch that still runs on one lane
or shard of a linear render, k_display's flipped-row index or partial last block, and any difference
between the device's expf / powf at a caller's exposure and gamma and the hostsim build's."""
from __future__ import annotations

import pytest

import display_cases as dc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("base", ["blank", "random"])
@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_gpu_round_trip(scene, base):
    dc.case_round_trip(False, scene, base)


@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_gpu_linear_frame_pinned_by_checkpoint(scene):
    dc.case_linear_pinned(False, scene)


def test_gpu_linear_resolve_is_pure():
    dc.case_resolve_pure(False)


@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_gpu_split_invariance(scene):
    dc.case_split(False, scene)


def test_gpu_row_shard():
    dc.case_shard(False)


def test_gpu_two_shard_loopback():
    dc.case_multi(False)


@pytest.mark.parametrize("gamma", dc.GAMMAS)
@pytest.mark.parametrize("exposure", dc.EXPOSURES)
def test_gpu_display_against_hostsim(exposure, gamma):
    dc.case_model(False, exposure, gamma)


def test_gpu_edge_values():
    dc.case_edges(False)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_rgba8_and_shapes(shape):
    dc.case_shape(False, *shape)


def test_gpu_errors():
    dc.case_errors(False)


def test_gpu_python_render_kernel():
    dc.case_python(False)
