"""The noise estimate of a tracked progression on gfx950: the cases of tests/noise_cases.py through the
product library. What can fail for a real reason here: k_noise_tiles' lane-to-pixel map, partial tiles and
partial last block, its butterfly against the pairwise tree, the atomics' totals, the device's division and
square root against numpy's, and the order of the folds against the passes, resolves and queries on a stream."""
from __future__ import annotations

import pytest

import noise_cases as nc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", ["ordinary", "edge"])
@pytest.mark.parametrize("halves", nc.HALVES, ids=lambda h: f"{h[0]}+{h[1]}")
@pytest.mark.parametrize("shape", nc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_model_by_injected_state(shape, halves, which):
    nc.case_model(False, shape, halves, which)


@pytest.mark.parametrize("split", nc.SPLITS, ids=str)
@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_gpu_fold(scene, split):
    nc.case_fold(False, scene, split)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("split", nc.SPLITS, ids=str)
def test_gpu_tracking_changes_no_frame(split, device):
    nc.case_same_frame(False, split, device)


def test_gpu_checkpoint():
    nc.case_checkpoint(False)


def test_gpu_row_shard():
    nc.case_shard(False)


def test_gpu_errors_and_state():
    nc.case_errors(False)


def test_gpu_it_measures_noise():
    nc.case_measures_noise(False)


def test_gpu_python_render_kernel():
    nc.case_python(False)
