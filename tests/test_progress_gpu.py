"""Progressive rendering on gfx950: the cases of tests/progress_cases.py through the product
library. Cases 1-3 are the ones that can fail for a real reason here: a pause missed in k_tail or
the fast lane, an RNG word saved at the wrong moment, a state indexed by a lane's slots."""
from __future__ import annotations

import pytest

import progress_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("split", pc.SPLITS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("scene", pc.SCENES)
def test_gpu_split_invariance(scene, split):
    pc.case_split(False, scene, split, base="random" if split == [3, 1, 2] else "blank")


def test_gpu_row_shard():
    pc.case_shard(False)


@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_gpu_seed31_line(scene):
    pc.case_seed31(False, scene)


@pytest.mark.parametrize("schedule", list(pc.SCHEDULES))
def test_gpu_schedules(schedule):
    pc.case_schedule(False, schedule)


def test_gpu_schedule_change_between_passes():
    pc.case_schedule_change(False)


def test_gpu_edges():
    pc.case_edges(False)


def test_gpu_resolve_is_pure():
    pc.case_pure(False)


def test_gpu_interleaving():
    pc.case_interleave(False)


def test_gpu_checkpoint():
    pc.case_checkpoint(False)


def test_gpu_invalidation():
    pc.case_invalidation(False)


def test_gpu_errors():
    pc.case_errors(False)


def test_gpu_python_render_kernel():
    pc.case_python(False)
