"""The host / device form contract of the gfx950 stages (rt_backend_hip.h StagedCall), one case per
stage: tests/stage_cases.py."""
from __future__ import annotations

import pytest

import stage_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stage", stage_cases.STAGES)
def test_gpu_host_and_device_form(stage):
    stage_cases.case_forms(False, stage)
