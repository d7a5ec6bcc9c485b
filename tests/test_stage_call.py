"""The host and the device form of each stage on the hostsim build give the same words
(tests/stage_cases.py). The hostsim build times both forms on the host, so the -1 convention of
rt_last_kernel_ms is the gfx950 build's alone: tests/test_stage_call_gpu.py."""
from __future__ import annotations

import pytest

import stage_cases


@pytest.mark.parametrize("stage", stage_cases.STAGES)
def test_host_and_device_form(stage):
    stage_cases.case_forms(True, stage)
