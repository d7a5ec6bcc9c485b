"""Sessions on gfx950: the scripts of tests/session_cases.py on one long-lived context each, under
the product's schedule and the geometry zoo's two extra ones, every step bitwise against a fresh
oracle. Only this half sees stale device state: buffers that only grow, the scene view and the
flags an upload derives, scratch carved from what an earlier call sized."""
from __future__ import annotations

import pytest

import session_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("schedule", list(session_cases.SCHEDULES))
@pytest.mark.parametrize("name", list(session_cases.SESSIONS))
def test_gpu_session(name, schedule):
    session_cases.run(name, hostsim=False, schedule=schedule)


def test_gpu_implicit_env_is_not_the_callers():
    session_cases.run_state_errors(hostsim=False)
