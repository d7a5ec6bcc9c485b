"""Sessions on the hostsim build: one long-lived context through rebinds and resizes
(tests/session_cases.py), every step bitwise against a fresh oracle. hostsim reads the context's
host vectors directly, so this half holds the state flags and argument paths of rt_capi_host.cpp,
which the gfx950 build shares, and proves that every scripted state is one the oracle accepts."""
from __future__ import annotations

import pytest

import session_cases


@pytest.mark.parametrize("name", list(session_cases.SESSIONS))
def test_session(name):
    session_cases.run(name, hostsim=True)


def test_implicit_env_is_not_the_callers():
    session_cases.run_state_errors(hostsim=True)
