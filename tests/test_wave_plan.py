"""The wavefront plan (rt_plan.h wave_plan: lane count, tail and fast-lane figures, each
lane's share of the launch) against a table worked out by hand from the expressions it
replaced (tests/native/plan_check.cpp)."""
from __future__ import annotations

import subprocess

from test_numerics import _native


def test_wave_plan_matches_table():
    r = subprocess.run([_native("plan_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
