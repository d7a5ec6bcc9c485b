"""The frame stages' argument errors, both forms, on the hostsim build: every call of
tests/stage_error_cases.py answers with the return code and the rt_last_error text that
tests/golden/stage_errors.json records from the build before the stages' checks were gathered into
csrc/rt_stage_args.h. No case is left out and none is extra: the file's keys are the module's, in order."""
from __future__ import annotations

import json

import pytest

import stage_error_cases as sec


@pytest.fixture(scope="module")
def golden():
    with open(sec.GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def got():
    return sec.run_all()


def test_case_list(golden, got):
    keys = sec.case_keys()
    assert len(set(keys)) == len(keys)
    assert list(golden) == keys, sorted(set(golden) ^ set(keys))
    assert list(got) == keys, sorted(set(got) ^ set(keys))
    for stage in sec.STAGES:
        for form in sec.FORMS:
            assert golden[f"{stage}/{form}/valid"] == [0, ""], (stage, form)


@pytest.mark.parametrize("form", sec.FORMS)
@pytest.mark.parametrize("stage", sec.STAGES)
def test_errors_as_recorded(golden, got, stage, form):
    prefix = f"{stage}/{form}/"
    mine = [k for k in sec.case_keys() if k.startswith(prefix)]
    assert mine
    diff = {k: (got[k], golden[k]) for k in mine if got[k] != golden[k]}
    assert not diff, f"(got, recorded) of {len(diff)} of {len(mine)} calls: {diff}"
