"""The hostsim build's rt_denoise and rt_denoise_var against the digests tests/golden/atrous_bits.json records
from the build before the two filters' per-pixel code was made one template (tools/gen_golden_atrous_bits.py):
every output of every case of tests/atrous_bits_cases.py, bit for bit. The gfx950 kernels are held to the
hostsim build in tests/test_denoise.py and tests/test_dnv_gpu.py, so this pins their bits as well."""
from __future__ import annotations

import json

import pytest

import atrous_bits_cases as ab


@pytest.fixture(scope="module")
def golden():
    with open(ab.GOLDEN) as f:
        return json.load(f)["cases"]


def test_case_list(golden):
    assert list(golden) == [ab.key(*c) for c in ab.CASES]
    assert len(golden) == 4 * 5 * 2


@pytest.mark.parametrize("w,h,passes,guides", ab.CASES)
def test_bits_as_recorded(golden, w, h, passes, guides):
    assert ab.digests(w, h, passes, guides) == golden[ab.key(w, h, passes, guides)]
