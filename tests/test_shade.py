"""The shading zoo on the CPU (tests/shade_cases.py): the oracle against the reference's own frames
(tests/golden/shade_*.npz, tools/gen_golden_shade.py); the hostsim build of the device code against
the oracle on every env, material table, emissive list and framebuffer on entry, bit for bit with
NaN matching NaN, as a full frame and as a scattered pixel list over a non-zero framebuffer; the
env-CDF search alone (rt_device_env_search) against the reference's loop restated in numpy at the
exact CDF entries; the search form each env takes, read from a stats render; and the proof that
each case shows what it is there for."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import golden_io as gio
import shade_cases as sc
from conftest import load_golden
from test_gpu_parity import assert_parity

import rt_amd
from rt_amd import _capi

with open(os.path.join(gio.GOLDEN, "shade_manifest.json")) as _f:
    MANIFEST = json.load(_f)

IDS = [c.name for c in sc.CASES]
# what each size of the issue's table must take (the rule itself is shade_cases.expected_form)
SIZE_FORMS = {(1, 1): "binary", (1, 8): "binary", (16, 1): "lds", (48, 7): "lds", (20, 9): "binary", (127, 5): "binary",
              (16, 1024): "lds", (16, 1025): "global", (16, 1040): "global", (16, 4097): "global", (16, 4098): "binary",
              (4096, 2): "lds", (4112, 2): "binary"}
PIXELS = gio.sample_pixels(sc.FRAME["W"], sc.FRAME["H"], 96, 5)


def test_zoo_is_what_the_issue_lists():
    assert len(sc.ENVS) == len(set(sc.ENVS)) == 13 + 8 * 3
    for (w, h), form in SIZE_FORMS.items():
        assert sc.expected_form(sc.env(f"grad_{w}x{h}")) == form, (w, h)
    forms = {n: sc.expected_form(sc.env(n)) for n in sc.ENVS}
    for c in ("black60", "first", "last", "black", "inf", "rgba"):  # monotone CDFs: the size decides
        assert [forms[f"{c}_{w}x{h}"] for w, h in sc.FORM_SIZES] == ["lds", "global", "binary"], c
    for c in ("neg", "nan"):  # a decreasing CDF, a NaN in it
        assert [forms[f"{c}_{w}x{h}"] for w, h in sc.FORM_SIZES] == ["binary"] * 3, c
    e = sc.env("black60_48x7")
    assert (e[0] == 0).all() and (e[-1] == 0).all() and (e[:, 0] == 0).all() and (e[:, -1] == 0).all()
    assert 0.55 < (e == 0).all(-1).mean() < 0.85
    assert sc.env_cdf(sc.env("black_20x9"))[-1] == 0.0
    assert np.isinf(sc.env_cdf(sc.env("inf_48x7"))[-1]) and np.isnan(sc.env_cdf(sc.env("nan_48x7"))[-1])
    assert (np.diff(sc.env_cdf(sc.env("neg_16x1040"))) < 0).sum() == 1
    a = sc.env("rgba_48x7")[..., 3]
    assert np.isnan(a).any() and np.isinf(a).any()
    t = sc.triangles("zero_area")[12].reshape(3, 3)
    assert (t[0] == t[1]).all() and sc.emissive("zero_area")[-1] == 12
    assert {c.flag for c in sc.CASES} == {"finite", "nan_expected"}


@pytest.mark.parametrize("name", sc.ENVS)
def test_product_cdf_is_the_restated_one(name):
    """rt_env_luminance_cdf over 3 or 4 channels == shade_cases.env_cdf (what ref_search reads)."""
    e = sc.env(name)
    h, w, ch = e.shape
    lum, cdf = np.empty(w * h, np.float32), np.empty(w * h, np.float32)
    L = _capi.lib(True)
    assert L.rt_env_luminance_cdf(_capi.ptr(e), w, h, ch, _capi.ptr(lum), _capi.ptr(cdf)) == 0
    want = sc.env_cdf(e)
    assert (((cdf.view(np.uint32) == want.view(np.uint32)) | (np.isnan(cdf) & np.isnan(want)))).all()


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_case_shows_what_it_is_for(case):
    """finite: no NaN, and more of the frame than test_zoo's share differs from the sky alone;
    nan_expected: a NaN pixel, and a finite one that differs from the sky alone. On the oracle."""
    want = sc.oracle_frame(case)[..., :3]
    sky = sc.sky_only_frame(case.env)[..., :3]
    nan = np.isnan(want).any(-1)
    seen = (want != sky).any(-1) & ~nan
    print(case.name, "nan", nan.mean(), "seen", seen.mean())
    if case.flag == "finite":
        assert not nan.any()
        assert seen.mean() > sc.SKY_ONLY_MIN
    else:
        assert nan.any() and seen.any()


@pytest.mark.parametrize("name", sorted(MANIFEST["pinned"]))
def test_oracle_equals_the_reference(name):
    want = load_golden(f"shade_{name}.npz")["rgba"]
    assert gio.sha256(want) == MANIFEST["pinned"][name]["rgba_sha256"]
    c = gio.compare_rgb(sc.oracle_frame(sc.BY_NAME[name]), want)
    assert c["bitwise_fraction"] == 1.0 and c["nan_mismatch"] == 0, c


def test_every_case_is_pinned_or_listed():
    assert set(MANIFEST["pinned"]) | set(MANIFEST["unavailable"]) == set(IDS)
    assert not set(MANIFEST["pinned"]) & set(MANIFEST["unavailable"])
    assert {f"env-{e}" for e in sc.ENVS} <= set(MANIFEST["pinned"])
    for name in MANIFEST["unavailable"]:
        c = sc.BY_NAME[name]
        assert c.fb != "zero" or not sc.mtl_expressible(c), name


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_hostsim_equals_oracle(case):
    rk = sc.kernel(case, True)
    assert_parity(sc.render(rk, case), sc.oracle_frame(case), min_bitwise=1.0)
    # a scattered pixel list over a framebuffer that is not zero: the case's own, or the random one
    init = sc.framebuffer(case.fb if case.fb != "zero" else "random")
    F = sc.FRAME
    want, _ = sc.oracle(case).render(sc.camera(), F["W"], F["H"], F["spp"], F["bounces"], pixels=PIXELS, fb=init.copy())
    rk.frame_buffer.pixels[...] = init
    rk.ray_trace_pixels(PIXELS)
    got = rk.frame_buffer.pixels
    assert_parity(got[PIXELS[:, 1], PIXELS[:, 0]], want, min_bitwise=1.0)
    rest = np.ones((F["H"], F["W"]), bool)
    rest[PIXELS[:, 1], PIXELS[:, 0]] = False
    np.testing.assert_array_equal(got[rest].view(np.uint32), init[rest].view(np.uint32))


@pytest.mark.parametrize("name", sc.ENVS)
def test_hostsim_env_search_equals_the_reference_loop(name):
    e = sc.env(name)
    v = sc.search_values(e)
    want = sc.ref_search(e, v)
    assert (want[:, 0] < e.shape[1]).all() and (want[:, 1] < e.shape[0]).all() and (want >= 0).all()
    rk = sc.kernel(sc.BY_NAME[f"env-{name}"], True)
    for form in (0, 1):
        np.testing.assert_array_equal(sc.env_search(rk, form, v), want, err_msg=f"{name} form {form}")


def _cdf_loads(case):
    rk = sc.kernel(case, True)
    rk.set_stats(True)
    try:
        assert_parity(sc.render(rk, case), sc.oracle_frame(case), min_bitwise=1.0)
        return rk.stats()["cdf"]
    finally:
        rk.set_stats(False)


def test_context_takes_the_expected_search_form():
    """A fence search adds exactly 6 to the CDF counter, the binary form its probes. Every env case
    has the same paths (the env only weighs them), so the same number of searches: that of the 1 x 8
    map, whose row search is always 3 probes and whose column search none."""
    searches, rem = divmod(_cdf_loads(sc.BY_NAME["env-grad_1x8"]), 3)
    assert rem == 0 and searches > 2000, searches
    assert _cdf_loads(sc.BY_NAME["env-grad_1x1"]) == 0
    for name in sc.ENVS:
        form = sc.expected_form(sc.env(name))
        loads = _cdf_loads(sc.BY_NAME[f"env-{name}"])
        print(name, form, loads, "searches", searches)
        assert (loads == 6 * searches) == (form != "binary"), (name, form, loads, searches)
