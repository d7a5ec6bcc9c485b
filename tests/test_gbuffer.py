"""The first-hit G-buffer on the render's walks (rt_render_gbuffer, rt_gbuffer.h) on the hostsim build:
the records against rt_query(CLOSEST) on rt_camera_rays under feature_pixel's rule, against
rt_render_features, the routing counts, the gb_force_every stressor and the argument rules."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import gbuffer_cases as gc
import rt_amd
import scenes
from rt_amd import _capi


@pytest.fixture(autouse=True)
def _reset():
    yield
    gc.reset_schedules(True)


@pytest.mark.parametrize("size", gc.CPU_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scene,kind", gc.CASES)
def test_gbuffer_is_the_query_records_and_the_features(scene, kind, size):
    rk = gc.kernel(scene, True, kind)
    w, h = size
    got = rk.gbuffer(size, ids=True)
    routed = rk.gbuffer_last_exact()
    want_alb, want_nd, want_ids, rec = gc.records_from_query(rk, w, h)
    gc.assert_same(got, (want_alb, want_nd, want_ids), f"{scene} {size}: gbuffer vs the query records")
    found = rec[:, 0] == 1
    ids = got[2].reshape(-1, 2)
    np.testing.assert_array_equal(ids[found, 0], rec[found, 1])
    assert (ids[~found] == -1).all()
    np.testing.assert_array_equal(ids[found, 1], rk.gb_mat_idx[ids[found, 0]])
    feat = rk.features(size)
    gc.assert_same(got[:2], feat, f"{scene} {size}: gbuffer vs features on an in-box camera")
    # (the search-BVH walks answer the pixels of a camera inside the near box; Cornell's preset stands outside)
    assert (0 <= routed <= w * h // 10 + 1) if gc.camera_inside(scene, kind) else routed == w * h, routed
    exact = rk.gbuffer(size, exact=True, ids=True)
    assert rk.gbuffer_last_exact() == w * h
    gc.assert_same(exact[:2], feat, f"{scene} {size}: gbuffer(exact=True) vs features")
    np.testing.assert_array_equal(exact[2], got[2])
    gc.assert_same(rk.gbuffer(size), got[:2], f"{scene} {size}: without ids")
    if size == gc.BIG:
        hit = got[1][..., 3] > 0
        assert hit.any() and (got[2][hit, 0] >= 0).all()


@pytest.mark.parametrize("scene", gc.SCENES)
def test_far_camera_takes_the_exact_walk(scene):
    rk = gc.kernel(scene, True, "far")
    w, h = gc.FAR_SIZE
    assert not gc.camera_inside(scene, "far"), "the far camera lies outside the near box"
    got = rk.gbuffer(gc.FAR_SIZE, ids=True)
    assert rk.gbuffer_last_exact() == w * h
    gc.assert_same(got[:2], rk.features(gc.FAR_SIZE), f"{scene}: far camera vs features")
    assert (got[1][..., 3] > 0).any(), "the far camera still sees the scene"


@pytest.mark.parametrize("kind", ["spheres", "brute"])
def test_sphere_and_brute_contexts_equal_features(kind):
    rk = gc.kernel("cornell", True, kind)
    w, h = gc.BIG
    got = rk.gbuffer(gc.BIG, ids=True)
    assert rk.gbuffer_last_exact() == w * h
    gc.assert_same(got[:2], rk.features(gc.BIG), f"{kind}: gbuffer vs features")
    want = gc.records_from_query(rk, w, h)
    gc.assert_same(got, want[:3], f"{kind}: gbuffer vs the query records")
    if kind == "spheres":
        n_tris = gc.parsed_scene("cornell").triangles.shape[0]
        assert (got[2][..., 0] >= n_tris).any(), "a sphere is the first hit somewhere"


@pytest.mark.parametrize("every", [1, 7])
@pytest.mark.parametrize("scene,kind", gc.CASES)
def test_force_every_changes_no_output(scene, kind, every):
    rk = gc.kernel(scene, True, kind)
    w, h = gc.BIG
    want = gc.host_reference(scene, gc.BIG, kind)
    rk.test_schedule(gb_force_every=every)
    got = rk.gbuffer(gc.BIG, ids=True)
    assert rk.gbuffer_last_exact() >= -(-(w * h) // every)
    gc.assert_same(got, want, f"{scene}: gb_force_every={every}")
    rk.test_schedule(gb_force_every=0)
    rk.gbuffer(gc.BIG)
    assert gc.camera_inside(scene, kind) == (rk.gbuffer_last_exact() < -(-(w * h) // every))


def test_schedule_keys():
    rk = gc.kernel("cornell", True, "near")
    rk.test_schedule(gb_variant=2, gb_force_every=3)
    rk.test_schedule(reset=0)
    rk.gbuffer((5, 3))
    assert rk.gbuffer_last_exact() <= 1


def _call(L, h, form, w, hh, flags, alb, nd, ids):
    p = lambda a: None if a is None else ctypes.c_void_p(a)  # noqa: E731
    if form == "host":
        return L.rt_render_gbuffer(h, w, hh, flags, p(alb), p(nd), p(ids))
    return L.rt_render_gbuffer_device(h, w, hh, flags, p(alb), p(nd), p(ids), None)


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_rules(form):
    rk = gc.kernel("cornell", True)
    L, h = rk.L, rk.ctx
    w, hh = 8, 4
    n = w * hh
    store = np.zeros(64 * n + 64, np.uint8)
    base = store.ctypes.data + (-store.ctypes.data) % 16
    alb, nd, ids = base, base + 16 * n, base + 32 * n
    assert _call(L, h, form, w, hh, 0, alb, nd, ids) == 0
    assert _call(L, h, form, w, hh, _capi.GBUFFER_EXACT, alb, nd, None) == 0
    bad = rt_amd.RT_ERR_ARG
    assert _call(L, None, form, w, hh, 0, alb, nd, ids) == bad
    for ww, hw in ((0, 4), (8, 0), (-1, 4), (8, -2), (11586, 11586)):  # (11586^2 > 2^27 - 1)
        assert _call(L, h, form, ww, hw, 0, alb, nd, ids) == bad, (ww, hw)
        assert L.rt_last_error(h)
    for flags in (1, 0x200, 0x101, -1):
        assert _call(L, h, form, w, hh, flags, alb, nd, ids) == bad, flags
    assert _call(L, h, form, w, hh, 0, None, nd, ids) == bad
    assert _call(L, h, form, w, hh, 0, alb, None, ids) == bad
    # any two buffers overlapping by range
    assert _call(L, h, form, w, hh, 0, alb, alb, ids) == bad
    assert _call(L, h, form, w, hh, 0, alb, alb + 16 * (n - 1), ids) == bad
    assert _call(L, h, form, w, hh, 0, alb, nd, alb + 16 * n - 8) == bad
    assert _call(L, h, form, w, hh, 0, alb, nd, nd + 16) == bad
    # alignment: the device form only (16 bytes for the float4 buffers, 8 for ids)
    want = bad if form == "device" else 0
    assert _call(L, h, form, w, hh, 0, alb + 8, nd + 8, ids + 16) == want
    assert _call(L, h, form, w, hh, 0, alb, nd, ids + 4) == want
    assert _call(L, h, form, w, hh, 0, alb, nd, ids + 8) == 0
    assert L.rt_gbuffer_last_exact(None) == bad


@pytest.mark.parametrize("form", ["host", "device"])
def test_state_errors(form):
    L, h = gc.raw_context(True)
    buf = np.zeros(3 * 16 * 16, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    assert _call(L, h, form, 4, 4, 0, base, base + 256, None) == rt_amd.RT_ERR_STATE
    assert L.rt_last_error(h)
    # scene and BVH but no camera
    P = gc.parsed_scene("cornell")
    tris = np.ascontiguousarray(P.triangles, np.float32).reshape(-1, 9)
    mi = np.ascontiguousarray(P.material_indices, np.int32)
    mats = np.ascontiguousarray(P.materials, np.float32).reshape(-1, 10)
    ptr = rt_amd.ptr
    assert L.rt_set_scene(h, ptr(tris), tris.shape[0], ptr(mi), mi.shape[0], ptr(mats), mats.shape[0], None, 0, None, 0) == 0
    assert L.rt_build_bvh(h, 8, 4) == 0
    assert _call(L, h, form, 4, 4, 0, base, base + 256, None) == rt_amd.RT_ERR_STATE
    assert b"camera" in L.rt_last_error(h)
    L.rt_destroy(h)


NAMES = ("RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png")


def _cli(tmp_path, out, *flags):
    from rt_amd import cli
    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    return cli.main([scenes.scene_path("cornell12"), f"--sky={hdr}", "--w=16", "--h=12", "--samples=2", "--bounces=2",
                     "--hostsim", "--camera=cornell", f"--out={out}", *flags])


def test_cli_guides(tmp_path, capsys):
    assert _cli(tmp_path, tmp_path / "bad", "--guides=octets") == 2
    assert "--guides= takes walks or exact" in capsys.readouterr().err
    for flags in ((), ("--upscale=2",)):
        plain, walks, exact = (tmp_path / (n + str(len(flags))) for n in ("plain", "walks", "exact"))
        assert _cli(tmp_path, plain, *flags) == 0
        assert _cli(tmp_path, walks, "--guides=walks", *flags) == 0
        assert _cli(tmp_path, exact, "--guides=exact", *flags) == 0
        for n in NAMES:
            assert (plain / n).read_bytes() == (walks / n).read_bytes(), n
            assert (plain / n).read_bytes() == (exact / n).read_bytes(), n


def test_guide_source_switches_the_stages_to_gbuffer(monkeypatch):
    rk = gc.kernel("cornell", True, "near")
    calls = []
    real = rk.gbuffer
    monkeypatch.setattr(rk, "gbuffer", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    img = rt_amd.Image(4, 4)
    img.pixels[...] = 0.5
    a = rk.denoise(img, 1.0)
    assert not calls
    monkeypatch.setattr(rk, "guide_source", "walks")
    b = rk.denoise(img, 1.0)
    assert len(calls) == 1
    np.testing.assert_array_equal(gc.bits(a.pixels), gc.bits(b.pixels))
