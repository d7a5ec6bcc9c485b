"""The shading zoo on the gfx950 library (tests/shade_cases.py): every env, material table,
emissive list and framebuffer on entry through the wavefront render under three schedules (k_step
and k_tail each stage the env's row tables and the material table in LDS themselves), the env-CDF
search alone in both of its device forms (rt_device_env_search) at the exact CDF entries, both LDS
fallbacks in one kernel instance, the material tables as rt_render_variants replicas and the
non-zero framebuffer as rt_render_device row shards, bit for bit against the CPU oracle with NaN
matching NaN. tests/test_shade.py pins the oracle on the same cases to the reference."""
from __future__ import annotations

import numpy as np
import pytest

import rt_cases
import shade_cases as sc
from conftest import parsed_scene
from test_gpu_parity import assert_parity
from test_zoo_gpu import SCHEDULES

import rt_amd

pytestmark = pytest.mark.gpu

IDS = [c.name for c in sc.CASES]


@pytest.fixture(autouse=True)
def _product_schedule():
    yield
    for key, rk in sc._kernels.items():
        if not key[1]:
            rk.test_schedule(reset=1)


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_gpu_case_equals_oracle(case):
    """48x36 x 4 spp x 4 bounces under the product's schedule, one lane without a tail kernel and an
    early tail (k_tail shades nearly every path)."""
    rk = sc.kernel(case, False)
    want = sc.oracle_frame(case)
    for sch in SCHEDULES:
        rk.test_schedule(reset=1)
        rk.test_schedule(**sch)
        assert_parity(sc.render(rk, case), want, min_bitwise=1.0)


@pytest.mark.parametrize("name", sc.ENVS)
def test_gpu_env_search_equals_the_reference_loop(name):
    """cdf_search as the shading kernels run it (form 0, after lds_shade_init's staging) and with
    every table from global memory (form 1): x and y of every value are the reference loop's."""
    e = sc.env(name)
    v = sc.search_values(e)
    want = sc.ref_search(e, v)
    rk = sc.kernel(sc.BY_NAME[f"env-{name}"], False)
    for form in (0, 1):
        np.testing.assert_array_equal(sc.env_search(rk, form, v), want, err_msg=f"{name} form {form}")


@pytest.mark.parametrize("name", ["grad_16x1040", "grad_127x5"])
def test_gpu_both_lds_fallbacks_in_one_kernel(name, cameras):
    """A global-fence env and a binary env, each with the > 64 entry material table of
    test_gpu_parity.test_gpu_many_materials_match_oracle: neither LDS copy is staged."""
    from oracle_bindings import OracleScene
    P = parsed_scene("cornell")
    k, nm = 9, len(P.materials)
    mats = np.tile(P.materials, (k, 1))
    mi = (P.material_indices + nm * (np.arange(len(P.material_indices)) % k)).astype(P.material_indices.dtype)
    assert len(mats) > 64 and sc.expected_form(sc.env(name)) != "lds"
    e = sc.env(name)
    W, H, spp, nb = 48, 36, 4, 5
    c = cameras["cornell"]
    want, _ = OracleScene(P.triangles, mi, mats, P.emissive_triangle_indices, env=e).render(c, W, H, spp, nb)
    fb = rt_amd.Image(W, H)
    rk = rt_amd.RenderKernel(W, H, spp, nb, fb, P.triangles, mats, P.emissive_triangle_indices, mi, None,
                             rt_amd.BVH(P.triangles), rt_amd.Image.from_rgb(e), None)
    rk.set_camera(rt_amd.Camera(c[:16], c[16]))
    for sch in SCHEDULES:
        rk.test_schedule(reset=1)
        rk.test_schedule(**sch)
        fb.pixels[...] = np.float32([0.0, 0.0, 0.0, 1.0])
        rk.render()
        assert_parity(fb.pixels, want, min_bitwise=1.0)


DEFAULT = sc.Case("mat-default", "mat", "S", "default", "default", "zero", "finite")


def test_gpu_material_tables_as_variants():
    """rt_render_variants over every table of the material zoo on one device: variant v is the
    oracle's frame for table v. Tables with an emitting primitive and without one (emit0) alternate,
    so the BRDF-to-light ray (bl_rays) is switched per variant."""
    keys = ["default", "emit0"] + [k for k in sc.MATS[1:] if k != "emit0"] + ["emit0", "default"]
    cases = [DEFAULT if k == "default" else sc.BY_NAME[f"mat-{k}"] for k in keys]
    rk = sc.kernel(DEFAULT, False)
    frames = rk.render_variants([sc.materials(k) for k in keys])
    for v, c in enumerate(cases):
        print("variant", v, c.name)
        assert_parity(frames[v], sc.oracle_frame(c), min_bitwise=1.0)
    # the bound table is untouched
    assert_parity(sc.render(rk, DEFAULT), sc.oracle_frame(DEFAULT), min_bitwise=1.0)


def test_gpu_empty_light_list_keeps_the_brdf_light_ray():
    """No listed light but emitting materials (em-empty), then the same context's variants with and
    without emission: the frames are the oracle's either way."""
    case = sc.BY_NAME["em-empty"]
    rk = sc.kernel(case, False)
    keys = ["emit0", "default", "emit0", "emit_huge"]
    frames = rk.render_variants([sc.materials(k) for k in keys])
    for v, k in enumerate(keys):
        assert_parity(frames[v], sc.oracle_frame(case._replace(name=f"em-empty-{k}", mats=k)), min_bitwise=1.0)


def test_gpu_random_framebuffer_row_shards():
    """rt_render_device accumulates into its shard's rows: stride 3, every offset, from the random
    framebuffer, against the oracle's rows."""
    from hip_mem import DeviceBuffer
    case = sc.BY_NAME["fb-random"]
    rk = sc.kernel(case, False)
    want = sc.oracle_frame(case)
    init = sc.framebuffer("random")
    for off in range(3):
        rows = np.ascontiguousarray(init[off::3])
        buf = DeviceBuffer(rows.nbytes)
        buf.upload(rows)
        rk.render_device(buf.ptr, off, 3, None)
        got = buf.download(rows.shape, np.float32)
        assert_parity(got, want[off::3], min_bitwise=1.0)
        np.testing.assert_array_equal(got[..., 3].view(np.uint32), want[off::3, :, 3].view(np.uint32))
