"""The batched ray queries on the gfx950 library (rt_query.hip): the fixtures and in-box sets of
tests/test_query.py, bitwise against the hostsim build and against rt_intersect on the GPU,
for each kernel variant (rt_test_schedule "rq_variant": 0 the product's, 1 plain rounds,
2 per-quad refill); sizes across the kernels' boundaries with a guard region behind the
output; the device-pointer and torch forms; a render on either side of a query."""
from __future__ import annotations

import numpy as np
import pytest

import query_cases as qc
import rt_cases
from conftest import parsed_scene

import rt_amd

pytestmark = pytest.mark.gpu

VARIANTS = [0, 1, 2]
SENTINEL = 0x5A5A5A5A
GUARD_WORDS = 1024


@pytest.fixture(autouse=True)
def _product_variant():
    yield
    for key, rk in qc._kernels.items():
        if not key[1]:
            rk.test_schedule(rq_variant=0)


@pytest.mark.parametrize("name", list(qc.FIXTURES))
def test_gpu_query_fixtures(name):
    scene, spheres, _ = qc.FIXTURES[name]
    rays = qc.fixture_rays(name)
    rk = qc.kernel(scene, hostsim=False, spheres=spheres)
    rh = qc.kernel(scene, hostsim=True, spheres=spheres)
    want = rk.intersect(rays)
    host = rh.query(rays, "closest")
    host_any = rh.query(rays, "any")
    np.testing.assert_array_equal(host, want, err_msg=f"{name}: hostsim rt_query vs rt_intersect on the GPU")
    for v in VARIANTS:
        rk.test_schedule(rq_variant=v)
        np.testing.assert_array_equal(rk.query(rays, "closest"), want, err_msg=f"{name}: closest, variant {v}")
        routed = rk.query_last_exact()
        assert rk.last_kernel_ms() > 0.0
        np.testing.assert_array_equal(rk.query(rays, "any"), host_any, err_msg=f"{name}: any, variant {v}")
        if name == "brute_rays_dragon_tie_prone.npz":
            assert 0 < routed < rays.shape[0], f"variant {v}: the fallback path must run"
        if name.startswith("far_rays"):
            _, outside = qc.near_masks(scene, rays[:, 0:3].astype(np.float64))
            assert int(outside.sum()) <= routed < rays.shape[0], f"variant {v}"
    rk.test_schedule(rq_variant=0)
    # the exact flag, the sphere routing and (Cornell) the USE_BVH 0 contexts with the reference's hits
    qc.check_fixture(name, hostsim=False, brute_context=scene != "dragon")


@pytest.mark.parametrize("scene", ["cornell", "dragon"])
def test_gpu_inbox_rays(scene):
    rays = qc.inbox_rays(scene)
    n = rays.shape[0]
    rk = qc.kernel(scene, hostsim=False)
    rh = qc.kernel(scene, hostsim=True)
    want = rk.intersect(rays)
    np.testing.assert_array_equal(rh.query(rays, "closest"), want)
    for v in VARIANTS:
        rk.test_schedule(rq_variant=v)
        for mode, w in (("closest", want), ("any", want[:, 0])):
            np.testing.assert_array_equal(rk.query(rays, mode), w, err_msg=f"{mode}, variant {v}")
            e = rk.query_last_exact()
            print(f"in-box {scene} {mode} variant {v}: exact walks {e} of {n}")
            assert e <= n // 10, (mode, v, e)


def test_gpu_degenerate_rays():
    for scene in ("cornell", "dragon"):
        rays = qc.degenerate_rays(scene)
        rk = qc.kernel(scene, hostsim=False)
        want = rk.intersect(rays)
        np.testing.assert_array_equal(qc.kernel(scene, hostsim=True).query(rays, "closest"), want)
        for v in VARIANTS:
            rk.test_schedule(rq_variant=v)
            np.testing.assert_array_equal(rk.query(rays, "closest"), want, err_msg=f"{scene} variant {v}")
            np.testing.assert_array_equal(rk.query(rays, "any"), want[:, 0], err_msg=f"{scene} variant {v}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_gpu_sizes_and_guard(variant):
    """1 .. 4097 rays: less than a quad's wave share, one short of and one past 16 (a wave's
    round), 64 (a block) and 256, and past 4096; the device-pointer form on the default stream
    writes its n records and not a word of the sentinel behind them."""
    from hip_mem import DeviceBuffer
    rk = qc.kernel("dragon", hostsim=False)
    rk.test_schedule(rq_variant=variant)
    all_rays = qc.inbox_rays("dragon", 4097)
    assert all_rays.shape[0] == 4097
    want_all = rk.intersect(all_rays)
    d_rays = DeviceBuffer(all_rays.nbytes)
    d_rays.upload(all_rays)
    for mode, words in (("closest", 11), ("any", 1)):
        d_out = DeviceBuffer((4097 * words + GUARD_WORDS) * 4)
        for n in (1, 3, 15, 17, 63, 65, 255, 257, 4097):
            d_out.upload(np.full(4097 * words + GUARD_WORDS, SENTINEL, np.int32))
            rk.query_device(d_rays.ptr, n, d_out.ptr, mode=mode)
            got = d_out.download((4097 * words + GUARD_WORDS,), np.int32)
            assert rk.device_last_kernel_ms() > 0.0
            assert rk.last_kernel_ms() > 0.0  # (rt_device_last_kernel_ms stores what it read)
            w = want_all[:n] if mode == "closest" else want_all[:n, 0]
            np.testing.assert_array_equal(got[:n * words].reshape(w.shape), w, err_msg=f"{mode} n={n}")
            assert (got[n * words:] == SENTINEL).all(), f"{mode} n={n}: wrote past its {n} records"
            np.testing.assert_array_equal(rk.query(all_rays[:n], mode), w, err_msg=f"{mode} n={n} (host form)")


def test_gpu_device_form_reports_minus_one_until_read():
    from hip_mem import DeviceBuffer, hip
    rk = qc.kernel("cornell", hostsim=False)
    rays = qc.inbox_rays("cornell", 512)
    d_rays, d_out = DeviceBuffer(rays.nbytes), DeviceBuffer(512 * 44)
    d_rays.upload(rays)
    rk.query_device(d_rays.ptr, 512, d_out.ptr, mode="closest", exact=True)
    assert rk.last_kernel_ms() == -1.0
    assert hip().hipDeviceSynchronize() == 0
    assert rk.device_last_kernel_ms() > 0.0
    assert rk.query_last_exact() == 512
    np.testing.assert_array_equal(d_out.download((512, 11), np.int32), rk.intersect(rays))


def test_gpu_torch_form():
    """Tensors on a non-default stream; the second call is larger than the first, so the
    context's workspace grows between them."""
    import torch
    from rt_amd import torch_query
    P = parsed_scene("cornell")
    rk = rt_amd.RenderKernel(4, 4, 1, 1, rt_amd.Image(4, 4), P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles), rt_amd.Image(1, 1), None)
    far = qc.fixture_rays("far_rays_cornell.npz")
    stream = torch.cuda.Stream()
    for rays in (qc.inbox_rays("cornell", 1000), np.concatenate([qc.inbox_rays("cornell", 4096), far])):
        want = rk.query(rays, "closest")
        n_exact = rk.query_last_exact()
        with torch.cuda.stream(stream):
            t = torch.from_numpy(rays).to("cuda", non_blocking=False)
            seen = torch_query.query(rk, t, mode="any")
            hits = torch_query.query(rk, t)
            t_words = hits.view(torch.float32)[:, 2]
        stream.synchronize()
        assert hits.dtype == torch.int32 and tuple(hits.shape) == (rays.shape[0], 11)
        assert seen.dtype == torch.int32 and tuple(seen.shape) == (rays.shape[0],)
        np.testing.assert_array_equal(hits.cpu().numpy(), want)
        np.testing.assert_array_equal(seen.cpu().numpy(), want[:, 0])
        np.testing.assert_array_equal(t_words.cpu().numpy().view(np.int32), want[:, 2])
        assert rk.query_last_exact() == n_exact
    with pytest.raises(ValueError):
        torch_query.query(rk, torch.zeros((4, 5), device="cuda"))
    with pytest.raises(TypeError):
        torch_query.query(rk, torch.zeros((4, 6)))


def test_gpu_query_leaves_the_render_alone(cameras):
    """A 64x64 Cornell render, a query on the same context, the render again: equal frames."""
    P = parsed_scene("cornell")
    W, H = 64, 64
    fb = rt_amd.Image(W, H)
    rk = rt_amd.RenderKernel(W, H, 4, 3, fb, P.triangles, P.materials, P.emissive_triangle_indices,
                             P.material_indices, None, rt_amd.BVH(P.triangles),
                             rt_amd.Image.from_rgb(rt_cases.sky("S")), None)
    c = cameras["cornell"]
    rk.set_camera(rt_amd.Camera(c[:16], c[16]))
    start = fb.pixels.copy()
    rk.render()
    first = fb.pixels.copy()
    assert not np.array_equal(first, start)
    rays = np.concatenate([qc.inbox_rays("cornell"), qc.fixture_rays("far_rays_cornell.npz")])
    want = rk.intersect(rays)
    for v in VARIANTS:
        rk.test_schedule(rq_variant=v)
        np.testing.assert_array_equal(rk.query(rays, "closest"), want)
        np.testing.assert_array_equal(rk.query(rays, "any"), want[:, 0])
        fb.pixels[...] = start
        rk.render()
        assert np.array_equal(fb.pixels.view(np.uint32), first.view(np.uint32)), f"variant {v}"
