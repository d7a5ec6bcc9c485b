"""First-hit feature buffers (rt_render_features, rt_camera_rays): the guides of the
denoise stage. CPU: hostsim against what rt_intersect and the oracle answer for the same
rays. GPU: the gfx950 kernel against hostsim, bitwise."""
from __future__ import annotations

import numpy as np
import pytest

import rt_amd
import rt_cases
from oracle_bindings import OracleScene

W, H = 37, 29  # odd, not a multiple of a wave or of the 256-thread block; 5 blocks


def _cornell(cameras, manifest, hostsim, name="cornell32_128"):
    e = rt_cases.golden_case(name, manifest)
    rk, _ = rt_cases.make_kernel(e, cameras, hostsim, W=W, H=H, spp=1, bounces=1)
    return rk, e


def _tiny(cameras, hostsim, n=5):
    tris, mi, mats, em = rt_cases.tiny_scene(n)
    rk = rt_amd.RenderKernel(W, H, 1, 1, rt_amd.Image(W, H), tris, mats, em, mi, None, rt_amd.BVH(tris),
                             rt_amd.Image.from_rgb(rt_cases.sky("S")), None, hostsim=hostsim)
    c = cameras["cornell"]
    rk.set_camera(rt_amd.Camera(c[:16], c[16]))
    return rk, (tris, mi, mats, em)


def _expected_from_intersect(rk, mats, mat_idx):
    """(albedo, normal_depth) implied by rt_intersect on rt_camera_rays."""
    rays = rk.camera_rays()
    out = rk.intersect(rays.reshape(-1, 6))
    found = out[:, 0] == 1
    nd = np.zeros((H * W, 4), np.float32)
    alb = np.zeros((H * W, 4), np.float32)
    nd[:, 3] = -1.0
    nd.view(np.int32)[found, 0:3] = out[found, 6:9]
    nd.view(np.int32)[found, 3] = out[found, 2]
    m = np.asarray(mats, np.float32).reshape(-1, 10)
    alb[found, 0:3] = m[np.asarray(mat_idx)[out[found, 1]], 4:7]
    return alb.reshape(H, W, 4), nd.reshape(H, W, 4), rays, out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _case(which, cameras, manifest, hostsim):
    """(kernel, materials, material indices, oracle scene) of a named case."""
    if which == "tiny":
        rk, (tris, mi, mats, em) = _tiny(cameras, hostsim)
        return rk, mats, mi, OracleScene(tris, mi, mats, em, env=rt_cases.sky("S"))
    e = rt_cases.golden_case("cornell32_128" if which == "cornell" else "spheres_cornell32_128", manifest)
    rk, _ = rt_cases.make_kernel(e, cameras, hostsim, W=W, H=H, spp=1, bounces=1)
    P = rt_cases.parsed_scene(e["scene"])
    mats, mi, _ = rt_cases.sphere_buffers(e, P, rt_cases.materials_for(e, P))
    return rk, mats, mi, rt_cases.oracle_scene(e)


@pytest.mark.parametrize("which", ["cornell", "spheres", "tiny"])
def test_features_match_intersect_and_oracle(which, cameras, manifest):
    rk, mats, mi, S = _case(which, cameras, manifest, True)
    alb, nd = rk.features()
    want_alb, want_nd, rays, out = _expected_from_intersect(rk, mats, mi)
    np.testing.assert_array_equal(_bits(nd), _bits(want_nd))
    np.testing.assert_array_equal(_bits(alb), _bits(want_alb))
    hit = nd[..., 3] > 0
    assert hit.any()
    assert np.all(nd[~hit] == np.float32([0, 0, 0, -1])) and np.all(alb[~hit] == 0)
    # the same rays through the oracle: the same primitive and t bits
    o = S.intersect(rays.reshape(-1, 6))
    np.testing.assert_array_equal(o[:, 0], out[:, 0])
    f = out[:, 0] == 1
    np.testing.assert_array_equal(o[f, 1], out[f, 1])
    np.testing.assert_array_equal(o[f, 2], out[f, 2])


def test_camera_rays_against_float64_model(cameras, manifest):
    rk, e = _cornell(cameras, manifest, True)
    rays = rk.camera_rays().astype(np.float64)
    c = np.asarray(cameras[e["camera"]], np.float64)
    m, fov = c[:16].reshape(4, 4), c[16]

    def xform(p):
        q = m @ np.append(p, 1.0)
        return q[:3] / q[3]

    org = xform(np.zeros(3))
    for y in (0, 7, H - 1):
        for x in (0, 11, W - 1):
            xn = (x / W * 2 - 1) * (np.float32(W) / np.float32(H))
            yn = y / H * 2 - 1
            d = xform(np.array([xn, yn, fov])) - org
            d /= np.linalg.norm(d)
            np.testing.assert_allclose(rays[y, x, :3], org, atol=1e-6)
            np.testing.assert_allclose(rays[y, x, 3:], d, atol=1e-6)


def test_features_brute_force_mode_same_buffers(cameras, manifest):
    rk, _ = _cornell(cameras, manifest, True)
    alb, nd = rk.features()
    rk.set_use_bvh(False)
    alb2, nd2 = rk.features()
    np.testing.assert_array_equal(_bits(nd), _bits(nd2))
    np.testing.assert_array_equal(_bits(alb), _bits(alb2))


def test_features_state_errors():
    L = rt_amd.lib(True)
    import ctypes
    h = ctypes.c_void_p()
    assert L.rt_create(0, ctypes.byref(h)) == 0
    buf = np.zeros((4, 4, 4), np.float32)
    buf2 = np.zeros_like(buf)
    assert L.rt_render_features(h, 4, 4, rt_amd.ptr(buf), rt_amd.ptr(buf2)) == rt_amd.RT_ERR_STATE
    assert L.rt_last_error(h)
    rays = np.zeros((16, 6), np.float32)
    assert L.rt_camera_rays(h, 4, 4, rt_amd.ptr(rays)) == rt_amd.RT_ERR_STATE
    assert L.rt_last_error(h)
    L.rt_destroy(h)


# ---------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cornell", "spheres", "tiny"])
def test_gpu_features_equal_hostsim(which, cameras, manifest):
    host, _, _, _ = _case(which, cameras, manifest, True)
    dev, _, _, _ = _case(which, cameras, manifest, False)
    ha, hn = host.features()
    da, dn = dev.features()
    np.testing.assert_array_equal(_bits(dn), _bits(hn))
    np.testing.assert_array_equal(_bits(da), _bits(ha))
    assert dev.last_kernel_ms() > 0


@pytest.mark.gpu
def test_gpu_features_device_pointers(cameras, manifest):
    from test_denoise import device_array
    dev, _, _, _ = _case("cornell", cameras, manifest, False)
    ha, hn = dev.features()
    seven = np.full((H, W, 4), 7.0, np.float32)
    ta, tn = device_array(seven), device_array(seven)
    dev.features_device(ta.ptr, tn.ptr)
    np.testing.assert_array_equal(_bits(ta.get()), _bits(ha))
    np.testing.assert_array_equal(_bits(tn.get()), _bits(hn))
