// dnv_shim_test.cpp — the drop-in's RenderKernel::denoise_var and progress_noise_sigma
// (include/render_kernel_hip.h) against the C ABI called directly: Cornell, a tracked
// progression of 4 samples in passes of 2; in the second pass's callback the drop-in's sigma
// equals rt_progress_noise_sigma on the kernel's context and the linear frame is resolved; the
// drop-in's denoise_var of that frame then equals rt_render_features + rt_denoise_var with the
// default parameters on a second context bound to the same scene, colour and sigma_out, bit for
// bit. Built like shim_test (the reference's headers and objects, linked to the hostsim build of
// the C ABI); tests/test_dnv_shim.py runs it.
//   dnv_shim_test <obj> <sky.raw> W H bounces
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "image.h"
#include "utils.h"
#include "render_kernel_hip.h"

static Image read_sky_raw(const char* path)  // int w, h; float rgb[h][w][3]
{
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(3);
    int wh[2];
    if (std::fread(wh, 4, 2, f) != 2) std::exit(3);
    std::vector<float> rgb((size_t)wh[0] * wh[1] * 3);
    if (std::fread(rgb.data(), 4, rgb.size(), f) != rgb.size()) std::exit(3);
    std::fclose(f);
    Image out(wh[0], wh[1]);
    for (int i = 0; i < wh[0] * wh[1]; i++) out[i] = Color(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f);
    return out;
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]), spp = 4;
    ParsedOBJ obj = Utils::parse_obj(argv[1]);
    BVH bvh(&obj.triangles);
    Image sky = read_sky_raw(argv[2]);
    std::vector<float> cdf = Utils::compute_env_map_cdf(sky);
    std::vector<Sphere> spheres;
    Camera cam = Camera::CORNELL_BOX_CAMERA;
    const size_t n = (size_t)W * H;

    Image fb(W, H), linear(W, H);
    RenderKernel rk(W, H, spp, nb, fb, obj.triangles, obj.materials, obj.emissive_triangle_indices,
                    obj.material_indices, spheres, bvh, sky, cdf);
    rk.set_camera(cam);
    std::vector<float> sigma, c_sigma(n);
    bool one_pass_throws = false, sigma_same = false, resolved = false;
    rk.render_progressive_tracked(2, [&](const Image&, int done, int) {
        if (done == 2) {
            try {
                rk.progress_noise_sigma();
            } catch (const std::runtime_error&) {
                one_pass_throws = true;
            }
            return true;
        }
        sigma = rk.progress_noise_sigma();
        sigma_same = rt_progress_noise_sigma(rk.context(), c_sigma.data()) == RT_OK &&
                     std::memcmp(sigma.data(), c_sigma.data(), n * 4) == 0;
        resolved = rt_progress_resolve_linear(rk.context(), linear.data()) == RT_OK;
        return true;
    });
    if (sigma.size() != n) {
        std::printf("DNV_SHIM no sigma\n");
        return 1;
    }
    std::vector<float> left1, left075;
    const Image d1 = rk.denoise_var(linear, sigma, 1.0f, &left1), d075 = rk.denoise_var(linear, sigma, 0.75f);

    rt_context* c = nullptr;
    int rc = rt_create(0, &c);
    rc = rc ? rc : rt_set_scene(c, reinterpret_cast<const float*>(obj.triangles.data()), (int)obj.triangles.size(),
                                obj.material_indices.data(), (int)obj.material_indices.size(),
                                reinterpret_cast<const float*>(obj.materials.data()), (int)obj.materials.size(),
                                obj.emissive_triangle_indices.data(), (int)obj.emissive_triangle_indices.size(),
                                nullptr, 0);
    rc = rc ? rc : rt_build_bvh(c, 32, 8);
    rc = rc ? rc : rt_set_camera(c, &cam.view_matrix.m[0][0], cam.fov_dist);
    std::vector<float> alb(n * 4), nd(n * 4), o1(n * 4), o075(n * 4), l1(n);
    rc = rc ? rc : rt_render_features(c, W, H, alb.data(), nd.data());
    rc = rc ? rc : rt_denoise_var(c, W, H, linear.data(), sigma.data(), alb.data(), nd.data(), nullptr, 1.0f, o1.data(), l1.data());
    rc = rc ? rc : rt_denoise_var(c, W, H, linear.data(), sigma.data(), alb.data(), nd.data(), nullptr, 0.75f, o075.data(), nullptr);
    if (rc) {
        std::printf("C ABI failed: %d %s\n", rc, rt_last_error(nullptr));
        return 1;
    }
    rt_destroy(c);
    const bool same1 = std::memcmp(d1.data(), o1.data(), n * 16) == 0;
    const bool same075 = std::memcmp(d075.data(), o075.data(), n * 16) == 0;
    const bool left = left1.size() == n && std::memcmp(left1.data(), l1.data(), n * 4) == 0;
    const bool differs = std::memcmp(d1.data(), linear.data(), n * 16) != 0;
    bool bad_size = false;
    try {
        rk.denoise_var(linear, std::vector<float>(n - 1), 1.0f);
    } catch (const std::runtime_error&) {
        bad_size = true;
    }
    std::printf("DNV_SHIM one_pass_throws %d sigma %d resolved %d blend1 %d blend075 %d sigma_out %d filtered %d bad_size_throws %d\n",
                one_pass_throws ? 1 : 0, sigma_same ? 1 : 0, resolved ? 1 : 0, same1 ? 1 : 0, same075 ? 1 : 0, left ? 1 : 0,
                differs ? 1 : 0, bad_size ? 1 : 0);
    return one_pass_throws && sigma_same && resolved && same1 && same075 && left && differs && bad_size ? 0 : 1;
}
