// denoise_shim_test.cpp — the drop-in's RenderKernel::denoise (include/render_kernel_hip.h,
// the call shape of Utils::OIDN_denoise) against the C ABI called directly: the same scene
// bound to a second context through rt_set_scene / rt_build_bvh / rt_set_env /
// rt_set_camera, rt_render_features + rt_denoise with the default parameters on the frame
// the drop-in rendered. Built like shim_test (the reference's headers and objects, linked to
// the hostsim build of the C ABI); tests/test_denoise_shim.py runs it.
//   denoise_shim_test <obj> <sky.raw> W H spp bounces
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
    if (argc < 7) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), spp = std::atoi(argv[5]), nb = std::atoi(argv[6]);
    ParsedOBJ obj = Utils::parse_obj(argv[1]);
    BVH bvh(&obj.triangles);
    Image sky = read_sky_raw(argv[2]);
    std::vector<float> cdf = Utils::compute_env_map_cdf(sky);
    std::vector<Sphere> spheres;
    Camera cam = Camera::CORNELL_BOX_CAMERA;

    Image fb(W, H);
    RenderKernel rk(W, H, spp, nb, fb, obj.triangles, obj.materials, obj.emissive_triangle_indices,
                    obj.material_indices, spheres, bvh, sky, cdf);
    rk.set_camera(cam);
    rk.render();
    const Image d1 = rk.denoise(fb, 1.0f), d075 = rk.denoise(fb, 0.75f);

    rt_context* c = nullptr;
    int rc = rt_create(0, &c);
    rc = rc ? rc : rt_set_scene(c, reinterpret_cast<const float*>(obj.triangles.data()), (int)obj.triangles.size(),
                                obj.material_indices.data(), (int)obj.material_indices.size(),
                                reinterpret_cast<const float*>(obj.materials.data()), (int)obj.materials.size(),
                                obj.emissive_triangle_indices.data(), (int)obj.emissive_triangle_indices.size(),
                                nullptr, 0);
    rc = rc ? rc : rt_build_bvh(c, 32, 8);
    rc = rc ? rc : rt_set_camera(c, &cam.view_matrix.m[0][0], cam.fov_dist);
    std::vector<float> alb((size_t)W * H * 4), nd(alb.size()), o1(alb.size()), o075(alb.size());
    rc = rc ? rc : rt_render_features(c, W, H, alb.data(), nd.data());
    rc = rc ? rc : rt_denoise(c, W, H, fb.data(), alb.data(), nd.data(), nullptr, 1.0f, o1.data());
    rc = rc ? rc : rt_denoise(c, W, H, fb.data(), alb.data(), nd.data(), nullptr, 0.75f, o075.data());
    if (rc) {
        std::printf("C ABI failed: %d %s\n", rc, rt_last_error(nullptr));
        return 1;
    }
    rt_destroy(c);
    const bool same1 = std::memcmp(d1.data(), o1.data(), o1.size() * 4) == 0;
    const bool same075 = std::memcmp(d075.data(), o075.data(), o1.size() * 4) == 0;
    const bool differs = std::memcmp(d1.data(), fb.data(), o1.size() * 4) != 0;
    bool alpha = true;
    for (int i = 0; i < W * H; i++) alpha = alpha && d075.data()[4 * i + 3] == 1.0f;
    std::printf("DENOISE_SHIM blend1 %d blend075 %d filtered %d alpha %d\n", same1 ? 1 : 0, same075 ? 1 : 0,
                differs ? 1 : 0, alpha ? 1 : 0);
    return same1 && same075 && differs && alpha ? 0 : 1;
}
