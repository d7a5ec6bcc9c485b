// temporal_shim_test.cpp — the drop-in's RenderKernel::temporal_accumulate
// (include/render_kernel_hip.h) against the C ABI called directly: Cornell, two frames under a moved
// camera, each a linear render with a synthetic sigma map; the drop-in's first frame (no history)
// and second frame (the first as its history) equal rt_render_features + rt_temporal_accumulate
// with the default parameters on a second context bound to the same scene, colour, sigma and
// length, bit for bit. Built like shim_test (the reference's headers and objects, linked to the
// hostsim build of the C ABI); tests/test_temporal_shim.py runs it.
//   temporal_shim_test <obj> <sky.raw> W H bounces
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
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]);
    ParsedOBJ obj = Utils::parse_obj(argv[1]);
    BVH bvh(&obj.triangles);
    Image sky = read_sky_raw(argv[2]);
    std::vector<float> cdf = Utils::compute_env_map_cdf(sky);
    std::vector<Sphere> spheres;
    Camera cam0 = Camera::CORNELL_BOX_CAMERA, cam1 = Camera::CORNELL_BOX_CAMERA;
    cam1.view_matrix.m[0][3] += 0.05f;
    cam1.view_matrix.m[1][3] += 0.02f;
    const size_t n = (size_t)W * H;
    std::vector<float> sigma(n);
    for (size_t i = 0; i < n; i++) sigma[i] = 0.05f + 0.01f * (float)(i % 17);

    // two linear frames of different sample totals (the seeding recipe's point: uncorrelated noise)
    Image f0(W, H), f1(W, H);
    RenderKernel rk0(W, H, 3, nb, f0, obj.triangles, obj.materials, obj.emissive_triangle_indices, obj.material_indices,
                     spheres, bvh, sky, cdf);
    rk0.set_camera(cam0);
    rk0.render_linear();
    RenderKernel rk(W, H, 4, nb, f1, obj.triangles, obj.materials, obj.emissive_triangle_indices, obj.material_indices,
                    spheres, bvh, sky, cdf);
    rk.set_camera(cam1);
    rk.render_linear();
    rk.set_camera(cam0);
    const RenderKernel::TemporalFrame t0 = rk.temporal_accumulate(f0, sigma, cam0);
    rk.set_camera(cam1);
    const RenderKernel::TemporalFrame t1 = rk.temporal_accumulate(f1, sigma, cam0, &t0);

    rt_context* c = nullptr;
    int rc = rt_create(0, &c);
    rc = rc ? rc : rt_set_scene(c, reinterpret_cast<const float*>(obj.triangles.data()), (int)obj.triangles.size(),
                                obj.material_indices.data(), (int)obj.material_indices.size(),
                                reinterpret_cast<const float*>(obj.materials.data()), (int)obj.materials.size(),
                                obj.emissive_triangle_indices.data(), (int)obj.emissive_triangle_indices.size(),
                                nullptr, 0);
    rc = rc ? rc : rt_build_bvh(c, 32, 8);
    std::vector<float> alb(n * 4), nd0(n * 4), nd1(n * 4), o0(n * 4), s0(n), l0(n), o1(n * 4), s1(n), l1(n);
    rc = rc ? rc : rt_set_camera(c, &cam0.view_matrix.m[0][0], cam0.fov_dist);
    rc = rc ? rc : rt_render_features(c, W, H, alb.data(), nd0.data());
    rc = rc ? rc : rt_temporal_accumulate(c, W, H, f0.data(), sigma.data(), nd0.data(), &cam0.view_matrix.m[0][0], cam0.fov_dist,
                                          nullptr, nullptr, nullptr, nullptr, nullptr, o0.data(), s0.data(), l0.data());
    rc = rc ? rc : rt_set_camera(c, &cam1.view_matrix.m[0][0], cam1.fov_dist);
    rc = rc ? rc : rt_render_features(c, W, H, alb.data(), nd1.data());
    rc = rc ? rc : rt_temporal_accumulate(c, W, H, f1.data(), sigma.data(), nd1.data(), &cam0.view_matrix.m[0][0], cam0.fov_dist,
                                          o0.data(), s0.data(), l0.data(), nd0.data(), nullptr, o1.data(), s1.data(), l1.data());
    if (rc) {
        std::printf("C ABI failed: %d %s\n", rc, rt_last_error(nullptr));
        return 1;
    }
    rt_destroy(c);
    auto same = [&](const RenderKernel::TemporalFrame& t, const std::vector<float>& o, const std::vector<float>& s,
                    const std::vector<float>& l, const std::vector<float>& nd) {
        return std::memcmp(t.rgba.data(), o.data(), n * 16) == 0 && std::memcmp(t.sigma.data(), s.data(), n * 4) == 0 &&
               std::memcmp(t.length.data(), l.data(), n * 4) == 0 && std::memcmp(t.normal_depth.data(), nd.data(), n * 16) == 0;
    };
    const bool first = same(t0, o0, s0, l0, nd0), second = same(t1, o1, s1, l1, nd1);
    size_t two = 0;
    for (float v : t1.length) two += v == 2.0f;
    const bool accumulated = two > n / 2 && std::memcmp(t1.rgba.data(), f1.data(), n * 16) != 0;
    bool bad_size = false;
    try {
        rk.temporal_accumulate(f1, std::vector<float>(n - 1), cam0);
    } catch (const std::runtime_error&) {
        bad_size = true;
    }
    std::printf("TEMPORAL_SHIM first %d second %d accumulated %d bad_size_throws %d\n", first ? 1 : 0, second ? 1 : 0,
                accumulated ? 1 : 0, bad_size ? 1 : 0);
    return first && second && accumulated && bad_size ? 0 : 1;
}
