// temporal_shim_test.cpp — the drop-in's RenderKernel::temporal_accumulate
// (include/render_kernel_hip.h) against the C ABI called directly: Cornell, two frames under a moved
// camera, each a linear render with a synthetic sigma map; the drop-in's first frame (no history)
// and second frame (the first as its history) equal rt_render_features + rt_temporal_accumulate
// with the default parameters on a second context bound to the same scene, colour, sigma and
// length, bit for bit.
//   temporal_shim_test <obj> <sky.raw | -> W H bounces
#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]);
    shim::Scene scene(argv[1], argv[2]);
    Camera cam0 = Camera::CORNELL_BOX_CAMERA, cam1 = Camera::CORNELL_BOX_CAMERA;
    cam1.view_matrix.m[0][3] += 0.05f;
    cam1.view_matrix.m[1][3] += 0.02f;
    const size_t n = (size_t)W * H;
    std::vector<float> sigma(n);
    for (size_t i = 0; i < n; i++) sigma[i] = 0.05f + 0.01f * (float)(i % 17);

    // two linear frames of different sample totals (the seeding recipe's point: uncorrelated noise)
    Image f0(W, H), f1(W, H);
    RenderKernel rk0 = scene.kernel(W, H, 3, nb, f0);
    rk0.set_camera(cam0);
    rk0.render_linear();
    RenderKernel rk = scene.kernel(W, H, 4, nb, f1);
    rk.set_camera(cam1);
    rk.render_linear();
    rk.set_camera(cam0);
    const RenderKernel::TemporalFrame t0 = rk.temporal_accumulate(f0, sigma, cam0);
    rk.set_camera(cam1);
    const RenderKernel::TemporalFrame t1 = rk.temporal_accumulate(f1, sigma, cam0, &t0);

    int rc = 0;
    rt_context* c = scene.c_context(rc);
    std::vector<float> alb(n * 4), nd0(n * 4), nd1(n * 4), o0(n * 4), s0(n), l0(n), o1(n * 4), s1(n), l1(n);
    rc = rc ? rc : rt_set_camera(c, &cam0.view_matrix.m[0][0], cam0.fov_dist);
    rc = rc ? rc : rt_render_features(c, W, H, alb.data(), nd0.data());
    rc = rc ? rc : rt_temporal_accumulate(c, W, H, f0.data(), sigma.data(), nd0.data(), &cam0.view_matrix.m[0][0], cam0.fov_dist,
                                          nullptr, nullptr, nullptr, nullptr, nullptr, o0.data(), s0.data(), l0.data());
    rc = rc ? rc : rt_set_camera(c, &cam1.view_matrix.m[0][0], cam1.fov_dist);
    rc = rc ? rc : rt_render_features(c, W, H, alb.data(), nd1.data());
    rc = rc ? rc : rt_temporal_accumulate(c, W, H, f1.data(), sigma.data(), nd1.data(), &cam0.view_matrix.m[0][0], cam0.fov_dist,
                                          o0.data(), s0.data(), l0.data(), nd0.data(), nullptr, o1.data(), s1.data(), l1.data());
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);
    auto same = [](const RenderKernel::TemporalFrame& t, const std::vector<float>& o, const std::vector<float>& s,
                   const std::vector<float>& l, const std::vector<float>& nd) {
        return shim::same_bits(t.rgba, o) && shim::same_bits(t.sigma, s) && shim::same_bits(t.length, l) &&
               shim::same_bits(t.normal_depth, nd);
    };
    const bool first = same(t0, o0, s0, l0, nd0), second = same(t1, o1, s1, l1, nd1);
    size_t two = 0;
    for (float v : t1.length) two += v == 2.0f;
    const bool accumulated = two > n / 2 && !shim::same_bits(t1.rgba, f1);
    const bool bad_size = shim::throws([&] { rk.temporal_accumulate(f1, std::vector<float>(n - 1), cam0); });
    return shim::verdict("TEMPORAL_SHIM",
                         {{"first", first}, {"second", second}, {"accumulated", accumulated}, {"bad_size_throws", bad_size}});
}
