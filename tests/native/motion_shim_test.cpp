// motion_shim_test.cpp — the drop-in's RenderKernel::motion_vectors and RenderKernel::motion_blur
// (include/render_kernel_hip.h) against the C ABI called directly: a Cornell linear render of few samples and its
// first-hit guides; the drop-in's vectors equal rt_motion_vectors' on the kernel's context and are zero but for
// rounding against the kernel's own camera; the drop-in's frame and reach equal rt_motion_blur's on a bare context
// (the blur needs no scene), bit for bit, at the defaults and with an open shutter and longer streaks, with the reach
// and without.
//   motion_shim_test <obj> <sky.raw | -> W H bounces
#include <cmath>

#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]);
    shim::Scene scene(argv[1], argv[2]);
    const size_t n = (size_t)W * H;

    Image frame(W, H);
    RenderKernel rk = scene.kernel(W, H, 2, nb, frame);
    Camera cam = Camera::CORNELL_BOX_CAMERA;
    rk.set_camera(cam);
    rk.render_linear();
    std::vector<float> albedo(n * 4), nd(n * 4);
    if (shim::c_abi_failed(rt_render_features(rk.context(), W, H, albedo.data(), nd.data()))) return 1;

    // the previous frame's camera: the same one moved to the right and up
    Camera prev = cam;
    prev.view_matrix.m[0][3] += 0.2f;
    prev.view_matrix.m[1][3] += 0.1f;
    const std::vector<float> mv = rk.motion_vectors(nd, W, H, prev);
    std::vector<float> mv_c(n * 2);
    if (shim::c_abi_failed(rt_motion_vectors(rk.context(), W, H, nd.data(), &prev.view_matrix.m[0][0], prev.fov_dist, mv_c.data()))) return 1;
    const bool vectors = shim::same_bits(mv, mv_c);
    const std::vector<float> mv_same = rk.motion_vectors(nd, W, H, cam);
    float largest = 0.0f, moved = 0.0f;
    for (size_t i = 0; i < 2 * n; i++) largest = std::fmax(largest, std::fabs(mv_same[i])), moved = std::fmax(moved, std::fabs(mv[i]));
    const bool still = largest < 1e-3f;

    rt_motion_params def, open;
    rt_motion_default_params(&def);
    open = def;
    open.shutter = 1.0f, open.max_radius = 16;
    std::vector<float> r_def, r_open;
    const Image c_def = rk.motion_blur(frame, nd, mv, nullptr, &r_def);
    const Image c_open = rk.motion_blur(frame, nd, mv, &open, &r_open);
    const Image c_none = rk.motion_blur(frame, nd, mv);

    rt_context* c = nullptr;
    int rc = rt_create(0, &c);
    std::vector<float> o0(n * 4), r0(n), o1(n * 4), r1(n), o2(n * 4);
    rc = rc ? rc : rt_motion_blur(c, W, H, frame.data(), nd.data(), mv.data(), &def, o0.data(), r0.data());
    rc = rc ? rc : rt_motion_blur(c, W, H, frame.data(), nd.data(), mv.data(), &open, o1.data(), r1.data());
    rc = rc ? rc : rt_motion_blur(c, W, H, frame.data(), nd.data(), mv.data(), nullptr, o2.data(), nullptr);
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);
    const bool defaults = shim::same_bits(c_def, o0) && shim::same_bits(r_def, r0);
    const bool params = shim::same_bits(c_open, o1) && shim::same_bits(r_open, r1) && !shim::same_bits(c_open, c_def);
    const bool no_reach = shim::same_bits(c_none, o2) && shim::same_bits(c_none, c_def);
    float reach = 0.0f;
    for (size_t i = 0; i < n; i++) reach = std::fmax(reach, r_open[i]);
    const bool something_moved = moved > 1.0f && reach > 0.5f && !shim::same_bits(c_open, frame);
    rt_motion_params bad = def;
    bad.max_radius = 17;
    const bool bad_radius = shim::throws([&] { rk.motion_blur(frame, nd, mv, &bad); });
    bad = def, bad.shutter = 1.5f;
    const bool bad_shutter = shim::throws([&] { rk.motion_blur(frame, nd, mv, &bad); });
    const bool bad_size = shim::throws([&] { rk.motion_blur(frame, nd, std::vector<float>(n)); });
    return shim::verdict("MOTION_SHIM", {{"vectors", vectors}, {"still_camera", still}, {"defaults", defaults}, {"params", params},
                                         {"no_reach", no_reach}, {"something_moved", something_moved},
                                         {"bad_max_radius_throws", bad_radius}, {"bad_shutter_throws", bad_shutter},
                                         {"bad_size_throws", bad_size}});
}
