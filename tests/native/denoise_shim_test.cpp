// denoise_shim_test.cpp — the drop-in's RenderKernel::denoise (include/render_kernel_hip.h,
// the call shape of Utils::OIDN_denoise) against the C ABI called directly: the same scene
// bound to a second context through rt_set_scene / rt_build_bvh / rt_set_camera,
// rt_render_features + rt_denoise with the default parameters on the frame the drop-in rendered.
//   denoise_shim_test <obj> <sky.raw | -> W H spp bounces
#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), spp = std::atoi(argv[5]), nb = std::atoi(argv[6]);
    shim::Scene scene(argv[1], argv[2]);
    Camera cam = Camera::CORNELL_BOX_CAMERA;

    Image fb(W, H);
    RenderKernel rk = scene.kernel(W, H, spp, nb, fb);
    rk.set_camera(cam);
    rk.render();
    const Image d1 = rk.denoise(fb, 1.0f), d075 = rk.denoise(fb, 0.75f);

    int rc = 0;
    rt_context* c = scene.c_context(rc);
    rc = rc ? rc : rt_set_camera(c, &cam.view_matrix.m[0][0], cam.fov_dist);
    std::vector<float> alb((size_t)W * H * 4), nd(alb.size()), o1(alb.size()), o075(alb.size());
    rc = rc ? rc : rt_render_features(c, W, H, alb.data(), nd.data());
    rc = rc ? rc : rt_denoise(c, W, H, fb.data(), alb.data(), nd.data(), nullptr, 1.0f, o1.data());
    rc = rc ? rc : rt_denoise(c, W, H, fb.data(), alb.data(), nd.data(), nullptr, 0.75f, o075.data());
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);
    bool alpha = true;
    for (int i = 0; i < W * H; i++) alpha = alpha && d075.data()[4 * i + 3] == 1.0f;
    return shim::verdict("DENOISE_SHIM", {{"blend1", shim::same_bits(d1, o1)}, {"blend075", shim::same_bits(d075, o075)},
                                          {"filtered", !shim::same_bits(d1, fb)}, {"alpha", alpha}});
}
