// dnv_shim_test.cpp — the drop-in's RenderKernel::denoise_var and progress_noise_sigma
// (include/render_kernel_hip.h) against the C ABI called directly: Cornell, a tracked
// progression of 4 samples in passes of 2; in the second pass's callback the drop-in's sigma
// equals rt_progress_noise_sigma on the kernel's context and the linear frame is resolved; the
// drop-in's denoise_var of that frame then equals rt_render_features + rt_denoise_var with the
// default parameters on a second context bound to the same scene, colour and sigma_out, bit for
// bit.
//   dnv_shim_test <obj> <sky.raw | -> W H bounces
#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]), spp = 4;
    shim::Scene scene(argv[1], argv[2]);
    Camera cam = Camera::CORNELL_BOX_CAMERA;
    const size_t n = (size_t)W * H;

    Image fb(W, H), linear(W, H);
    RenderKernel rk = scene.kernel(W, H, spp, nb, fb);
    rk.set_camera(cam);
    std::vector<float> sigma, c_sigma(n);
    bool one_pass_throws = false, sigma_same = false, resolved = false;
    rk.render_progressive_tracked(2, [&](const Image&, int done, int) {
        if (done == 2) {
            one_pass_throws = shim::throws([&] { rk.progress_noise_sigma(); });
            return true;
        }
        sigma = rk.progress_noise_sigma();
        sigma_same = rt_progress_noise_sigma(rk.context(), c_sigma.data()) == RT_OK && sigma.size() == n &&
                     shim::same_bits(sigma, c_sigma);
        resolved = rt_progress_resolve_linear(rk.context(), linear.data()) == RT_OK;
        return true;
    });
    if (sigma.size() != n) {
        std::printf("DNV_SHIM no sigma\n");
        return 1;
    }
    std::vector<float> left1, left075;
    const Image d1 = rk.denoise_var(linear, sigma, 1.0f, &left1), d075 = rk.denoise_var(linear, sigma, 0.75f);

    int rc = 0;
    rt_context* c = scene.c_context(rc);
    rc = rc ? rc : rt_set_camera(c, &cam.view_matrix.m[0][0], cam.fov_dist);
    std::vector<float> alb(n * 4), nd(n * 4), o1(n * 4), o075(n * 4), l1(n);
    rc = rc ? rc : rt_render_features(c, W, H, alb.data(), nd.data());
    rc = rc ? rc : rt_denoise_var(c, W, H, linear.data(), sigma.data(), alb.data(), nd.data(), nullptr, 1.0f, o1.data(), l1.data());
    rc = rc ? rc : rt_denoise_var(c, W, H, linear.data(), sigma.data(), alb.data(), nd.data(), nullptr, 0.75f, o075.data(), nullptr);
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);
    const bool left = left1.size() == n && shim::same_bits(left1, l1);
    const bool bad_size = shim::throws([&] { rk.denoise_var(linear, std::vector<float>(n - 1), 1.0f); });
    return shim::verdict("DNV_SHIM", {{"one_pass_throws", one_pass_throws}, {"sigma", sigma_same}, {"resolved", resolved},
                                      {"blend1", shim::same_bits(d1, o1)}, {"blend075", shim::same_bits(d075, o075)},
                                      {"sigma_out", left}, {"filtered", !shim::same_bits(d1, linear)},
                                      {"bad_size_throws", bad_size}});
}
