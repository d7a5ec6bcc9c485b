// upscale_shim_test.cpp — the drop-in's RenderKernel::upscale (include/render_kernel_hip.h) against
// the C ABI called directly: a Cornell linear render of few samples at half the size, with a NaN
// pixel planted, and a synthetic sigma map; the drop-in's frame and sigma equal rt_upscale's on a
// bare context (the stage needs no scene) fed with rt_render_features' guides at both sizes, bit
// for bit, at the defaults with a sigma and with parameters without one; the wrong sizes throw.
//   upscale_shim_test <obj> <sky.raw | -> W H bounces
#include <cmath>
#include <limits>

#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]);
    const int WL = (W + 1) / 2, HL = (H + 1) / 2;
    shim::Scene scene(argv[1], argv[2]);

    Image low(WL, HL);
    RenderKernel rk = scene.kernel(WL, HL, 2, nb, low);
    rk.set_camera(Camera::CORNELL_BOX_CAMERA);
    rk.render_linear();
    low[1] = Color(std::numeric_limits<float>::quiet_NaN(), 0.5f, 0.5f, 1.0f);
    const size_t n_lo = (size_t)WL * HL, n = (size_t)W * H;
    std::vector<float> sigma(n_lo), s_shim;
    for (size_t i = 0; i < n_lo; i++) sigma[i] = 0.05f + 0.001f * (float)(i % 97);
    sigma[2] = std::numeric_limits<float>::infinity();

    rt_upscale_params tight;
    rt_upscale_default_params(&tight);
    tight.sigma_normal = 0.2f, tight.sigma_depth = 0.05f, tight.min_weight = 0.3f;
    const Image up_def = rk.upscale(low, W, H, sigma, nullptr, &s_shim);
    const Image up_par = rk.upscale(low, W, H, &tight);

    std::vector<float> alb_lo(n_lo * 4), nd_lo(n_lo * 4), alb_hi(n * 4), nd_hi(n * 4), s_c(n);
    Image c_def(W, H), c_par(W, H);
    rt_context* c = nullptr;
    int rc = rt_create(0, &c);
    rc = rc ? rc : rt_render_features(rk.context(), WL, HL, alb_lo.data(), nd_lo.data());
    rc = rc ? rc : rt_render_features(rk.context(), W, H, alb_hi.data(), nd_hi.data());
    rc = rc ? rc : rt_upscale(c, WL, HL, W, H, low.data(), sigma.data(), alb_lo.data(), nd_lo.data(), alb_hi.data(), nd_hi.data(),
                              nullptr, c_def.data(), s_c.data());
    rc = rc ? rc : rt_upscale(c, WL, HL, W, H, low.data(), nullptr, alb_lo.data(), nd_lo.data(), alb_hi.data(), nd_hi.data(),
                              &tight, c_par.data(), nullptr);
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);
    const bool frame = up_def.width() == W && up_def.height() == H && shim::same_bits(up_def, c_def);
    const bool sig = shim::same_bits(s_shim, s_c);
    const bool params = shim::same_bits(up_par, c_par) && !shim::same_bits(up_par, up_def);
    bool finite = true;  // (the NaN pixel and the infinite sigma are rebuilt from their neighbours)
    for (size_t i = 0; i < n; i++) finite = finite && std::isfinite(up_def[i].r) && std::isfinite(s_shim[i]) && up_def[i].a == 1.0f;
    rt_upscale_params bad = tight;
    bad.min_weight = 1.0f;
    int thrown = shim::throws([&] { rk.upscale(low, WL - 1, H); });
    thrown += shim::throws([&] { rk.upscale(low, W, H, std::vector<float>(3, 0.1f), nullptr, &s_shim); });
    thrown += shim::throws([&] { rk.upscale(low, W, H, sigma); });
    thrown += shim::throws([&] { rk.upscale(low, W, H, &bad); });
    std::printf("UPSCALE_SHIM frame %d sigma %d params %d finite %d bad_arguments_throw %d\n", frame ? 1 : 0, sig ? 1 : 0,
                params ? 1 : 0, finite ? 1 : 0, thrown);
    return frame && sig && params && finite && thrown == 4 ? 0 : 1;
}
