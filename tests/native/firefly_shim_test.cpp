// firefly_shim_test.cpp — the drop-in's RenderKernel::firefly_clamp (include/render_kernel_hip.h)
// against the C ABI called directly: a Cornell linear render of few samples with a synthetic sigma
// map and two planted spikes; the drop-in's colour, sigma_out and scale_out equal rt_firefly's on a
// bare context (the stage needs no scene), bit for bit, with a sigma and without, at the defaults
// and at radius 2 / rank 3.
//   firefly_shim_test <obj> <sky.raw | -> W H bounces
#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]);
    shim::Scene scene(argv[1], argv[2]);
    const size_t n = (size_t)W * H;
    std::vector<float> sigma(n);
    for (size_t i = 0; i < n; i++) sigma[i] = 0.05f + 0.01f * (float)(i % 17);

    Image frame(W, H);
    RenderKernel rk = scene.kernel(W, H, 2, nb, frame);
    rk.set_camera(Camera::CORNELL_BOX_CAMERA);
    rk.render_linear();
    frame[(size_t)(H / 2) * W + W / 2] = Color(80.0f, 70.0f, 60.0f, 1.0f);  // an interior spike ...
    frame[0] = Color(90.0f, 90.0f, 90.0f, 1.0f);                            // ... and one in a corner

    rt_firefly_params def, wide;
    rt_firefly_default_params(&def);
    wide = def;
    wide.radius = 2, wide.rank = 3, wide.gain = 1.5f, wide.floor = 0.01f;
    std::vector<float> s_def, f_def, s_wide, f_wide, f_none;
    const Image c_def = rk.firefly_clamp(frame, sigma, def, &s_def, &f_def);
    const Image c_wide = rk.firefly_clamp(frame, sigma, wide, &s_wide, &f_wide);
    const Image c_none = rk.firefly_clamp(frame, std::vector<float>(), def, nullptr, &f_none);

    rt_context* c = nullptr;
    int rc = rt_create(0, &c);
    std::vector<float> o0(n * 4), s0(n), f0(n), o1(n * 4), s1(n), f1(n), o2(n * 4), f2(n);
    rc = rc ? rc : rt_firefly(c, W, H, frame.data(), sigma.data(), nullptr, o0.data(), s0.data(), f0.data());
    rc = rc ? rc : rt_firefly(c, W, H, frame.data(), sigma.data(), &wide, o1.data(), s1.data(), f1.data());
    rc = rc ? rc : rt_firefly(c, W, H, frame.data(), nullptr, &def, o2.data(), nullptr, f2.data());
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);
    const bool defaults = shim::same_bits(c_def, o0) && shim::same_bits(s_def, s0) && shim::same_bits(f_def, f0);
    const bool params = shim::same_bits(c_wide, o1) && shim::same_bits(s_wide, s1) && shim::same_bits(f_wide, f1);
    const bool no_sigma = shim::same_bits(c_none, o2) && shim::same_bits(f_none, f2) && shim::same_bits(c_none, c_def);
    const bool clamped = f_def[(size_t)(H / 2) * W + W / 2] < 0.5f && f_def[0] < 0.5f && !shim::same_bits(c_def, frame);
    const bool bad_size = shim::throws([&] { rk.firefly_clamp(frame, std::vector<float>(n - 1), def); });
    const bool bad_out = shim::throws([&] {
        std::vector<float> s;
        rk.firefly_clamp(frame, std::vector<float>(), def, &s);
    });
    return shim::verdict("FIREFLY_SHIM", {{"defaults", defaults}, {"params", params}, {"no_sigma", no_sigma}, {"clamped", clamped},
                                          {"bad_size_throws", bad_size}, {"sigma_out_without_sigma_throws", bad_out}});
}
