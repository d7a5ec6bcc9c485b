// meter_shim_test.cpp — the drop-in's RenderKernel::meter and RenderKernel::auto_exposure
// (include/render_kernel_hip.h) against the C ABI called directly: a Cornell linear render of few
// samples with a NaN, a negative and a very bright pixel planted; the drop-in's histogram equals
// rt_meter's on a bare context (the stage needs no scene) word for word, and its exposure equals
// rt_meter_solve's on that histogram, at the defaults and with parameters, a previous exposure
// and a time step.
//   meter_shim_test <obj> <sky.raw | -> W H bounces
#include <limits>

#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]);
    shim::Scene scene(argv[1], argv[2]);

    Image frame(W, H);
    RenderKernel rk = scene.kernel(W, H, 2, nb, frame);
    rk.set_camera(Camera::CORNELL_BOX_CAMERA);
    rk.render_linear();
    frame[0] = Color(std::numeric_limits<float>::quiet_NaN(), 0.5f, 0.5f, 1.0f);
    frame[1] = Color(-1.0f, -2.0f, -0.5f, 1.0f);
    frame[(size_t)(H / 2) * W + W / 2] = Color(9000.0f, 8000.0f, 7000.0f, 1.0f);
    Image black(5, 3, Color(0.0f, 0.0f, 0.0f, 1.0f));

    rt_meter_params slow;
    rt_meter_default_params(&slow);
    slow.key = 0.3f, slow.low = 0.2f, slow.tau_up = 2.0f, slow.tau_down = 0.5f;
    const rt_meter_hist h_shim = rk.meter(frame), h_black = rk.meter(black);
    rt_meter_result r_def, r_slow, r_black;
    const float e_def = rk.auto_exposure(frame, 0.0f, 0.0f, nullptr, &r_def);
    const float e_slow = rk.auto_exposure(frame, 40.0f, 0.25f, &slow, &r_slow);
    const float e_black = rk.auto_exposure(black, 0.75f, 0.25f, nullptr, &r_black);

    rt_context* c = nullptr;
    int rc = rt_create(0, &c);
    rt_meter_hist h0, h1;
    rt_meter_result s_def, s_slow, s_black;
    rc = rc ? rc : rt_meter(c, W, H, frame.data(), &h0);
    rc = rc ? rc : rt_meter(c, 5, 3, black.data(), &h1);
    rc = rc ? rc : rt_meter_solve(&h0, nullptr, 0.0f, 0.0f, &s_def);
    rc = rc ? rc : rt_meter_solve(&h0, &slow, 40.0f, 0.25f, &s_slow);
    rc = rc ? rc : rt_meter_solve(&h1, nullptr, 0.75f, 0.25f, &s_black);
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);
    auto same = [](const rt_meter_result& a, const rt_meter_result& b) { return std::memcmp(&a, &b, sizeof a) == 0; };
    const bool hist = std::memcmp(&h_shim, &h0, sizeof h0) == 0 && std::memcmp(&h_black, &h1, sizeof h1) == 0;
    const bool counts = h0.nonfinite == 1 && h0.nonpositive >= 1 && h0.counted + h0.nonpositive + h0.nonfinite == (unsigned)(W * H) &&
                        h1.counted == 0 && h1.nonpositive == 15;
    const bool defaults = same(r_def, s_def) && e_def == s_def.exposure && s_def.valid == 1 && e_def == s_def.target;
    const bool params = same(r_slow, s_slow) && e_slow == s_slow.exposure && e_slow != s_slow.target && e_slow != e_def;
    const bool empty = same(r_black, s_black) && e_black == 0.75f && s_black.valid == 0;
    const bool bad_params = shim::throws([&] {
        rt_meter_params bad = slow;
        bad.key = 1.5f;
        rk.auto_exposure(frame, 0.0f, 0.0f, &bad);
    });
    std::printf("METER_SHIM hist %d counts %d defaults %d params %d empty %d bad_params_throw %d exposure %.9g\n", hist ? 1 : 0,
                counts ? 1 : 0, defaults ? 1 : 0, params ? 1 : 0, empty ? 1 : 0, bad_params ? 1 : 0, (double)e_def);
    return hist && counts && defaults && params && empty && bad_params ? 0 : 1;
}
