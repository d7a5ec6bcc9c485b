// bloom_shim_test.cpp — the drop-in's RenderKernel::bloom (include/render_kernel_hip.h) against the C
// ABI called directly: a Cornell linear render of few samples with two planted bright pixels; the
// drop-in's frame and layer equal rt_bloom's on a bare context (the stage needs no scene), bit for
// bit, at the defaults and at three levels with a lower threshold, with the layer and without.
//   bloom_shim_test <obj> <sky.raw | -> W H bounces
#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]);
    shim::Scene scene(argv[1], argv[2]);
    const size_t n = (size_t)W * H;

    Image frame(W, H);
    RenderKernel rk = scene.kernel(W, H, 2, nb, frame);
    rk.set_camera(Camera::CORNELL_BOX_CAMERA);
    rk.render_linear();
    frame[(size_t)(H / 2) * W + W / 2] = Color(80.0f, 70.0f, 60.0f, 1.0f);  // a bright pixel inside ...
    frame[0] = Color(90.0f, 90.0f, 90.0f, 1.0f);                            // ... and one in a corner

    rt_bloom_params def, low;
    rt_bloom_default_params(&def);
    low = def;
    low.threshold = 0.5f, low.knee = 0.25f, low.intensity = 0.6f, low.levels = 3;
    std::vector<float> l_def, l_low;
    const Image c_def = rk.bloom(frame, nullptr, &l_def);
    const Image c_low = rk.bloom(frame, &low, &l_low);
    const Image c_none = rk.bloom(frame);

    rt_context* c = nullptr;
    int rc = rt_create(0, &c);
    std::vector<float> o0(n * 4), l0(n * 4), o1(n * 4), l1(n * 4), o2(n * 4);
    rc = rc ? rc : rt_bloom(c, W, H, frame.data(), &def, o0.data(), l0.data());
    rc = rc ? rc : rt_bloom(c, W, H, frame.data(), &low, o1.data(), l1.data());
    rc = rc ? rc : rt_bloom(c, W, H, frame.data(), nullptr, o2.data(), nullptr);
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);
    const bool defaults = shim::same_bits(c_def, o0) && shim::same_bits(l_def, l0);
    const bool params = shim::same_bits(c_low, o1) && shim::same_bits(l_low, l1) && !shim::same_bits(c_low, c_def);
    const bool no_layer = shim::same_bits(c_none, o2) && shim::same_bits(c_none, c_def);
    // the neighbour of the planted pixel got brighter, and the layer there is what was added
    const size_t q = (size_t)(H / 2) * W + W / 2 + 1;
    const bool glow = c_def[q].r > frame[q].r && l_def[4 * q] > 0.0f && l_def[4 * q + 3] == 0.0f && !shim::same_bits(c_def, frame);
    rt_bloom_params bad = def;
    bad.levels = 9;
    const bool bad_levels = shim::throws([&] { rk.bloom(frame, &bad); });
    bad = def, bad.knee = 2.0f;
    const bool bad_knee = shim::throws([&] { rk.bloom(frame, &bad); });
    return shim::verdict("BLOOM_SHIM", {{"defaults", defaults}, {"params", params}, {"no_layer", no_layer}, {"glow", glow},
                                        {"bad_levels_throw", bad_levels}, {"bad_knee_throws", bad_knee}});
}
