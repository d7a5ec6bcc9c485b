// display_shim_test.cpp — the drop-in's RenderKernel::render_linear, display and write_image_hdr
// (include/render_kernel_hip.h) against its own render(): Cornell, display(render_linear()) at
// the defaults equals render()'s Image on the same base bit for bit, the linear Image keeps the
// base's alpha and differs from the displayed one, another exposure gives another image, and the
// .hdr file of the linear frame reads back to that frame within the format's truncation.
//   display_shim_test <obj> <sky.raw | -> W H bounces <out.hdr>
#include <algorithm>
#include <cmath>

#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]), spp = 6;
    shim::Scene scene(argv[1], argv[2]);
    Camera cam = Camera::CORNELL_BOX_CAMERA;

    Image whole(W, H), linear(W, H);
    for (int i = 0; i < W * H; i++)  // a base that is not the default
        whole[i] = linear[i] = Color((float)(i % 7) / 16.0f, (float)(i % 5) / 8.0f, 0.125f, 0.25f);

    RenderKernel rk = scene.kernel(W, H, spp, nb, whole);
    rk.set_camera(cam);
    rk.render();

    RenderKernel rl = scene.kernel(W, H, spp, nb, linear);
    rl.set_camera(cam);
    rl.render_linear();
    bool alpha = true;
    for (int i = 0; i < W * H; i++) alpha = alpha && linear.data()[4 * i + 3] == 0.25f;
    const Image shown = rl.display(linear);
    const bool same = shown.width() == W && shown.height() == H && shim::same_bits(shown, whole);
    const bool differs = !shim::same_bits(linear, whole);
    const bool exposure = !shim::same_bits(rl.display(linear, 0.5f, 2.2f), whole);
    const bool explicit_same = shim::same_bits(rl.display(linear, 1.5f, 2.2f), whole);

    // the .hdr file of the linear frame read back (rt_read_hdr; both flips default on and cancel): every
    // channel within the format's truncation, 0 <= written - read < 2^(e - 8), e the frexp exponent
    // of the pixel's largest channel
    bool hdr = RenderKernel::write_image_hdr(linear, argv[6]);
    int rw = 0, rh = 0;
    hdr = hdr && rt_read_hdr(argv[6], 1, &rw, &rh, nullptr) == RT_OK && rw == W && rh == H;
    if (hdr) {
        std::vector<float> back((size_t)W * H * 4);
        hdr = rt_read_hdr(argv[6], 1, &rw, &rh, back.data()) == RT_OK;
        float top = 0.0f;
        for (int i = 0; hdr && i < W * H; i++) {
            const float* a = linear.data() + 4 * (size_t)i;
            const float m = std::max(a[0], std::max(a[1], a[2]));
            int e = 0;
            std::frexp(m, &e);
            const double bound = std::ldexp(1.0, e - 8);
            for (int ch = 0; ch < 3; ch++) {
                const double d = (double)a[ch] - (double)back[4 * (size_t)i + ch];
                hdr = hdr && a[ch] >= 0.0f && d >= 0.0 && (m < 1e-32f || d < bound);
            }
            top = std::max(top, m);
        }
        hdr = hdr && top > 0.0f;
    }

    return shim::verdict("DISPLAY_SHIM", {{"round_trip", same}, {"alpha", alpha}, {"linear_differs", differs},
                                          {"exposure", exposure}, {"explicit", explicit_same}, {"hdr", hdr}});
}
