// display_shim_test.cpp — the drop-in's RenderKernel::render_linear, display and write_image_hdr
// (include/render_kernel_hip.h) against its own render(): Cornell, display(render_linear()) at
// the defaults equals render()'s Image on the same base bit for bit, the linear Image keeps the
// base's alpha and differs from the displayed one, another exposure gives another image, and the
// .hdr file of the linear frame reads back to that frame within the format's truncation. Built like shim_test (the
// reference's headers and objects; linked to the hostsim build, and to the product library for
// the GPU run); tests/test_display_shim.py runs it.
//   display_shim_test <obj> <sky.raw> W H bounces <out.hdr>
#include <algorithm>
#include <cmath>
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
    if (argc < 7) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]), spp = 6;
    ParsedOBJ obj = Utils::parse_obj(argv[1]);
    BVH bvh(&obj.triangles);
    Image sky = read_sky_raw(argv[2]);
    std::vector<float> cdf = Utils::compute_env_map_cdf(sky);
    std::vector<Sphere> spheres;
    Camera cam = Camera::CORNELL_BOX_CAMERA;

    Image whole(W, H), linear(W, H);
    for (int i = 0; i < W * H; i++)  // a base that is not the default
        whole[i] = linear[i] = Color((float)(i % 7) / 16.0f, (float)(i % 5) / 8.0f, 0.125f, 0.25f);
    const size_t bytes = (size_t)W * H * 4 * sizeof(float);

    RenderKernel rk(W, H, spp, nb, whole, obj.triangles, obj.materials, obj.emissive_triangle_indices,
                    obj.material_indices, spheres, bvh, sky, cdf);
    rk.set_camera(cam);
    rk.render();

    RenderKernel rl(W, H, spp, nb, linear, obj.triangles, obj.materials, obj.emissive_triangle_indices,
                    obj.material_indices, spheres, bvh, sky, cdf);
    rl.set_camera(cam);
    rl.render_linear();
    bool alpha = true;
    for (int i = 0; i < W * H; i++) alpha = alpha && linear.data()[4 * i + 3] == 0.25f;
    const Image shown = rl.display(linear);
    const bool same = shown.width() == W && shown.height() == H && std::memcmp(shown.data(), whole.data(), bytes) == 0;
    const bool differs = std::memcmp(linear.data(), whole.data(), bytes) != 0;
    const Image dark = rl.display(linear, 0.5f, 2.2f);
    const bool exposure = std::memcmp(dark.data(), whole.data(), bytes) != 0;
    const Image again = rl.display(linear, 1.5f, 2.2f);
    const bool explicit_same = std::memcmp(again.data(), whole.data(), bytes) == 0;

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

    std::printf("DISPLAY_SHIM round_trip %d alpha %d linear_differs %d exposure %d explicit %d hdr %d\n", same ? 1 : 0,
                alpha ? 1 : 0, differs ? 1 : 0, exposure ? 1 : 0, explicit_same ? 1 : 0, hdr ? 1 : 0);
    return same && alpha && differs && exposure && explicit_same && hdr ? 0 : 1;
}
