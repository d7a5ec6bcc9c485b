// upscale_shim_test.cpp — the drop-in's RenderKernel::upscale (include/render_kernel_hip.h) against
// the C ABI called directly: a Cornell linear render of few samples at half the size, with a NaN
// pixel planted, and a synthetic sigma map; the drop-in's frame and sigma equal rt_upscale's on a
// bare context (the stage needs no scene) fed with rt_render_features' guides at both sizes, bit
// for bit, at the defaults with a sigma and with parameters without one; the wrong sizes throw.
// Built like shim_test (the reference's headers and objects, linked to the hostsim build of the C
// ABI); tests/test_upscale_shim.py runs it, and make sanitize-upscale builds it with ASan and UBSan
// over the hostsim sources and runs it.
//   upscale_shim_test <obj> <sky.raw | -> W H bounces      (-: a flat grey sky of 8 x 4 texels)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "image.h"
#include "utils.h"
#include "render_kernel_hip.h"

static Image read_sky_raw(const char* path)  // int w, h; float rgb[h][w][3]
{
    if (std::strcmp(path, "-") == 0) {
        Image flat(8, 4);
        for (int i = 0; i < 32; i++) flat[i] = Color(0.5f, 0.5f, 0.5f, 0.0f);
        return flat;
    }
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
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]);
    const int WL = (W + 1) / 2, HL = (H + 1) / 2;
    ParsedOBJ obj = Utils::parse_obj(argv[1]);
    BVH bvh(&obj.triangles);
    Image sky = read_sky_raw(argv[2]);
    std::vector<float> cdf = Utils::compute_env_map_cdf(sky);
    std::vector<Sphere> spheres;

    Image low(WL, HL);
    RenderKernel rk(WL, HL, 2, nb, low, obj.triangles, obj.materials, obj.emissive_triangle_indices, obj.material_indices,
                    spheres, bvh, sky, cdf);
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
    if (rc) {
        std::printf("C ABI failed: %d %s\n", rc, rt_last_error(nullptr));
        return 1;
    }
    rt_destroy(c);
    const bool frame = std::memcmp(up_def.data(), c_def.data(), n * 16) == 0 && up_def.width() == W && up_def.height() == H;
    const bool sig = s_shim.size() == n && std::memcmp(s_shim.data(), s_c.data(), n * 4) == 0;
    const bool params = std::memcmp(up_par.data(), c_par.data(), n * 16) == 0 && std::memcmp(up_par.data(), up_def.data(), n * 16) != 0;
    bool finite = true;  // (the NaN pixel and the infinite sigma are rebuilt from their neighbours)
    for (size_t i = 0; i < n; i++) finite = finite && std::isfinite(up_def[i].r) && std::isfinite(s_shim[i]) && up_def[i].a == 1.0f;
    int thrown = 0;
    try {
        rk.upscale(low, WL - 1, H);
    } catch (const std::runtime_error&) {
        thrown++;
    }
    try {
        rk.upscale(low, W, H, std::vector<float>(3, 0.1f), nullptr, &s_shim);
    } catch (const std::runtime_error&) {
        thrown++;
    }
    try {
        rk.upscale(low, W, H, sigma);
    } catch (const std::runtime_error&) {
        thrown++;
    }
    try {
        rt_upscale_params bad = tight;
        bad.min_weight = 1.0f;
        rk.upscale(low, W, H, &bad);
    } catch (const std::runtime_error&) {
        thrown++;
    }
    std::printf("UPSCALE_SHIM frame %d sigma %d params %d finite %d bad_arguments_throw %d\n", frame ? 1 : 0, sig ? 1 : 0,
                params ? 1 : 0, finite ? 1 : 0, thrown);
    return frame && sig && params && finite && thrown == 4 ? 0 : 1;
}
