// firefly_shim_test.cpp — the drop-in's RenderKernel::firefly_clamp (include/render_kernel_hip.h)
// against the C ABI called directly: a Cornell linear render of few samples with a synthetic sigma
// map and two planted spikes; the drop-in's colour, sigma_out and scale_out equal rt_firefly's on a
// bare context (the stage needs no scene), bit for bit, with a sigma and without, at the defaults
// and at radius 2 / rank 3. Built like shim_test (the reference's headers and objects, linked to the
// hostsim build of the C ABI); tests/test_firefly_shim.py runs it, and make sanitize-firefly builds
// it with ASan and UBSan over the hostsim sources.
//   firefly_shim_test <obj> <sky.raw> W H bounces
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
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]);
    ParsedOBJ obj = Utils::parse_obj(argv[1]);
    BVH bvh(&obj.triangles);
    Image sky = read_sky_raw(argv[2]);
    std::vector<float> cdf = Utils::compute_env_map_cdf(sky);
    std::vector<Sphere> spheres;
    const size_t n = (size_t)W * H;
    std::vector<float> sigma(n);
    for (size_t i = 0; i < n; i++) sigma[i] = 0.05f + 0.01f * (float)(i % 17);

    Image frame(W, H);
    RenderKernel rk(W, H, 2, nb, frame, obj.triangles, obj.materials, obj.emissive_triangle_indices, obj.material_indices,
                    spheres, bvh, sky, cdf);
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
    if (rc) {
        std::printf("C ABI failed: %d %s\n", rc, rt_last_error(nullptr));
        return 1;
    }
    rt_destroy(c);
    auto same = [&](const Image& img, const std::vector<float>& o, const std::vector<float>* s, const std::vector<float>* sw,
                    const std::vector<float>& f, const std::vector<float>& fw) {
        return std::memcmp(img.data(), o.data(), n * 16) == 0 && (!s || std::memcmp(s->data(), sw->data(), n * 4) == 0) &&
               std::memcmp(f.data(), fw.data(), n * 4) == 0;
    };
    const bool defaults = same(c_def, o0, &s_def, &s0, f_def, f0), params = same(c_wide, o1, &s_wide, &s1, f_wide, f1);
    const bool no_sigma = same(c_none, o2, nullptr, nullptr, f_none, f2) && std::memcmp(c_none.data(), c_def.data(), n * 16) == 0;
    const bool clamped = f_def[(size_t)(H / 2) * W + W / 2] < 0.5f && f_def[0] < 0.5f &&
                         std::memcmp(c_def.data(), frame.data(), n * 16) != 0;
    bool bad_size = false, bad_out = false;
    try {
        rk.firefly_clamp(frame, std::vector<float>(n - 1), def);
    } catch (const std::runtime_error&) {
        bad_size = true;
    }
    try {
        std::vector<float> s;
        rk.firefly_clamp(frame, std::vector<float>(), def, &s);
    } catch (const std::runtime_error&) {
        bad_out = true;
    }
    std::printf("FIREFLY_SHIM defaults %d params %d no_sigma %d clamped %d bad_size_throws %d sigma_out_without_sigma_throws %d\n",
                defaults ? 1 : 0, params ? 1 : 0, no_sigma ? 1 : 0, clamped ? 1 : 0, bad_size ? 1 : 0, bad_out ? 1 : 0);
    return defaults && params && no_sigma && clamped && bad_size && bad_out ? 0 : 1;
}
