// progress_shim_test.cpp — the drop-in's RenderKernel::render_progressive
// (include/render_kernel_hip.h) against its own render(): Cornell in passes of 2 samples, the
// callback sees done = 2, 4, 6 of 6, and the final Image equals render()'s on an Image holding
// the same base, bit for bit; a callback that returns false stops after its pass. Built like
// shim_test (the reference's headers and objects; linked to the hostsim build, and to the product
// library for the GPU run); tests/test_progress_shim.py runs it.
//   progress_shim_test <obj> <sky.raw> W H bounces
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
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]), spp = 6;
    ParsedOBJ obj = Utils::parse_obj(argv[1]);
    BVH bvh(&obj.triangles);
    Image sky = read_sky_raw(argv[2]);
    std::vector<float> cdf = Utils::compute_env_map_cdf(sky);
    std::vector<Sphere> spheres;
    Camera cam = Camera::CORNELL_BOX_CAMERA;

    Image whole(W, H), passes(W, H), stopped(W, H);
    for (int i = 0; i < W * H; i++)  // a base that is not the default
        whole[i] = passes[i] = stopped[i] = Color((float)(i % 7) / 16.0f, (float)(i % 5) / 8.0f, 0.125f, 0.25f);
    size_t bytes = (size_t)W * H * 4 * sizeof(float);

    RenderKernel rk(W, H, spp, nb, whole, obj.triangles, obj.materials, obj.emissive_triangle_indices,
                    obj.material_indices, spheres, bvh, sky, cdf);
    rk.set_camera(cam);
    rk.render();

    RenderKernel rp(W, H, spp, nb, passes, obj.triangles, obj.materials, obj.emissive_triangle_indices,
                    obj.material_indices, spheres, bvh, sky, cdf);
    rp.set_camera(cam);
    std::vector<int> seen;
    bool image_ok = true, preview_differs = false;
    rp.render_progressive(2, [&](const Image& img, int done, int total) {
        seen.push_back(done);
        image_ok = image_ok && &img == &passes && total == spp;
        if (done < total) preview_differs = preview_differs || std::memcmp(img.data(), whole.data(), bytes) != 0;
        return true;
    });
    const bool calls = seen == std::vector<int>{2, 4, 6};
    const bool same = std::memcmp(passes.data(), whole.data(), bytes) == 0;

    RenderKernel rs(W, H, spp, nb, stopped, obj.triangles, obj.materials, obj.emissive_triangle_indices,
                    obj.material_indices, spheres, bvh, sky, cdf);
    rs.set_camera(cam);
    int stop_calls = 0;
    rs.render_progressive(4, [&](const Image&, int done, int) {
        stop_calls++;
        return done != 4;  // stop after the first pass
    });
    rs.render();  // the context renders on as usual afterwards (on the preview as its base)

    std::printf("PROGRESS_SHIM calls %d image %d preview_differs %d final %d stopped %d\n", calls ? 1 : 0,
                image_ok ? 1 : 0, preview_differs ? 1 : 0, same ? 1 : 0, stop_calls == 1 ? 1 : 0);
    return calls && image_ok && preview_differs && same && stop_calls == 1 ? 0 : 1;
}
