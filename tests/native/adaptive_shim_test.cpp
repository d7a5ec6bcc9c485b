// adaptive_shim_test.cpp — the drop-in's RenderKernel::render_adaptive (include/render_kernel_hip.h)
// against the C ABI: Cornell, 8 samples in passes of 2. The threshold is the middle value of the tile
// map after two uniform passes, read through the C calls on a second kernel's context; the same
// passes made through the C calls on that context give the Image and the tile counts that
// render_adaptive returns, bit for bit, with both active and inactive tiles among them. At threshold 0
// every tile takes every pass: the counts are all 8 and the Image is render()'s. max_passes = 1 stops
// after one adaptive pass (counts 4 and 6).
//   adaptive_shim_test <obj> <sky.raw | -> W H bounces
#include <algorithm>

#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]), spp = 8, step = 2;
    shim::Scene scene(argv[1], argv[2]);
    Camera cam = Camera::CORNELL_BOX_CAMERA;
    const int n_tiles = ((W + 7) / 8) * ((H + 7) / 8);

    // the C calls, on the context of a kernel that has rendered (scene, BVH, env and camera bound)
    Image whole(W, H), blank(W, H);
    RenderKernel rc = scene.kernel(W, H, spp, nb, whole);
    rc.set_camera(cam);
    rc.render();
    rt_context* ctx = rc.context();
    std::vector<float> tiles((size_t)n_tiles), want_fb((size_t)W * H * 4);
    std::vector<int> want_n((size_t)n_tiles);
    rt_noise_stats st;
    bool c_ok = rt_progress_begin(ctx, W, H, spp, nb, blank.data(), 0, 1) == RT_OK && rt_progress_noise_track(ctx) == RT_OK &&
                rt_progress_advance(ctx, step, nullptr) == RT_OK && rt_progress_advance(ctx, step, nullptr) == RT_OK &&
                rt_progress_noise(ctx, 0.0f, &st, nullptr, tiles.data()) == RT_OK;
    std::vector<float> sorted = tiles;
    std::sort(sorted.begin(), sorted.end());
    const float threshold = sorted[sorted.size() / 2];
    int c_passes = 0;
    while (c_ok) {
        int info[8];
        c_ok = rt_progress_advance_adaptive(ctx, step, threshold, nullptr, info) == RT_OK;
        if (!c_ok || info[0] == 0) break;
        c_passes++;
    }
    c_ok = c_ok && rt_progress_resolve(ctx, want_fb.data()) == RT_OK &&
           rt_progress_tile_counts(ctx, want_n.data(), nullptr) == RT_OK;
    rt_progress_end(ctx);

    Image adaptive(W, H), full(W, H), one(W, H);
    RenderKernel ra = scene.kernel(W, H, spp, nb, adaptive);
    ra.set_camera(cam);
    const std::vector<int> got_n = ra.render_adaptive(threshold, step);
    const bool frame = c_ok && shim::same_bits(adaptive, want_fb);
    const bool counts = c_ok && got_n == want_n;
    const int lo = *std::min_element(got_n.begin(), got_n.end()), hi = *std::max_element(got_n.begin(), got_n.end());
    const bool mixed = c_passes >= 1 && lo == 2 * step && hi > lo && hi <= spp;

    RenderKernel rf = scene.kernel(W, H, spp, nb, full);
    rf.set_camera(cam);
    const std::vector<int> full_n = rf.render_adaptive(0.0f, step);
    const bool all = std::count(full_n.begin(), full_n.end(), spp) == n_tiles && shim::same_bits(full, whole);

    RenderKernel ro = scene.kernel(W, H, spp, nb, one);
    ro.set_camera(cam);
    const std::vector<int> one_n = ro.render_adaptive(threshold, step, 1);
    bool capped = (int)one_n.size() == n_tiles;
    for (size_t t = 0; capped && t < one_n.size(); t++) capped = one_n[t] == std::min(want_n[t], 3 * step);

    const bool throws = shim::throws([&] { ro.render_adaptive(-1.0f, step); });  // (a threshold the C ABI refuses)

    return shim::verdict("ADAPTIVE_SHIM", {{"frame", frame}, {"counts", counts}, {"mixed", mixed}, {"all", all},
                                           {"max_passes", capped}, {"throws", throws}});
}
