// noise_shim_test.cpp — the drop-in's RenderKernel::progress_track_noise / progress_noise and
// render_progressive_tracked (include/render_kernel_hip.h) against the C ABI: Cornell, 6 samples in
// passes of 2. The callback queries the noise from the second pass on and the struct equals what
// rt_progress_noise reports on the kernel's context at that point, whose tile map's largest value is
// the struct's max_tile; a query after one pass throws; the tracked frame is render()'s Image bit for
// bit; a threshold above the first max_tile stops the passes after the second.
//   noise_shim_test <obj> <sky.raw | -> W H bounces
#include "shim_common.h"

static bool same(const rt_noise_stats& a, const rt_noise_stats& b)
{
    return std::memcmp(&a.max_tile, &b.max_tile, 4) == 0 && a.tiles == b.tiles && a.tiles_over == b.tiles_over &&
           a.nonfinite == b.nonfinite && a.samples_a == b.samples_a && a.samples_b == b.samples_b && a.passes == b.passes;
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]), spp = 6;
    const float threshold = 0.05f;
    shim::Scene scene(argv[1], argv[2]);
    Camera cam = Camera::CORNELL_BOX_CAMERA;

    Image whole(W, H), tracked(W, H), early(W, H);
    RenderKernel rk = scene.kernel(W, H, spp, nb, whole);
    rk.set_camera(cam);
    rk.render();

    RenderKernel rt = scene.kernel(W, H, spp, nb, tracked);
    rt.set_camera(cam);
    std::vector<rt_noise_stats> got, want;
    bool threw = false, max_ok = true;
    const int n_tiles = ((W + 7) / 8) * ((H + 7) / 8);
    std::vector<float> tiles((size_t)n_tiles), px((size_t)W * H);
    rt.render_progressive_tracked(2, [&](const Image&, int done, int) {
        rt_noise_stats st;
        if (done == 2) {
            threw = shim::throws([&] { rt.progress_noise(threshold, st); });  // (one pass only)
            return true;
        }
        rt.progress_noise(threshold, st);
        got.push_back(st);
        rt_noise_stats c_st;  // the C ABI on the same context, with the maps
        if (rt_progress_noise(rt.context(), threshold, &c_st, px.data(), tiles.data()) != RT_OK) return false;
        want.push_back(c_st);
        float top = 0.0f;
        for (float t : tiles) top = t > top ? t : top;
        max_ok = max_ok && top == c_st.max_tile;
        return true;
    });
    const bool frame = shim::same_bits(tracked, whole);

    bool agree = got.size() == 2 && want.size() == 2;
    for (size_t i = 0; agree && i < got.size(); i++) agree = same(got[i], want[i]);
    const bool sane = agree && max_ok && got[0].tiles == ((W + 7) / 8) * ((H + 7) / 8) && got[0].samples_a == 2 &&
                      got[0].samples_b == 2 && got[0].passes == 2 && got[1].samples_a == 4 && got[1].samples_b == 2 &&
                      got[1].passes == 3 && got[0].nonfinite == 0 && got[0].max_tile > 0.0f;

    // a threshold above the first max_tile: the callback stops after the second pass
    RenderKernel re = scene.kernel(W, H, spp, nb, early);
    re.set_camera(cam);
    int calls = 0, stopped_at = 0;
    re.render_progressive_tracked(2, [&](const Image&, int done, int) {
        calls++;
        if (done < 4) return true;
        rt_noise_stats st;
        re.progress_noise(sane ? got[0].max_tile * 2.0f + 1.0f : 1e30f, st);
        stopped_at = done;
        return st.tiles_over != 0;
    });
    const bool stops = calls == 2 && stopped_at == 4;

    // an untracked render_progressive leaves the progression untracked: the query throws
    bool untracked = false;
    re.render_progressive(3, [&](const Image&, int done, int) {
        rt_noise_stats st;
        if (done == 6) untracked = shim::throws([&] { re.progress_noise(threshold, st); });
        return true;
    });

    return shim::verdict("NOISE_SHIM", {{"frame", frame}, {"one_pass_throws", threw}, {"agree", agree}, {"sane", sane},
                                        {"stops", stops}, {"untracked_throws", untracked}});
}
