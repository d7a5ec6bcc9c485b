// progress_shim_test.cpp — the drop-in's RenderKernel::render_progressive
// (include/render_kernel_hip.h) against its own render(): Cornell in passes of 2 samples, the
// callback sees done = 2, 4, 6 of 6, and the final Image equals render()'s on an Image holding
// the same base, bit for bit; a callback that returns false stops after its pass.
//   progress_shim_test <obj> <sky.raw | -> W H bounces
#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), nb = std::atoi(argv[5]), spp = 6;
    shim::Scene scene(argv[1], argv[2]);
    Camera cam = Camera::CORNELL_BOX_CAMERA;

    Image whole(W, H), passes(W, H), stopped(W, H);
    for (int i = 0; i < W * H; i++)  // a base that is not the default
        whole[i] = passes[i] = stopped[i] = Color((float)(i % 7) / 16.0f, (float)(i % 5) / 8.0f, 0.125f, 0.25f);

    RenderKernel rk = scene.kernel(W, H, spp, nb, whole);
    rk.set_camera(cam);
    rk.render();

    RenderKernel rp = scene.kernel(W, H, spp, nb, passes);
    rp.set_camera(cam);
    std::vector<int> seen;
    bool image_ok = true, preview_differs = false;
    rp.render_progressive(2, [&](const Image& img, int done, int total) {
        seen.push_back(done);
        image_ok = image_ok && &img == &passes && total == spp;
        if (done < total) preview_differs = preview_differs || !shim::same_bits(img, whole);
        return true;
    });
    const bool calls = seen == std::vector<int>{2, 4, 6};

    RenderKernel rs = scene.kernel(W, H, spp, nb, stopped);
    rs.set_camera(cam);
    int stop_calls = 0;
    rs.render_progressive(4, [&](const Image&, int done, int) {
        stop_calls++;
        return done != 4;  // stop after the first pass
    });
    rs.render();  // the context renders on as usual afterwards (on the preview as its base)

    return shim::verdict("PROGRESS_SHIM", {{"calls", calls}, {"image", image_ok}, {"preview_differs", preview_differs},
                                           {"final", shim::same_bits(passes, whole)}, {"stopped", stop_calls == 1}});
}
