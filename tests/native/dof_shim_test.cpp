// dof_shim_test.cpp — the drop-in's RenderKernel::dof (include/render_kernel_hip.h) against the C ABI
// called directly: a Cornell linear render of few samples and its first-hit guides; the drop-in's frame
// and radius equal rt_dof's on a bare context (the stage needs no scene), bit for bit, at the defaults
// and with the focus on the centre pixel's hit and a wider lens, with the radius and without.
//   dof_shim_test <obj> <sky.raw | -> W H bounces
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
    std::vector<float> albedo(n * 4), nd(n * 4);
    if (shim::c_abi_failed(rt_render_features(rk.context(), W, H, albedo.data(), nd.data()))) return 1;
    const size_t centre = (size_t)(H / 2) * W + W / 2;

    rt_dof_params def, lens;
    rt_dof_default_params(&def);
    lens = def;
    lens.focus = nd[4 * centre + 3] > 0.0f ? nd[4 * centre + 3] : 2.0f, lens.coc_inf = 9.0f, lens.max_radius = 12;
    std::vector<float> r_def, r_lens;
    const Image c_def = rk.dof(frame, nd, nullptr, &r_def);
    const Image c_lens = rk.dof(frame, nd, &lens, &r_lens);
    const Image c_none = rk.dof(frame, nd);

    rt_context* c = nullptr;
    int rc = rt_create(0, &c);
    std::vector<float> o0(n * 4), r0(n), o1(n * 4), r1(n), o2(n * 4);
    rc = rc ? rc : rt_dof(c, W, H, frame.data(), nd.data(), &def, o0.data(), r0.data());
    rc = rc ? rc : rt_dof(c, W, H, frame.data(), nd.data(), &lens, o1.data(), r1.data());
    rc = rc ? rc : rt_dof(c, W, H, frame.data(), nd.data(), nullptr, o2.data(), nullptr);
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);
    const bool defaults = shim::same_bits(c_def, o0) && shim::same_bits(r_def, r0);
    const bool params = shim::same_bits(c_lens, o1) && shim::same_bits(r_lens, r1) && !shim::same_bits(c_lens, c_def);
    const bool no_coc = shim::same_bits(c_none, o2) && shim::same_bits(c_none, c_def);
    // a pixel off the focus distance has a radius and changed; the centre pixel, focused on, has none
    size_t q = n;
    for (size_t i = 0; i < n && q == n; i++)
        if (r_lens[i] > 1.0f) q = i;
    const bool background = q < n && r_lens[centre] == 0.0f && !shim::same_bits(c_lens, frame) &&
                            (c_lens[q].r != frame[q].r || c_lens[q].g != frame[q].g || c_lens[q].b != frame[q].b);
    rt_dof_params bad = def;
    bad.max_radius = 13;
    const bool bad_radius = shim::throws([&] { rk.dof(frame, nd, &bad); });
    bad = def, bad.focus = 0.0f;
    const bool bad_focus = shim::throws([&] { rk.dof(frame, nd, &bad); });
    return shim::verdict("DOF_SHIM", {{"defaults", defaults}, {"params", params}, {"no_coc", no_coc}, {"background_changed", background},
                                      {"bad_max_radius_throws", bad_radius}, {"bad_focus_throws", bad_focus}});
}
