// gbuffer_shim_test.cpp — the drop-in's RenderKernel::gbuffer (include/render_kernel_hip.h, over
// rt_render_gbuffer) against the C calls made directly on a second context bound to the same scene
// under the Cornell camera: the two guide images against rt_render_features, with and without
// exact, and the ids against words 0 and 1 of rt_query(RT_QUERY_CLOSEST) on rt_camera_rays and the
// scene's material indices.
//   gbuffer_shim_test <obj> W H
#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    shim::Scene scene(argv[1]);  // (no sky: the guides need none)
    Image fb(W, H);
    Camera cam = Camera::CORNELL_BOX_CAMERA;
    RenderKernel rk = scene.kernel(W, H, 1, 1, fb);
    rk.set_camera(cam);

    int rc = 0;
    rt_context* c = scene.c_context(rc);
    rc = rc ? rc : rt_set_camera(c, &cam.view_matrix.m[0][0], cam.fov_dist);
    const size_t n = (size_t)W * H;
    std::vector<float> r(n * 6), want_alb(n * 4), want_nd(n * 4);
    std::vector<int> rec(n * 11);
    rc = rc ? rc : rt_camera_rays(c, W, H, r.data());
    rc = rc ? rc : rt_query(c, RT_QUERY_CLOSEST, r.data(), (long)n, rec.data());
    rc = rc ? rc : rt_render_features(c, W, H, want_alb.data(), want_nd.data());
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);

    Image alb, nd, alb_x, nd_x;
    std::vector<int> ids, ids_x;
    rk.gbuffer(alb, nd, &ids);
    rk.gbuffer(alb_x, nd_x, &ids_x, true);
    const bool walks = shim::same_bits(alb, want_alb.data()) && shim::same_bits(nd, want_nd.data());
    const bool exact = shim::same_bits(alb_x, want_alb.data()) && shim::same_bits(nd_x, want_nd.data());
    bool id_ok = ids.size() == 2 * n && ids == ids_x;
    size_t found = 0;
    for (size_t i = 0; i < n && id_ok; i++) {
        const int* w = &rec[11 * i];
        if (!w[0]) {
            id_ok = ids[2 * i] == -1 && ids[2 * i + 1] == -1;
            continue;
        }
        found++;
        id_ok = ids[2 * i] == w[1] && ids[2 * i + 1] == scene.obj.material_indices[(size_t)w[1]];
    }
    Image alb2, nd2;
    rk.gbuffer(alb2, nd2);  // (no ids)
    const bool no_ids = shim::same_bits(alb2, alb) && shim::same_bits(nd2, nd);
    const bool some = found > n / 2;  // (the Cornell camera looks into the box)
    return shim::verdict("GBUFFER_SHIM", {{"walks", walks}, {"exact", exact}, {"ids", id_ok}, {"no_ids", no_ids}, {"hits", some}});
}
