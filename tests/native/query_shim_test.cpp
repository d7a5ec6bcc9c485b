// query_shim_test.cpp — the drop-in's RenderKernel::query_closest / query_any
// (include/render_kernel_hip.h, over rt_query) against rt_intersect called directly on a
// second context bound to the same scene: the Cornell camera rays of a W x H frame
// (rt_camera_rays), every HitInfo field and every occlusion flag.
//   query_shim_test <obj> W H
#include "ray.h"
#include "shim_common.h"

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    shim::Scene scene(argv[1]);  // (no sky: the queries need none)
    Image fb(W, H);
    Camera cam = Camera::CORNELL_BOX_CAMERA;
    RenderKernel rk = scene.kernel(W, H, 1, 1, fb);
    rk.set_camera(cam);

    int rc = 0;
    rt_context* c = scene.c_context(rc);
    rc = rc ? rc : rt_set_camera(c, &cam.view_matrix.m[0][0], cam.fov_dist);
    const size_t n = (size_t)W * H;
    std::vector<float> r(n * 6);
    std::vector<int> want(n * 11);
    rc = rc ? rc : rt_camera_rays(c, W, H, r.data());
    rc = rc ? rc : rt_intersect(c, r.data(), (int)n, want.data());
    if (shim::c_abi_failed(rc)) return 1;
    rt_destroy(c);

    std::vector<Ray> rays;
    for (size_t i = 0; i < n; i++)
        rays.push_back(Ray(Point(r[6 * i], r[6 * i + 1], r[6 * i + 2]), Vector(r[6 * i + 3], r[6 * i + 4], r[6 * i + 5])));
    std::vector<HitInfo> hits;
    std::vector<char> occluded;
    rk.query_closest(rays, hits);
    rk.query_any(rays, occluded);
    bool closest = hits.size() == n, any = occluded.size() == n;
    size_t found = 0;
    for (size_t i = 0; i < n && closest && any; i++) {
        const int* w = &want[11 * i];
        any = any && occluded[i] == (w[0] ? 1 : 0);
        if (!w[0]) {
            closest = closest && hits[i].t == -1.0f && hits[i].primitive_index == -1;
            continue;
        }
        found++;
        const float f[7] = {hits[i].t,
                            hits[i].inter_point.x,
                            hits[i].inter_point.y,
                            hits[i].inter_point.z,
                            hits[i].normal_at_intersection.x,
                            hits[i].normal_at_intersection.y,
                            hits[i].normal_at_intersection.z};
        closest = closest && hits[i].primitive_index == w[1] && std::memcmp(f, w + 2, sizeof f) == 0;
    }
    const bool some = found > n / 2;  // (the Cornell camera looks into the box)
    return shim::verdict("QUERY_SHIM", {{"closest", closest}, {"any", any}, {"hits", some}});
}
