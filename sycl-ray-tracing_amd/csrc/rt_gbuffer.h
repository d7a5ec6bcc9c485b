// rt_gbuffer.h — the first-hit G-buffer on the render's walks (include/rt_hip.h rt_render_gbuffer /
// rt_render_gbuffer_device): what the gfx950 kernels (rt_gbuffer.hip) and the CPU build
// (rt_hostsim.cpp) share, the records of a pixel and the stressor's rule.
//
// A pixel's ray is feature_ray's (rt_denoise.h), its routing rt_query's (rt_query.h, stated there
// once): far_origin pixels, sphere contexts, rt_set_intersect_mode(0) and RT_GBUFFER_EXACT take the
// exact walk, every other pixel the search-BVH walk with the exact walk behind it. Either walk's
// (t, k) goes through gb_record, which is feature_pixel's rule (hit_from, then the material of the
// primitive) and so what rq_closest_record's words 1, 2 and 6..8 hold for that ray.
#pragma once

#include "rt_denoise.h"
#include "rt_query.h"

namespace rtk {

// The three records of a pixel: normal_depth = {n, t}, albedo = {diffuse, 0} and
// ids = {primitive, material_indices[primitive]}; a miss is {0, 0, 0, -1}, zeros and {-1, -1}.
struct GbRecord {
    float4_ nd, alb;
    int32_t prim, mat;
};

RT_HD GbRecord gb_record(const RtSceneView& S, V3 o, V3 d, float t, int k)
{
    GbRecord r;
    Hit h;
    if (hit_from(S, o, d, t, k, h)) {
        r.prim = h.prim;
        r.mat = S.mat_idx[h.prim];
        const RtMat m = S.mats[r.mat];
        r.nd = float4_{h.n.x, h.n.y, h.n.z, h.t};
        r.alb = float4_{m.dr, m.dg, m.db, 0.0f};
    } else {
        r.prim = r.mat = -1;
        r.nd = float4_{0.0f, 0.0f, 0.0f, -1.0f};
        r.alb = float4_{0.0f, 0.0f, 0.0f, 0.0f};
    }
    return r;
}

// Pixel i's ray: feature_ray of (i mod W, i / W).
RT_HD void gb_ray(const CamView& V, int i, V3& o, V3& d)
{
    const int y = i / V.W, x = i - y * V.W;
    feature_ray(V, x, y, o, d);
}

// The stressor (rt_test_schedule "gb_force_every" = N): pixels with i mod N == 0 skip the search-BVH
// walk for the exact walk. 0: off.
RT_HD bool gb_forced(int every, int i) { return every > 0 && i % every == 0; }

// Pixel i on one lane (the hostsim build): feature_ray, rt_query's hostsim routing
// (fast_query_closest tests far_origin itself), then the record. *exact: the exact walk answered.
template <class STK>
RT_HD GbRecord gb_pixel(const RtSceneView& S, const CamView& V, int i, bool all_exact, int force_every, StackEnt* stack,
                        STK& fst, bool* exact)
{
    V3 o, d;
    gb_ray(V, i, o, d);
    float t;
    int k;
    const bool settled = !all_exact && !gb_forced(force_every, i) && fast_query_closest(S, o, d, fst, t, k, nullptr);
    if (!settled) query_closest(S, o, d, stack, t, k, nullptr);
    *exact = !settled;
    return gb_record(S, o, d, t, k);
}

}  // namespace rtk
