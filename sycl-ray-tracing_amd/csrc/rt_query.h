// rt_query.h — the batched ray queries (include/rt_hip.h rt_query / rt_query_device): what
// the gfx950 kernels (rt_query.hip) and the CPU build (rt_hostsim.cpp) share, the answer
// records and the routing rule.
//
// Routing, the render's own policy (k_trace):
//   * a query whose origin lies outside the near box (rt_fast.h far_origin) takes the exact
//     walk (query_closest: the octree walk or the brute-force loop, then the sphere loop);
//   * every other query takes the search-BVH walk (gfx950: a quad of lanes, rt_quad.h;
//     hostsim: the one-lane walks of rt_fast.h); a walk that does not settle (a tie, a failed
//     chain check, an overflow of the bounded stack) hands its query to the exact walk;
//   * a context with spheres, or in rt_set_intersect_mode(0), and a call with RT_QUERY_EXACT
//     send every query to the exact walk.
// Either walk's (t, k) goes through rq_closest_record, k_intersect's record.
#pragma once

#include "rt_wave.h"

namespace rtk {

#define RQ_WORDS 11  // int32 words of a closest-hit record (rt_intersect's)

// rt_intersect's record of a closest-hit answer (t, k): {found, primitive, t, point, normal,
// u = v = -1}; point and normal are zeros when there is no answer at all (t == -1).
RT_HD void rq_closest_record(const RtSceneView& S, V3 o, V3 d, float t, int k, int32_t* ot)
{
    Hit h;
    const bool f = hit_from(S, o, d, t, k, h);
    ot[0] = f ? 1 : 0;
    ot[1] = h.prim;
    ot[2] = (int32_t)rt_asuint(t);
    const bool any = t != -1.0f;
    ot[3] = any ? (int32_t)rt_asuint(h.p.x) : 0;
    ot[4] = any ? (int32_t)rt_asuint(h.p.y) : 0;
    ot[5] = any ? (int32_t)rt_asuint(h.p.z) : 0;
    ot[6] = any ? (int32_t)rt_asuint(h.n.x) : 0;
    ot[7] = any ? (int32_t)rt_asuint(h.n.y) : 0;
    ot[8] = any ? (int32_t)rt_asuint(h.n.z) : 0;
    ot[9] = (int32_t)rt_asuint(-1.0f);
    ot[10] = (int32_t)rt_asuint(-1.0f);
}

// The exact walk's answer for query i of rays[n][6]: the closest record, or its `found` word.
RT_HD void rq_exact(const RtSceneView& S, const float* rays, size_t i, bool any, StackEnt* stack, int32_t* out)
{
    const float* r = rays + 6 * i;
    const V3 o = v3(r[0], r[1], r[2]), d = v3(r[3], r[4], r[5]);
    float t;
    int k;
    query_closest(S, o, d, stack, t, k, nullptr);
    if (any)
        out[i] = t > 0.0f ? 1 : 0;  // (hit_from's `found`)
    else
        rq_closest_record(S, o, d, t, k, out + RQ_WORDS * i);
}

}  // namespace rtk
