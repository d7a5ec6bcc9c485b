// rt_denoise.h — the post stage (include/rt_hip.h rt_render_features / rt_denoise): the
// per-pixel arithmetic of the first-hit feature pass and of the edge-avoiding à-trous
// filter (Dammertz et al. 2010), written once for the gfx950 kernels (rt_denoise.hip) and
// the CPU build of the same code (rt_hostsim.cpp). Both are compiled with -ffp-contract=off
// and use rt_libm's expf, so the two builds give the same bits.
//
// The filter, pass i of `passes` (step s = 1 << i, guides fixed across passes): for pixel p
// and each tap (dy, dx) in {-2..2}^2, dy outer, q = p + s (dx, dy) inside the image:
//   k = h[dy+2] h[dx+2]                      h = {1/16, 1/4, 3/8, 1/4, 1/16}
//   e = |c_p - c_q|^2 / sc_i^2               sc_i = sigma_color 2^-i (rgb of the pass's input)
//     + |n_p - n_q|^2 / sn^2 + |a_p - a_q|^2 / sa^2
//     + ((t_p - t_q) / max(t_p, t_q))^2 / st^2    both hit (t > 0); 0: both miss;
//                                                 one hit, one miss: the tap is skipped
//   w = k expf(-e);  out_p = sum w c_q / sum w     in tap order
// A tap whose colour is not finite is skipped; a centre that is not finite passes through.
// The four 1 / sigma^2 are computed once on the host (dn_inv_sigma2) and multiplied in.
#pragma once

#include "rt_wave.h"

namespace rtk {

// ------------------------------------------------------------ feature pass
// The frame's camera constants (set_view_consts' operations) for camera_ray_at.
struct CamView {
    RtCamera cam;
    float cam_o[3];
    float aspect;
    int W, H;
};

RT_HD CamView cam_view(const RtCamera& cam, int w, int h)
{
    CamView V;
    V.cam = cam;
    const V3 o = xform_point(cam, v3(0.0f, 0.0f, 0.0f));
    V.cam_o[0] = o.x;
    V.cam_o[1] = o.y;
    V.cam_o[2] = o.z;
    V.aspect = (float)w / (float)h;
    V.W = w;
    V.H = h;
    return V;
}

// The ray through the centre of pixel (x, y)'s jitter window: the reference jitters
// x_j = (x + 0.5) + r - 1, r in [0, 1) (render_kernel.cpp:88-89), so the centre is x_j = x.
RT_HD void feature_ray(const CamView& V, int x, int y, V3& o, V3& d)
{
    camera_ray_at(V.cam, V.cam_o, V.aspect, V.W, V.H, (float)x, (float)y, o, d);
}

// First hit of pixel (x, y), as rt_intersect answers that ray (query_closest + hit_from):
// normal_depth = {n, t}, albedo = {diffuse of materials[material_indices[prim]], 0};
// a miss is {0, 0, 0, -1} and {0, 0, 0, 0}.
RT_HD void feature_pixel(const RtSceneView& S, const CamView& V, int x, int y, StackEnt* stack, float4_& nd,
                         float4_& alb)
{
    V3 o, d;
    feature_ray(V, x, y, o, d);
    float t;
    int k;
    query_closest(S, o, d, stack, t, k, nullptr);
    Hit h;
    if (hit_from(S, o, d, t, k, h)) {
        const RtMat m = S.mats[S.mat_idx[h.prim]];
        nd = float4_{h.n.x, h.n.y, h.n.z, h.t};
        alb = float4_{m.dr, m.dg, m.db, 0.0f};
    } else {
        nd = float4_{0.0f, 0.0f, 0.0f, -1.0f};
        alb = float4_{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

// ------------------------------------------------------------------ filter
struct DnPass {
    int w, h, step;
    float inv_c, inv_n, inv_a, inv_t;  // 1 / sigma^2 of this pass (dn_inv_sigma2)
    const float4_* in;                 // the pass's input colour
    const float4_* nd;                 // guides (both null: the colour-only filter)
    const float4_* alb;
};

// 1 / sigma^2 as a float kept inside the normal range, so that 0 x it is 0 (the centre
// tap's e) and a finite difference x it is never NaN, whatever the sigma.
inline float dn_inv_sigma2(double sigma)
{
    const double v = 1.0 / (sigma * sigma);
    return v > 3.4028234663852886e38 ? 3.4028234663852886e38f : v < 1.1754943508222875e-38 ? 1.1754943508222875e-38f : (float)v;
}

RT_HD bool dn_finite3(const float4_& c)
{
    return (rt_asuint(c.x) & 0x7f800000u) != 0x7f800000u && (rt_asuint(c.y) & 0x7f800000u) != 0x7f800000u &&
           (rt_asuint(c.z) & 0x7f800000u) != 0x7f800000u;
}

RT_HD float dn_dist2(const float4_& a, const float4_& b)
{
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return dx * dx + dy * dy + dz * dz;
}

// The B3-spline kernel h = {1/16, 1/4, 3/8, 1/4, 1/16} at offset d = -2..2.
RT_HD float dn_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// Pixel reads straight from the pass's buffers (the hostsim loop, the direct kernel).
struct DnDirect {
    const DnPass& P;
    RT_HD float4_ color(int x, int y) const { return P.in[(size_t)y * P.w + x]; }
    RT_HD float4_ nd(int x, int y) const { return P.nd[(size_t)y * P.w + x]; }
    RT_HD float4_ alb(int x, int y) const { return P.alb[(size_t)y * P.w + x]; }
};

// One output pixel of one pass. F says where a pixel's records are read from (DnDirect, or
// the LDS tile of rt_denoise.hip); it is asked only for pixels inside the image. The sums
// run in tap order whatever F does. Alpha is carried through.
template <class F>
RT_HD float4_ dn_filter_pixel(const DnPass& P, int x, int y, const F& f)
{
    const float4_ cp = f.color(x, y);
    if (!dn_finite3(cp)) return cp;
    const bool guides = P.nd != nullptr;
    float4_ np = float4_{0, 0, 0, 0}, ap = float4_{0, 0, 0, 0};
    if (guides) {
        np = f.nd(x, y);
        ap = f.alb(x, y);
    }
    const bool hit_p = np.w > 0.0f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * P.step;
        if (qy < 0 || qy >= P.h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * P.step;
            if (qx < 0 || qx >= P.w) continue;
            const float4_ cq = f.color(qx, qy);
            if (!dn_finite3(cq)) continue;
            float e = dn_dist2(cp, cq) * P.inv_c;
            if (guides) {
                const float4_ nq = f.nd(qx, qy);
                const float4_ aq = f.alb(qx, qy);
                const bool hit_q = nq.w > 0.0f;
                if (hit_p != hit_q) continue;
                e = e + dn_dist2(np, nq) * P.inv_n;
                e = e + dn_dist2(ap, aq) * P.inv_a;
                if (hit_p) {
                    const float r = (np.w - nq.w) / rt_max(np.w, nq.w);
                    e = e + (r * r) * P.inv_t;
                }
            }
            if (!(e >= 0.0f)) continue;  // (NaN guides: no weight)
            const float wgt = (dn_h(dy) * dn_h(dx)) * rt_expf(-e);
            sr = sr + wgt * cq.x;
            sg = sg + wgt * cq.y;
            sb = sb + wgt * cq.z;
            sw = sw + wgt;
        }
    }
    if (!(sw > 0.0f)) return cp;  // (only with NaN guides at p: the centre tap has e = 0 otherwise)
    return float4_{sr / sw, sg / sw, sb / sw, cp.w};
}

// After the last pass, as Utils::OIDN_denoise blends (utils.cpp:184-186):
// rgb = blend filtered + (1 - blend) input, alpha 1.
RT_HD float4_ dn_blend(const float4_& f, const float4_& in, float blend)
{
    const float k = 1.0f - blend;
    return float4_{blend * f.x + k * in.x, blend * f.y + k * in.y, blend * f.z + k * in.z, 1.0f};
}

}  // namespace rtk
