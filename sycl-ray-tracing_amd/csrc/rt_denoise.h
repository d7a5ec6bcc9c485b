// rt_denoise.h — the post stage (include/rt_hip.h rt_render_features / rt_denoise): the
// per-pixel arithmetic of the first-hit feature pass and of the edge-avoiding à-trous
// filter (Dammertz et al. 2010), written once for the gfx950 kernels (rt_denoise.hip) and
// the CPU build of the same code (rt_hostsim.cpp). Both are compiled with -ffp-contract=off
// and use rt_libm's expf, so the two builds give the same bits.
//
// The filter is one template, dn_filter_pixel<M>; rt_denoise takes it with M = DnFixed, the
// variance-guided rt_denoise_var (rt_dnv.h) with M = DnVar. What the two share, pass i of
// `passes` (step s = 1 << i, guides fixed across passes): for pixel p and each tap (dy, dx)
// in {-2..2}^2, dy outer, q = p + s (dx, dy) inside the image:
//   k = h[dy+2] h[dx+2]                      h = {1/16, 1/4, 3/8, 1/4, 1/16}
//   e = |c_p - c_q|^2 r_p                    r_p: the mode's colour scale (rgb of the pass's input)
//     + |n_p - n_q|^2 / sn^2 + |a_p - a_q|^2 / sa^2
//     + ((t_p - t_q) / max(t_p, t_q))^2 / st^2    both hit (t > 0); 0: both miss;
//                                                 one hit, one miss: the tap is skipped
//   w = k expf(-e);  out_p = sum w c_q / sum w     in tap order
// A tap whose colour is not finite is skipped, as is one whose e is NaN (a NaN guide); a centre
// that is not finite, or one left without a tap (a NaN guide at p), passes through.
// The four 1 / sigma^2 are computed once on the host (dn_inv_sigma2) and multiplied in.
// DnFixed: r_p = 1 / sc_i^2, sc_i = sigma_color 2^-i; alpha is carried through.
// DnVar: r_p from the variance around p, and a fourth output channel: rt_dnv.h.
#pragma once

#include <cmath>

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
constexpr float DNV_VMAX = 3.4028234663852886e38f;  // the largest finite float

struct DnPass {
    int w, h, step;
    float inv_c, inv_n, inv_a, inv_t;  // 1 / sigma^2 of this pass (dn_inv_sigma2)
    float var_floor;                   // (DnVar only)
    const float4_* in;                 // the pass's input: colour, or DnVar's records {r, g, b, v}
    const float4_* nd;                 // guides (both null: no guide terms)
    const float4_* alb;
};

// 1 / sigma^2 as a float kept inside the normal range, so that 0 x it is 0 (the centre
// tap's e) and a finite difference x it is never NaN, whatever the sigma.
inline float dn_inv_sigma2(double sigma)
{
    const double v = 1.0 / (sigma * sigma);
    return v > 3.4028234663852886e38 ? 3.4028234663852886e38f : v < 1.1754943508222875e-38 ? 1.1754943508222875e-38f : (float)v;
}

// Pass i of a call but for its three buffers: step 1 << i and the four 1 / sigma^2.
inline DnPass dn_pass(int w, int h, int i, double sigma_color, float sigma_normal, float sigma_albedo, float sigma_depth,
                      float var_floor)
{
    return DnPass{w, h, 1 << i, dn_inv_sigma2(sigma_color), dn_inv_sigma2(sigma_normal), dn_inv_sigma2(sigma_albedo),
                  dn_inv_sigma2(sigma_depth), var_floor, nullptr, nullptr, nullptr};
}
inline DnPass dn_pass(int w, int h, int i, const rt_denoise_params& p)  // (sigma_color halves with every pass)
{
    return dn_pass(w, h, i, std::ldexp((double)p.sigma_color, -i), p.sigma_normal, p.sigma_albedo, p.sigma_depth, 0.0f);
}
inline DnPass dn_pass(int w, int h, int i, const rt_denoise_var_params& p)  // (the same in every pass)
{
    return dn_pass(w, h, i, p.sigma_color, p.sigma_normal, p.sigma_albedo, p.sigma_depth, p.var_floor);
}

// The passes of one call: pass i reads what pass i - 1 wrote (the first: `first`) and writes pp[(i + o) & 1]
// (the last: out). run(P, dst, last) does one pass; a return other than 0 ends the call with it.
template <class Params, class Run>
int dn_run_passes(int w, int h, const Params& p, const float4_* first, float4_* const (&pp)[2], int o, float4_* out,
                  const float4_* nd, const float4_* alb, Run run)
{
    const float4_* src = first;
    for (int i = 0; i < p.passes; i++) {
        const bool last = i + 1 == p.passes;
        DnPass P = dn_pass(w, h, i, p);
        P.in = src, P.nd = nd, P.alb = alb;
        float4_* dst = last ? out : pp[(i + o) & 1];
        if (int r = run(P, dst, last)) return r;
        src = dst;
    }
    return 0;
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

// Pixel reads straight from the pass's buffers (the hostsim loop, the direct kernels).
struct DnDirect {
    const DnPass& P;
    RT_HD float4_ color(int x, int y) const { return P.in[(size_t)y * P.w + x]; }
    RT_HD float var(int x, int y) const { return P.in[(size_t)y * P.w + x].w; }
    RT_HD float4_ nd(int x, int y) const { return P.nd[(size_t)y * P.w + x]; }
    RT_HD float4_ alb(int x, int y) const { return P.alb[(size_t)y * P.w + x]; }
};

// rt_denoise's mode: the pass's own colour scale, three sums, alpha carried through.
struct DnFixed {
    static constexpr bool variance = false;
    template <class F>
    RT_HD static float color_scale(const DnPass& P, int, int, const F&)
    {
        return P.inv_c;
    }
};

// One output pixel of one pass in mode M (DnFixed, or rt_dnv.h's DnVar). F says where a pixel's
// records are read from (DnDirect, or the LDS tile of rt_atrous_hip.h); it is asked only for
// pixels inside the image. The sums run in tap order whatever F does.
template <class M, class F>
RT_HD float4_ dn_filter_pixel(const DnPass& P, int x, int y, const F& f)
{
    const float4_ cp = f.color(x, y);
    if (!dn_finite3(cp)) return cp;
    const float rp = M::color_scale(P, x, y, f);
    const bool guides = P.nd != nullptr;
    float4_ np = float4_{0, 0, 0, 0}, ap = float4_{0, 0, 0, 0};
    if (guides) {
        np = f.nd(x, y);
        ap = f.alb(x, y);
    }
    const bool hit_p = np.w > 0.0f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
    [[maybe_unused]] float sv = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * P.step;
        if (qy < 0 || qy >= P.h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * P.step;
            if (qx < 0 || qx >= P.w) continue;
            const float4_ cq = f.color(qx, qy);
            if (!dn_finite3(cq)) continue;
            float e = dn_dist2(cp, cq) * rp;
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
            if (!(e >= 0.0f)) continue;  // (NaN guides, DnVar's overflowed distance x 0: no weight)
            const float wgt = (dn_h(dy) * dn_h(dx)) * rt_expf(-e);
            sr = sr + wgt * cq.x;
            sg = sg + wgt * cq.y;
            sb = sb + wgt * cq.z;
            sw = sw + wgt;
            // (not (w w) v: w w is denormal from w = 1e-19 down, where v may be 1e38)
            if constexpr (M::variance) sv = sv + wgt * (wgt * cq.w);
        }
    }
    if (!(sw > 0.0f)) return cp;  // (only with NaN guides at p: the centre tap has e = 0 otherwise)
    if constexpr (M::variance) return float4_{sr / sw, sg / sw, sb / sw, rt_min(sv / (sw * sw), DNV_VMAX)};
    else return float4_{sr / sw, sg / sw, sb / sw, cp.w};
}

// After the last pass, as Utils::OIDN_denoise blends (utils.cpp:184-186):
// rgb = blend filtered + (1 - blend) input, alpha 1.
RT_HD float4_ dn_blend(const float4_& f, const float4_& in, float blend)
{
    const float k = 1.0f - blend;
    return float4_{blend * f.x + k * in.x, blend * f.y + k * in.y, blend * f.z + k * in.z, 1.0f};
}

// The end of a pass for pixel q: the filter's output for the next pass, or (orig != null: the last
// pass) the blend with the caller's input and, where asked for, DnVar's sigma_out = sqrt(out.v).
RT_HD void dn_store(const float4_& f, size_t q, float4_* __restrict__ out, const float4_* __restrict__ orig, float blend,
                    float* __restrict__ sigma_out)
{
    if (!orig) {
        out[q] = f;
        return;
    }
    out[q] = dn_blend(f, orig[q], blend);
    if (sigma_out) sigma_out[q] = rt_sqrtf(f.w);
}

}  // namespace rtk
