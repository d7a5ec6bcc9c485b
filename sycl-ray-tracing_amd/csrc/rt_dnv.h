// rt_dnv.h — the variance-guided post stage (include/rt_hip.h rt_progress_noise_sigma /
// rt_denoise_var): the per-pixel arithmetic of the absolute noise figure and of the à-trous
// filter whose colour edge-stop is scaled by the centre pixel's variance (Schied et al. 2017,
// SVGF's spatial half), written once for the gfx950 kernels (rt_dnv.hip) and the CPU build of
// the same code (rt_hostsim.cpp). Both are compiled with -ffp-contract=off, divide with IEEE
// division and take rt_libm's expf and rt_sqrtf, so the two builds give the same bits.
//
// The noise figure: s = k * d, rt_noise.h's noise_pixel stopped before its division (the same
// operations in the same order, restated here so that rt_noise.hip and rt_adapt.hip compile
// as they did), with the tile's own counts in an adaptive progression (adapt_tile_args).
//
// The filter. Prep: one 16-byte record {r, g, b, v} per pixel, v = s * s of the caller's
// sigma map, a NaN v replaced by 0 and an infinite one by the largest finite float, so v is
// finite from there on. Pass i of `passes` (step 1 << i, guides fixed), pixel p:
//   g_p = sum k v_q / sum k over the 3x3 at unit spacing around p inside the image,
//         k = b[dy+1] b[dx+1], b = {1/4, 1/2, 1/4}; every pixel inside the image counts,
//         whatever its colour; a sum that overflowed is the largest finite float
//   r_p = inv_c / (g_p + var_floor)           inv_c = dn_inv_sigma2(sigma_color), every pass
//   each tap q = p + step (dx, dy) as in dn_filter_pixel (its order and its skips), with
//   e = |c_p - c_q|^2 r_p + the three guide terms;  w = k expf(-e)
//   out.rgb = sum w c_q / sum w              out.v = sum w (w v_q) / (sum w  sum w)
//   (w (w v), not (w w) v: w w leaves the normal range from w = 1e-19 down, where v may be 1e38)
// Edge cases:
//   a centre whose colour is not finite     its record passes through, v included
//   no tap with weight (a NaN guide at p)   the same: the record passes through
//   a tap whose colour is not finite        skipped: no weight in the colour or in out.v
//   g_p + var_floor = +inf                  r_p = 0: the colour term drops out; a tap whose colour
//                                           distance overflowed then has e = NaN and is skipped
//   out.v                                   a quotient that rounded past the largest finite float is
//                                           that float (the centre tap has w = 9/64, so sum w >= 9/64)
// After the last pass dn_blend runs on the rgb and sigma_out, when asked for, is rt_sqrtf(out.v).
#pragma once

#include "rt_adapt.h"
#include "rt_denoise.h"

namespace rtk {

constexpr float DNV_VMAX = 3.4028234663852886e38f;  // the largest finite float

// ------------------------------------------------------------ noise figure
// k * d of rt_noise.h's noise_pixel: its operations up to the division.
RT_HD float dnv_noise_sigma(const float4_& state, const float4_& half, const NoiseArgs& A)
{
    const float mr = state.x / A.n_all, mg = state.y / A.n_all, mb = state.z / A.n_all;
    const float ar = half.x / A.n_a, ag = half.y / A.n_a, ab = half.z / A.n_a;
    const float d = (noise_abs(mr - ar) + noise_abs(mg - ag)) + noise_abs(mb - ab);
    return A.k * d;
}

// ------------------------------------------------------------------ filter
RT_HD float dnv_variance(float s)
{
    const float v = s * s;
    if (rt_isnan(v)) return 0.0f;
    return rt_min(v, DNV_VMAX);
}

RT_HD float4_ dnv_prep(const float4_& rgba, float s) { return float4_{rgba.x, rgba.y, rgba.z, dnv_variance(s)}; }

struct DnvPass {
    int w, h, step;
    float inv_c, inv_n, inv_a, inv_t;  // 1 / sigma^2 (dn_inv_sigma2), the same in every pass
    float var_floor;
    const float4_* in;                 // the pass's input records {r, g, b, v}
    const float4_* nd;                 // guides (both null: colour and variance only)
    const float4_* alb;
};

// Record reads straight from the pass's buffers (the hostsim loop, the direct kernel).
struct DnvDirect {
    const DnvPass& P;
    RT_HD float4_ color(int x, int y) const { return P.in[(size_t)y * P.w + x]; }
    RT_HD float var(int x, int y) const { return P.in[(size_t)y * P.w + x].w; }
    RT_HD float4_ nd(int x, int y) const { return P.nd[(size_t)y * P.w + x]; }
    RT_HD float4_ alb(int x, int y) const { return P.alb[(size_t)y * P.w + x]; }
};

// The binomial kernel b = {1/4, 1/2, 1/4} at offset d = -1..1.
RT_HD float dnv_b(int d) { return d == 0 ? 0.5f : 0.25f; }

// The 3x3 prefilter of the variance around (x, y), dy outer.
template <class F>
RT_HD float dnv_var3x3(const DnvPass& P, int x, int y, const F& f)
{
    float sv = 0.0f, sk = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= P.h) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= P.w) continue;
            const float k = dnv_b(dy) * dnv_b(dx);
            sv = sv + k * f.var(qx, qy);
            sk = sk + k;
        }
    }
    return rt_min(sv / sk, DNV_VMAX);
}

// One output record of one pass. F as for dn_filter_pixel (DnvDirect, or the LDS tile of
// rt_dnv.hip), asked only for pixels inside the image; the sums run in tap order whatever F does.
template <class F>
RT_HD float4_ dnv_filter_pixel(const DnvPass& P, int x, int y, const F& f)
{
    const float4_ cp = f.color(x, y);
    if (!dn_finite3(cp)) return cp;
    const float rp = P.inv_c / (dnv_var3x3(P, x, y, f) + P.var_floor);
    const bool guides = P.nd != nullptr;
    float4_ np = float4_{0, 0, 0, 0}, ap = float4_{0, 0, 0, 0};
    if (guides) {
        np = f.nd(x, y);
        ap = f.alb(x, y);
    }
    const bool hit_p = np.w > 0.0f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sv = 0.0f;
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
            if (!(e >= 0.0f)) continue;  // (NaN guides, an overflowed distance x 0: no weight)
            const float wgt = (dn_h(dy) * dn_h(dx)) * rt_expf(-e);
            sr = sr + wgt * cq.x;
            sg = sg + wgt * cq.y;
            sb = sb + wgt * cq.z;
            sw = sw + wgt;
            sv = sv + wgt * (wgt * cq.w);  // (not (w w) v: w w is denormal from w = 1e-19 down, where v may be 1e38)
        }
    }
    if (!(sw > 0.0f)) return cp;
    return float4_{sr / sw, sg / sw, sb / sw, rt_min(sv / (sw * sw), DNV_VMAX)};
}

}  // namespace rtk
