// rt_dnv.h — the variance-guided post stage (include/rt_hip.h rt_progress_noise_sigma /
// rt_denoise_var): the per-pixel arithmetic of the absolute noise figure and of the mode of
// rt_denoise.h's à-trous filter whose colour edge-stop is scaled by the centre pixel's variance
// (Schied et al. 2017, SVGF's spatial half), written once for the gfx950 kernels (rt_dnv.hip)
// and the CPU build of the same code (rt_hostsim.cpp). Both are compiled with -ffp-contract=off,
// divide with IEEE division and take rt_libm's expf and rt_sqrtf, so the two builds give the same bits.
//
// The noise figure: s = k * d, rt_noise.h's noise_pixel stopped before its division (the same
// operations in the same order, a function of its own so that rt_noise.hip and rt_adapt.hip
// compile as they did), with the tile's own counts in an adaptive progression (adapt_tile_args).
//
// The filter. Prep: one 16-byte record {r, g, b, v} per pixel, v = s * s of the caller's
// sigma map, a NaN v replaced by 0 and an infinite one by the largest finite float, so v is
// finite from there on. Pass i of `passes` (step 1 << i, guides fixed), pixel p:
//   g_p = sum k v_q / sum k over the 3x3 at unit spacing around p inside the image,
//         k = b[dy+1] b[dx+1], b = {1/4, 1/2, 1/4}; every pixel inside the image counts,
//         whatever its colour; a sum that overflowed is the largest finite float
//   r_p = inv_c / (g_p + var_floor)           inv_c = dn_inv_sigma2(sigma_color), every pass
//   the taps, their order, their skips, e and w: dn_filter_pixel (rt_denoise.h) with this r_p
//   out.rgb = sum w c_q / sum w              out.v = sum w (w v_q) / (sum w  sum w)
//   (w (w v), not (w w) v: w w leaves the normal range from w = 1e-19 down, where v may be 1e38)
// Edge cases beyond the shared ones:
//   a centre that passes through            its record does, v included
//   a tap whose colour is not finite        skipped: no weight in out.v either
//   g_p + var_floor = +inf                  r_p = 0: the colour term drops out; a tap whose colour
//                                           distance overflowed then has e = NaN and is skipped
//   out.v                                   a quotient that rounded past the largest finite float is
//                                           that float (the centre tap has w = 9/64, so sum w >= 9/64)
// After the last pass dn_blend runs on the rgb and sigma_out, when asked for, is rt_sqrtf(out.v) (dn_store).
#pragma once

#include "rt_adapt.h"
#include "rt_denoise.h"

namespace rtk {

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

// The binomial kernel b = {1/4, 1/2, 1/4} at offset d = -1..1.
RT_HD float dnv_b(int d) { return d == 0 ? 0.5f : 0.25f; }

// The 3x3 prefilter of the variance around (x, y), dy outer.
template <class F>
RT_HD float dnv_var3x3(const DnPass& P, int x, int y, const F& f)
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

// rt_denoise_var's mode of dn_filter_pixel: the colour scale r_p, the sum for out.v.
struct DnVar {
    static constexpr bool variance = true;
    template <class F>
    RT_HD static float color_scale(const DnPass& P, int x, int y, const F& f)
    {
        return P.inv_c / (dnv_var3x3(P, x, y, f) + P.var_floor);
    }
};

}  // namespace rtk
