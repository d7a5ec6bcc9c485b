// rt_upscale.h — the guided upscale stage (include/rt_hip.h rt_upscale): a frame rendered at
// w_lo x h_lo taken to w x h by joint-bilateral upsampling (Kopf et al. 2007), each low-resolution
// tap weighted by how well its first-hit guides agree with the output pixel's full-size guides, so
// that object, material and silhouette edges come out at output resolution. Written once for the
// gfx950 kernels (rt_upscale.hip) and the CPU build of the same code (rt_hostsim.cpp). Both are
// compiled with -ffp-contract=off, divide with IEEE division and take rt_libm's expf and rt_sqrtf,
// so the two builds give the same bits.
//
// Tap position. sx = (float)w_lo / (float)w and sy = (float)h_lo / (float)h are computed once on
// the host. For output pixel (X, Y): fx = (float)X * sx, x0 = (int)fx, tx = fx - (float)x0, and the
// same in y: feature_ray aims at x_j = x, so there is no half-pixel term.
//
// Guide weight of a low tap q against output pixel p (dn_filter_pixel's guide part and nothing else;
// n, t from normal_depth, a from albedo, the 1 / sigma^2 from dn_inv_sigma2 on the host):
//   hit state differs (t > 0)                  the tap is skipped
//   e = |n_p - n_q|^2 inv_n + |a_p - a_q|^2 inv_a, + ((t_p - t_q) / max(t_p, t_q))^2 inv_t when both hit
//   !(e >= 0)                                  the tap is skipped;  else g = rt_expf(-e)
// Whatever the tier, a tap is also skipped when it lies outside the low frame, when its rgb is not
// all finite, when a sigma is given and the tap's is not finite, and when its spatial weight is
// exactly 0; these tests come before the guides are read.
//
//   tier 1  the taps (x0 + dx, y0 + dy), dx, dy in {0, 1}, dy outer; spatial weight b = (y weight)
//           (x weight), the weights (1 - t, t); wgt = b g. In tap order: sum wgt c, S = sum wgt and
//           V = sum wgt (wgt v_q), v_q = dnv_variance(sigma_q) (rt_dnv.h: s s, at most the largest
//           float; wgt (wgt v) and not (wgt wgt) v for rt_dnv.h's reason). Taken when S > min_weight.
//   tier 2  otherwise: dx, dy in {-1, 0, 1, 2}, dy outer, b = k(y) k(x), k(d) = 1 - |d| / 2 at
//           d = (float)(x0 + dx) - fx: the tent of half-width 2, continuous in fx as tier 1's is.
//           The same guide weight, the same sums, started again from 0. Taken when S > 0.
//   tier 3  otherwise: tier 1's taps and weights with g = 1 (plain bilinear over the finite taps
//           inside the frame; the hit states are not compared). Taken when S > 0.
//   empty   otherwise: rgba_out = {0, 0, 0, 1}, sigma_out = +inf.
// Output: rgb = sums / S, alpha 1; sigma_out = rt_sqrtf(min(V, largest float)) / S.
//
// Neighbouring outputs share taps, so their errors are correlated: sigma_out is each pixel's
// marginal standard deviation, not that of an independent sample. A filter that takes it as
// independent (rt_denoise_var) underestimates what is left after averaging neighbours.
//
// What follows from the rule, each case once:
//   a NaN in n_p or a_p         every e is a NaN in tiers 1 and 2: the pixel is tier 3's bilinear value
//   an infinite guide           the same where the difference is infinite or a NaN
//   p a miss, the taps all hits (or the reverse): tiers 1 and 2 are empty, tier 3 answers
//   a NaN, infinite or negative sigma_q   NaN and infinite: the tap is skipped; negative: v = s s
//   weights below 1e-19         (tier 2 where no tap agrees with p) V = sum wgt (wgt v) falls below float32's normal
//                               range and loses bits: sigma_out is then only as good as sqrt(2^-144) / S
//   the low rgba's alpha        never read; the low albedo's fourth component neither
//   sums that overflow          rgb is +-inf or a NaN as IEEE gives it, the same in both builds
//   the identity                w_lo == w, h_lo == h (up to 2^24 pixels a side, where (float)X is X)
//                               and the same guides: tx = ty = 0, tap (X, Y) alone has a weight, b = 1,
//                               e = 0, g = 1: rgb is c 1 / 1 = c bit for bit, and sigma_out is
//                               rt_sqrtf(s s) = s for a sigma >= 0 whose square neither overflows nor
//                               falls below the normal range. A pixel whose colour or sigma is not
//                               finite is rebuilt from its neighbours by tier 2.
//   overlapping buffers         an output whose bytes overlap an input's or the other output's is
//                               RT_ERR_ARG (rt_capi_stages.cpp): a block reads low pixels other blocks write
#pragma once

#include "rt_dnv.h"

namespace rtk {

struct UpArgs {
    int w_lo, h_lo, w, h;
    float sx, sy;                // (float)w_lo / (float)w, (float)h_lo / (float)h
    float inv_n, inv_a, inv_t;   // 1 / sigma^2 (dn_inv_sigma2)
    float min_weight;
    const float4_* rgba_lo;      // w_lo * h_lo
    const float* sigma_lo;       // w_lo * h_lo, or null
    const float4_* alb_lo;
    const float4_* nd_lo;
    const float4_* alb_hi;       // w * h
    const float4_* nd_hi;
};

struct UpOut {
    float4_ rgba;
    float sigma;
    int tier;  // 1, 2, 3; 0: empty (not stored)
};

RT_HD bool up_finite(float s) { return (rt_asuint(s) & 0x7f800000u) != 0x7f800000u; }

// A low pixel's record {r, g, b, sigma} (sigma 0 without a sigma map) and guides, read straight from
// the frame (the hostsim loop, the direct kernel); the LDS tile of rt_upscale.hip is the other F.
struct UpDirect {
    const UpArgs& A;
    RT_HD float4_ rec(int x, int y) const
    {
        const size_t q = (size_t)y * A.w_lo + x;
        const float4_ c = A.rgba_lo[q];
        return float4_{c.x, c.y, c.z, A.sigma_lo ? A.sigma_lo[q] : 0.0f};
    }
    RT_HD float4_ nd(int x, int y) const { return A.nd_lo[(size_t)y * A.w_lo + x]; }
    RT_HD float4_ alb(int x, int y) const { return A.alb_lo[(size_t)y * A.w_lo + x]; }
};

struct UpSums {
    float r = 0.0f, g = 0.0f, b = 0.0f, s = 0.0f, v = 0.0f;
};

// One tap with spatial weight b into the sums; guided: the guide weight, else g = 1 (tier 3).
template <class F>
RT_HD void up_tap(const UpArgs& A, const F& f, int qx, int qy, float b, bool guided, const float4_& np, const float4_& ap,
                  UpSums& U)
{
    if (b == 0.0f) return;
    if (qx < 0 || qx >= A.w_lo || qy < 0 || qy >= A.h_lo) return;
    const float4_ c = f.rec(qx, qy);
    if (!dn_finite3(c)) return;
    if (A.sigma_lo && !up_finite(c.w)) return;
    float g = 1.0f;
    if (guided) {
        const float4_ nq = f.nd(qx, qy);
        const float4_ aq = f.alb(qx, qy);
        const bool hit_p = np.w > 0.0f, hit_q = nq.w > 0.0f;
        if (hit_p != hit_q) return;
        float e = dn_dist2(np, nq) * A.inv_n;
        e = e + dn_dist2(ap, aq) * A.inv_a;
        if (hit_p) {
            const float r = (np.w - nq.w) / rt_max(np.w, nq.w);
            e = e + (r * r) * A.inv_t;
        }
        if (!(e >= 0.0f)) return;
        g = rt_expf(-e);
    }
    const float wgt = b * g;
    U.r = U.r + wgt * c.x;
    U.g = U.g + wgt * c.y;
    U.b = U.b + wgt * c.z;
    U.s = U.s + wgt;
    U.v = U.v + wgt * (wgt * dnv_variance(c.w));
}

// Tier 1's and tier 3's four taps.
template <class F>
RT_HD UpSums up_bilinear(const UpArgs& A, const F& f, int x0, int y0, float tx, float ty, bool guided, const float4_& np,
                         const float4_& ap)
{
    UpSums U;
    for (int dy = 0; dy <= 1; dy++) {
        const float by = dy ? ty : 1.0f - ty;
        for (int dx = 0; dx <= 1; dx++) up_tap(A, f, x0 + dx, y0 + dy, by * (dx ? tx : 1.0f - tx), guided, np, ap, U);
    }
    return U;
}

RT_HD float up_tent(int q, float fpos)
{
    const float d = (float)q - fpos;
    return 1.0f - (d < 0.0f ? -d : d) * 0.5f;
}

RT_HD UpOut up_result(const UpArgs& A, const UpSums& U, int tier)
{
    const float sigma = A.sigma_lo ? rt_sqrtf(rt_min(U.v, DNV_VMAX)) / U.s : 0.0f;
    return UpOut{float4_{U.r / U.s, U.g / U.s, U.b / U.s, 1.0f}, sigma, tier};
}

// One output pixel. np, ap: its full-size guides. F says where a low pixel's records are read from;
// it is asked only for pixels inside the low frame.
template <class F>
RT_HD UpOut up_pixel(const UpArgs& A, int X, int Y, const float4_& np, const float4_& ap, const F& f)
{
    const float fx = (float)X * A.sx, fy = (float)Y * A.sy;
    const int x0 = (int)fx, y0 = (int)fy;
    const float tx = fx - (float)x0, ty = fy - (float)y0;
    const UpSums U1 = up_bilinear(A, f, x0, y0, tx, ty, true, np, ap);
    if (U1.s > A.min_weight) return up_result(A, U1, 1);
    UpSums U2;
    for (int dy = -1; dy <= 2; dy++) {
        const float ky = up_tent(y0 + dy, fy);
        for (int dx = -1; dx <= 2; dx++) up_tap(A, f, x0 + dx, y0 + dy, ky * up_tent(x0 + dx, fx), true, np, ap, U2);
    }
    if (U2.s > 0.0f) return up_result(A, U2, 2);
    const UpSums U3 = up_bilinear(A, f, x0, y0, tx, ty, false, np, ap);
    if (U3.s > 0.0f) return up_result(A, U3, 3);
    return UpOut{float4_{0.0f, 0.0f, 0.0f, 1.0f}, __builtin_inff(), 0};
}

// The low-resolution footprint of the output rectangle [X0, X1] x [Y0, Y1] (inside the frame), tier
// 2's ring included: fx is monotone in X (a rounded conversion times a positive constant, rounded),
// so every x0 lies between the first and the last pixel's.
struct UpFoot {
    int x0, y0, w, h;  // origin in the low frame (may be -1), extent
};

RT_HD UpFoot up_footprint(const UpArgs& A, int X0, int Y0, int X1, int Y1)
{
    const int xa = (int)((float)X0 * A.sx), xb = (int)((float)X1 * A.sx);
    const int ya = (int)((float)Y0 * A.sy), yb = (int)((float)Y1 * A.sy);
    return UpFoot{xa - 1, ya - 1, xb - xa + 4, yb - ya + 4};
}

}  // namespace rtk
