// rt_dof.h — the depth-of-field stage for linear frames (include/rt_hip.h rt_dof): the lens blur of a
// thin lens built from the sharp pinhole frame and the first-hit distance the guides already hold, a
// gather over a disc whose radius is the circle of confusion (CoC). Written once for the gfx950
// kernels (rt_dof.hip) and the CPU build of the same code (rt_hostsim.cpp). Both are compiled with
// -ffp-contract=off and divide with IEEE division, as rt_bloom.h does, so the two builds give the same
// bits. No expf is evaluated, and no square root on the device: the distances of the taps come from
// a table the host builds.
//
// A w x h frame c, its guide record nd (only nd.w = t, the distance along the camera ray, is read),
// parameters focus, coc_inf, max_radius (validated: focus finite and > 0, coc_inf finite and >= 0,
// max_radius 1..12); R = (float)max_radius:
//   1  radius, per pixel p. far(p): t_p is not finite or not > 0 (a miss, a zero, a NaN).
//        r_p = far ? min(coc_inf, R) : min(coc_inf * (fabsf(t_p - focus) / t_p), R)
//      coc_out[p] = r_p. For the ordering of rule 2 a far pixel's distance is +inf. This is the
//      thin lens's circle of confusion A f |t - focus| / (t (focus - f)) with the aperture A and the
//      focal length f folded into its limit at infinity, coc_inf = A f / (focus - f), in pixels.
//      t is the distance along the ray, not the depth along the optical axis: the surface in focus
//      is a sphere about the eye. The planar form needs the camera and is not offered.
//   2  gather. For pixel p the taps q = p + (dx, dy), dy outer, dx inner, both -max_radius ..
//      max_radius ascending; a tap outside the image is skipped, and so is one whose rgb is not all
//      finite. For the others
//        re = (t_q > t_p) ? min(r_q, r_p) : r_q     a background tap never spreads further onto p than
//                                                   p's own blur: a sharp foreground stays sharp
//        a  = min((re + 0.5f) - D[|dy|][|dx|], 1.0f)   D: the float nearest sqrt(dx^2 + dy^2), a 13 x 13
//                                                   table built on the host (dof_build_table)
//        the tap is skipped unless a > 0
//        k(r) = 1.0f / (max(r, 0.5f) * max(r, 0.5f)),  wq = a * k(re)
//        S += wq * c_q.rgb,  W += wq                each product formed, then added, in tap order
//      k(re) is k(r_q) or k(r_p), two values known per pixel: the tap loop holds no division.
//   3  output. rgba_out[p] = {S / W, c_p.a}; a centre whose rgb is not all finite is copied bit for
//      bit. The centre tap of a finite centre has a = min(r_p + 0.5, 1) > 0, so W > 0.
// A skipped tap adds nothing. dof_tap below gives a skipped tap the weight +0 and a colour of zeroes
// and adds the products all the same: S and W start at +0, a sum of floats is -0 only when both terms
// are, so neither is ever -0 and adding +0 or -0 leaves each of them as it is, bit for bit (an
// infinite or NaN sum included). That is what lets a kernel visit a smaller window than the rule's
// and stay exact, and what lets a tile mark an entry outside the image like a bad colour.
// The gather is normalised, not energy-conserving: a pixel's output is a weighted mean of what
// reaches it, so a bright point spread over a disc of radius r keeps about 1 / (pi r^2) of its value
// where it lands on equally blurred neighbours, and more where its neighbours are sharper.
// Decisions the list above leaves open, made here:
//   min and max        are rt_min / rt_max (rt_fp.h): min(x, R) is R < x ? R : x. The one NaN the radius
//                      can meet is coc_inf = 0 times a ratio that overflowed (t below focus / FLT_MAX):
//                      dof_radius takes coc_inf = 0 before the product, so r = 0 for every pixel then.
//   the sign of a zero a channel of -0 comes back +0: S starts at +0, and +0 + (wq * -0) is +0, so the
//                      output is +0 / W. Equal as values, not as bits; alpha and a bad centre are copied
//                      bit for bit.
//   a negative channel is averaged like any other; nothing is clamped.
//   overflow of S      is not caught: at r = 0 the single weight is 2, so a channel above FLT_MAX / 2 sums
//                      to an infinity and the output is inf / 2 = inf; two infinities of opposite sign
//                      give a NaN, as the arithmetic does. W is at most 625 * 4.
//   t_q == t_p         is not "behind": re = r_q. Two far pixels (+inf both) likewise; their radii are equal.
//   a negative or NaN t is far, like a miss (t = -1): the guides write -1 for a miss, the rest is caution.
#pragma once

#include <cmath>

#include "rt_denoise.h"

namespace rtk {

constexpr int DOF_MAX_RADIUS = 12;
constexpr int DOF_TAB = DOF_MAX_RADIUS + 1;  // the table's side: D[|dy|][|dx|], 0..12 each

struct DofArgs {
    int w, h, R;           // validated; R = max_radius
    float focus, coc_inf;  // validated
    const float4_* in;
    const float4_* nd;
    float D[DOF_TAB * DOF_TAB];  // dof_build_table
};

// The host's part of rule 2: the float nearest sqrt(dx^2 + dy^2) (sqrtf is correctly rounded).
inline void dof_build_table(float* D)
{
    for (int dy = 0; dy < DOF_TAB; dy++)
        for (int dx = 0; dx < DOF_TAB; dx++) D[dy * DOF_TAB + dx] = std::sqrt((float)(dx * dx + dy * dy));
}

RT_HD float dof_inf() { return rt_asfloat(0x7f800000u); }
RT_HD float dof_neg_inf() { return rt_asfloat(0xff800000u); }
RT_HD int dof_absi(int v) { return v < 0 ? -v : v; }

RT_HD bool dof_far(float t) { return (rt_asuint(t) & 0x7f800000u) == 0x7f800000u || !(t > 0.0f); }

// Rule 1: the radius of a pixel with ray distance t.
RT_HD float dof_radius(const DofArgs& A, float t)
{
    const float R = (float)A.R;
    if (dof_far(t) || A.coc_inf == 0.0f) return rt_min(A.coc_inf, R);
    const float d = t - A.focus;
    return rt_min(A.coc_inf * ((d < 0.0f ? -d : d) / t), R);
}

RT_HD float dof_k(float r)
{
    const float m = rt_max(r, 0.5f);
    return 1.0f / (m * m);
}

// What a pixel is as a tap: its colour and radius in one 16-B record, its ordering distance and k(r)
// in one 8-B record. A tap the rule skips whatever the centre (outside the image, a bad colour) has
// r = -inf, which makes a of rule 2 -inf, and a colour of zeroes.
struct DofRec {
    float4_ cr;  // {r, g, b, r_q}
    float t, k;  // t_q (+inf when far), k(r_q)
};

RT_HD DofRec dof_skipped() { return DofRec{float4_{0.0f, 0.0f, 0.0f, dof_neg_inf()}, dof_inf(), 4.0f}; }

RT_HD DofRec dof_record(const DofArgs& A, const float4_& c, float t)
{
    if (!dn_finite3(c)) return dof_skipped();
    const float r = dof_radius(A, t);
    return DofRec{float4_{c.x, c.y, c.z, r}, dof_far(t) ? dof_inf() : t, dof_k(r)};
}

// The centre's side of rule 2, and the sums.
struct DofCentre {
    float r, t, k;  // r_p, t_p (+inf when far), k(r_p)
};
struct DofSum {
    float x, y, z, w;
};

// One tap of rule 2; D is the table's entry for its offset.
RT_HD void dof_tap(DofSum& s, const DofCentre& p, const float4_& cr, float tq, float kq, float D)
{
    const bool behind = tq > p.t;
    const bool own = behind && p.r < cr.w;  // min(r_q, r_p) is r_p
    const float re = own ? p.r : cr.w;
    const float a = rt_min((re + 0.5f) - D, 1.0f);
    const float wq = a > 0.0f ? a * (own ? p.k : kq) : 0.0f;
    s.x = s.x + wq * cr.x;
    s.y = s.y + wq * cr.y;
    s.z = s.z + wq * cr.z;
    s.w = s.w + wq;
}

// Rule 3 for a finite centre c.
RT_HD float4_ dof_resolve(const DofSum& s, const float4_& c) { return float4_{s.x / s.w, s.y / s.w, s.z / s.w, c.w}; }

// Taps straight from the frame (hostsim; k_dof_direct's DofGlobal answers the same from 16-B loads): the record of
// pixel (x, y), inside the image or not.
struct DofDirect {
    const DofArgs& A;
    RT_HD DofRec rec(int x, int y) const
    {
        if (x < 0 || x >= A.w || y < 0 || y >= A.h) return dof_skipped();
        const size_t q = (size_t)y * A.w + x;
        return dof_record(A, A.in[q], A.nd[q].w);
    }
};

// One output pixel over the rule's whole window; c and t are p's own records. *r_out receives r_p.
template <class F>
RT_HD float4_ dof_pixel(const DofArgs& A, int x, int y, const float4_& c, float t, const F& f, float* r_out)
{
    const float r = dof_radius(A, t);
    *r_out = r;
    if (!dn_finite3(c)) return c;
    const DofCentre p{r, dof_far(t) ? dof_inf() : t, dof_k(r)};
    DofSum s{0.0f, 0.0f, 0.0f, 0.0f};
    for (int dy = -A.R; dy <= A.R; dy++)
        for (int dx = -A.R; dx <= A.R; dx++) {
            const DofRec q = f.rec(x + dx, y + dy);
            dof_tap(s, p, q.cr, q.t, q.k, A.D[dof_absi(dy) * DOF_TAB + dof_absi(dx)]);
        }
    return dof_resolve(s, c);
}

}  // namespace rtk
