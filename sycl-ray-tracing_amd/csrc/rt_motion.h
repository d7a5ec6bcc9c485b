// rt_motion.h — the motion stages for linear frames (include/rt_hip.h rt_motion_vectors, rt_motion_blur):
// where each pixel's first hit stood in the previous camera's frame, and a shutter's blur built from
// the sharp frame along those vectors (McGuire et al. 2012, "A Reconstruction Filter for Plausible
// Motion Blur", with nearest taps and a hard cylinder). Written once for the gfx950 kernels
// (rt_motion.hip) and the CPU build of the same code (rt_hostsim.cpp). Both are compiled with
// -ffp-contract=off, divide with IEEE division and take rt_sqrtf and floorf, as rt_temporal.h does,
// so the two builds give the same bits. No expf is evaluated.
//
// rt_motion_vectors. Pixel p = (x, y) of a w x h frame, g = normal_depth[p] = {n, t} under the
// current camera, the previous camera given by prev_view and prev_fov_dist:
//   (fx, fy)  steps 3 and 4 of rt_temporal.h, the same expressions in the same order:
//             (o, d) = feature_ray(current camera, x, y); P = o + t d for a hit (t > 0), o_prev + d
//             for a miss; q = xform_point(prev_inv, P); ratio = q.z / prev_fov_dist;
//             fx = (((q.x / ratio) / aspect + 1) * 0.5) * (float)w, fy = ((q.y / ratio + 1) * 0.5) * (float)h
//   m_p = {fx - (float)x, fy - (float)y}: where the point was, minus where it is now
//   m_p = {0, 0} when one of g's four floats is a NaN, when ratio is not > 0 (the point was behind
//   the previous camera), or when fx or fy is not finite. Temporal's range test is not applied: a
//   point that came from off-screen still moved.
//
// rt_motion_blur. A w x h frame c, its guide record nd (only nd.w = t is read), a motion field m
// (float2 per pixel, in pixels per frame interval), parameters shutter (0..1), depth_soft (> 0,
// finite), max_radius (1..16); R = (float)max_radius:
//   1  reach, per pixel p. a = 0.5f * shutter, hx = a * m.x, hy = a * m.y, l2 = hx * hx + hy * hy.
//      l2 not finite (a NaN motion, one beyond about 1e19 px): h = 0, l = 0. Else l = rt_sqrtf(l2),
//      and when l > R: s = R / l, hx *= s, hy *= s, l = R (set, not recomputed). reach_out[p] = l.
//      k_p = 1.0f / rt_max(l, 0.5f). t'_p = (t finite and > 0) ? rt_min(t, 1e30f) : 1e30f (a miss, a
//      zero, a NaN count as far). iz_p = 1.0f / (depth_soft * t'_p).
//   2  tile max. Motion tiles are 16 x 16 pixels, partial at the right and bottom edges. A tile's
//      record {hx, hy, l} is that of its pixel of largest l, the first in raster order among equals:
//      the maximum of the 64-bit key (l's bits << 32) | (256 - index within the tile), which any
//      order of reduction gives (l >= 0, so its bits order as the floats do).
//   3  neighbour max. The tile and its up to eight neighbours inside the tile grid, dy outer, dx
//      inner, both -1 .. 1 ascending; the record of the first one visited, then any of strictly
//      larger l replaces it: {Nx, Ny, L}, uniform over the tile. max_radius <= 16 makes 3 x 3
//      tiles enough: no pixel's streak reaches further than one tile.
//   4  gather. Unless L >= 0.5f every pixel of the tile is copied bit for bit. Else
//      n = (int)floorf(L), plus one when (float)n < L (ceil: 1..R); dx = Nx / (float)n,
//      dy = Ny / (float)n, ds = L / (float)n. Taps j = -n .. n ascending. j = 0 is the centre, with
//      weight k_p. The others lie at q = p + (ox_j, oy_j), ox_j = (int)floorf((float)j * dx + 0.5f),
//      oy_j likewise; a tap outside the image or whose rgb is not all finite is skipped. Else
//      d = (float)|j| * ds,
//        fore = clamp01(1 - (t'_q - t'_p) * iz_p)      q in front of p: it spreads over p by its own reach
//        back = clamp01(1 - (t'_p - t'_q) * iz_p)      q behind p: p's own blur shows it
//        cone(d, k) = rt_max(1 - d * k, 0),  cyl(d, l) = d <= l ? 1 : 0
//        alpha = fore * cone(d, k_q) + back * cone(d, k_p) + 2 * (cyl(d, l_q) * cyl(d, l_p))
//      each product formed, then the three added left to right; S += alpha * c_q.rgb, W += alpha, in
//      tap order.
//   5  output. rgba_out[p] = {S / W, c_p.a}; a centre whose rgb is not all finite is copied bit for
//      bit. Any other centre has W >= k_p > 0 (k_p is in [1 / 16, 2]).
// A skipped tap adds nothing. mb_tap below gives a skipped tap the weight +0 and a colour of zeroes
// and adds the products all the same: S and W start at +0, a sum of floats is -0 only when both terms
// are, so neither is ever -0 and adding +0 or -0 leaves each of them as it is, bit for bit. A skipped
// tap's record is {0, 0, 0, l_q = -1}, {t'_q = -inf, k_q = +inf}: cyl(d, -1) is 0, cone(d, +inf) is 0
// (d > 0: ds >= 0.5), back is clamp01 of -inf or of a NaN, both 0; so alpha is +0 by the rule's own
// arithmetic and the tile of rt_motion.hip marks an entry outside the image like a bad colour.
// What follows from the rule: a still pixel (l_p = 0, k_p = 2) takes nothing from still neighbours at
// any depth (ds >= 0.5, so cone(d, 2) = 0, and cyl(d, 0) = 0); it takes nothing from moving taps more
// than depth_soft behind it (fore = 0) and then comes back exactly, (2 c) / 2; a moving nearer tap
// bleeds over it up to that tap's own reach (fore * cone(d, k_q)) and no further. shutter 0 or a
// motion of zeroes: every L is 0, the frame is copied bit for bit.
// Decisions the list above leaves open, made here:
//   clamp01(x)         is x > 0 ? (x < 1 ? x : 1) : 0, so a NaN is 0. iz_p is +inf when depth_soft * t'_p
//                      underflows to 0 and 0 when it overflows; (t'_q - t'_p) * iz_p is then a NaN for equal
//                      distances (fore = back = 0) and for a skipped tap.
//   rt_min, rt_max     as rt_fp.h has them: rt_max(l, 0.5f) is l < 0.5f ? 0.5f : l.
//   the tile's h       is the winner's clamped (hx, hy), which may be a pair of tiny non-zero floats whose
//                      l2 underflowed to l = 0; such a tile has L < 0.5 and is copied.
//   the sign of zero   a channel of -0 under a gather comes back +0 (S starts at +0); a copied tile keeps bits.
//   a negative channel is averaged like any other; nothing is clamped; overflow of S is what the arithmetic
//                      gives (W is at most 2 + 32 * 4).
//   ox_j               floorf(x + 0.5f) is not symmetric about 0 (j dx = -2.5 gives -2, +2.5 gives 3); the
//                      taps are the rule's all the same. |ox_j| is largest at j = -n or n.
//   a negative or NaN t is far, like a miss (t = -1): the guides write -1 for a miss, the rest is caution.
//   the vectors' NaN   a NaN in prev_view or the camera cannot pass the argument check; a NaN q or ratio from an
//                      overflow gives {0, 0} through the two tests of the list.
#pragma once

#include <cmath>

#include "rt_denoise.h"

namespace rtk {

constexpr int MB_MAX_RADIUS = 16;
constexpr int MB_TILE = 16;  // a motion tile's side in pixels

struct alignas(8) MbVec {
    float x, y;
};

// ------------------------------------------------------------------ vectors
struct MotionVecArgs {
    CamView cur;        // this frame's camera (cam_view of the context's camera)
    RtCamera prev_inv;  // m: the inverse of the previous view matrix; fov_dist: the previous camera's
    float o_prev[3];    // xform_point(previous camera, 0)
    const float4_* nd;
};

RT_HD bool mb_finite(float v) { return (rt_asuint(v) & 0x7f800000u) != 0x7f800000u; }

RT_HD MbVec mv_pixel(const MotionVecArgs& A, int x, int y, const float4_& g)
{
    const MbVec zero{0.0f, 0.0f};
    if (rt_isnan(g.x) || rt_isnan(g.y) || rt_isnan(g.z) || rt_isnan(g.w)) return zero;
    const int w = A.cur.W, h = A.cur.H;
    V3 o, d;
    feature_ray(A.cur, x, y, o, d);
    const V3 op = v3(A.o_prev[0], A.o_prev[1], A.o_prev[2]);
    const V3 P = g.w > 0.0f ? add(o, mul(g.w, d)) : add(op, d);
    const V3 q = xform_point(A.prev_inv, P);
    const float ratio = q.z / A.prev_inv.fov_dist;
    if (!(ratio > 0.0f)) return zero;
    const float fx = (((q.x / ratio) / A.cur.aspect + 1.0f) * 0.5f) * (float)w;
    const float fy = ((q.y / ratio + 1.0f) * 0.5f) * (float)h;
    if (!mb_finite(fx) || !mb_finite(fy)) return zero;
    return MbVec{fx - (float)x, fy - (float)y};
}

// ------------------------------------------------------------------ blur
struct MotionArgs {
    int w, h, R;          // validated; R = max_radius
    float a, depth_soft;  // a = 0.5f * shutter
    const float4_* in;
    const float4_* nd;
    const MbVec* motion;
};

RT_HD int mb_tiles_x(int w) { return (w + MB_TILE - 1) / MB_TILE; }
RT_HD int mb_tiles_y(int h) { return (h + MB_TILE - 1) / MB_TILE; }

RT_HD float mb_inf() { return rt_asfloat(0x7f800000u); }
RT_HD float mb_neg_inf() { return rt_asfloat(0xff800000u); }
RT_HD float mb_clamp01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

// Rule 1: {hx, hy, l, 0} of a pixel with motion m.
RT_HD float4_ mb_reach(const MotionArgs& A, const MbVec& m)
{
    float hx = A.a * m.x, hy = A.a * m.y;
    const float l2 = hx * hx + hy * hy;
    if (!mb_finite(l2)) return float4_{0.0f, 0.0f, 0.0f, 0.0f};
    float l = rt_sqrtf(l2);
    const float R = (float)A.R;
    if (l > R) {
        const float s = R / l;
        hx = hx * s;
        hy = hy * s;
        l = R;
    }
    return float4_{hx, hy, l, 0.0f};
}
RT_HD float mb_k(float l) { return 1.0f / rt_max(l, 0.5f); }
RT_HD float mb_far(float t) { return (mb_finite(t) && t > 0.0f) ? rt_min(t, 1e30f) : 1e30f; }

// Rule 2's key of the pixel at index i (0..255, raster order) within its tile; 0 is below every pixel's key.
RT_HD unsigned long long mb_key(float l, int i) { return ((unsigned long long)rt_asuint(l) << 32) | (unsigned)(MB_TILE * MB_TILE - i); }
RT_HD int mb_key_index(unsigned long long key) { return MB_TILE * MB_TILE - (int)(key & 0xffffffffu); }

// Rule 3: {Nx, Ny, L} of tile (tx, ty) from the tile records {hx, hy, l, 0}.
RT_HD float4_ mb_neighbour_max(const float4_* tiles, int ntx, int nty, int tx, int ty)
{
    float4_ N{0.0f, 0.0f, -1.0f, 0.0f};
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = tx + dx, qy = ty + dy;
            if (qx < 0 || qx >= ntx || qy < 0 || qy >= nty) continue;
            const float4_ r = tiles[(size_t)qy * ntx + qx];
            if (r.z > N.z) N = r;
        }
    return N;
}

// Rule 4's line of a tile: n, the steps per tap.
struct MbLine {
    int n;
    float dx, dy, ds;
};
RT_HD MbLine mb_line(const float4_& N)  // (N.z >= 0.5f)
{
    int n = (int)__builtin_floorf(N.z);
    if ((float)n < N.z) n++;
    const float fn = (float)n;
    return MbLine{n, N.x / fn, N.y / fn, N.z / fn};
}
RT_HD int mb_off(int j, float step) { return (int)__builtin_floorf((float)j * step + 0.5f); }
RT_HD int mb_absi(int v) { return v < 0 ? -v : v; }

// What a pixel is as a tap: its colour and reach in one 16-B record, its distance and k in one 8-B record.
struct MbRec {
    float4_ cl;  // {r, g, b, l_q}
    float t, k;  // t'_q, k_q
};
RT_HD MbRec mb_skipped() { return MbRec{float4_{0.0f, 0.0f, 0.0f, -1.0f}, mb_neg_inf(), mb_inf()}; }
RT_HD MbRec mb_record(const MotionArgs& A, const float4_& c, float t, const MbVec& m)
{
    if (!dn_finite3(c)) return mb_skipped();
    const float l = mb_reach(A, m).z;
    return MbRec{float4_{c.x, c.y, c.z, l}, mb_far(t), mb_k(l)};
}

// The centre's side of rule 4, and the sums.
struct MbCentre {
    float l, t, k, iz;  // l_p, t'_p, k_p, iz_p
};
RT_HD MbCentre mb_centre(const MotionArgs& A, float l, float t)
{
    const float tp = mb_far(t);
    return MbCentre{l, tp, mb_k(l), 1.0f / (A.depth_soft * tp)};
}
struct MbSum {
    float x, y, z, w;
};

// One tap of rule 4 at distance d along the line.
RT_HD void mb_tap(MbSum& s, const MbCentre& p, const float4_& cl, float tq, float kq, float d)
{
    const float fore = mb_clamp01(1.0f - (tq - p.t) * p.iz);
    const float back = mb_clamp01(1.0f - (p.t - tq) * p.iz);
    const float cq = rt_max(1.0f - d * kq, 0.0f), cp = rt_max(1.0f - d * p.k, 0.0f);
    const float cy = (d <= cl.w ? 1.0f : 0.0f) * (d <= p.l ? 1.0f : 0.0f);
    const float alpha = (fore * cq + back * cp) + 2.0f * cy;
    s.x = s.x + alpha * cl.x;
    s.y = s.y + alpha * cl.y;
    s.z = s.z + alpha * cl.z;
    s.w = s.w + alpha;
}
RT_HD void mb_centre_tap(MbSum& s, const MbCentre& p, const float4_& c)
{
    s.x = s.x + p.k * c.x;
    s.y = s.y + p.k * c.y;
    s.z = s.z + p.k * c.z;
    s.w = s.w + p.k;
}
RT_HD float4_ mb_resolve(const MbSum& s, const float4_& c) { return float4_{s.x / s.w, s.y / s.w, s.z / s.w, c.w}; }

// Taps straight from the frame (hostsim; k_mblur_direct's MbGlobal answers the same from whole-record loads): the
// record of pixel (x, y), inside the image or not.
struct MbDirect {
    const MotionArgs& A;
    RT_HD MbRec rec(int x, int y) const
    {
        if (x < 0 || x >= A.w || y < 0 || y >= A.h) return mb_skipped();
        const size_t q = (size_t)y * A.w + x;
        return mb_record(A, A.in[q], A.nd[q].w, A.motion[q]);
    }
};

// One output pixel of a tile whose rule 3 gave N = {Nx, Ny, L}; c, t and l are p's own colour, distance and reach.
template <class F>
RT_HD float4_ mb_pixel(const MotionArgs& A, int x, int y, const float4_& c, float t, float l, const float4_& N, const F& f)
{
    if (!(N.z >= 0.5f) || !dn_finite3(c)) return c;
    const MbLine ln = mb_line(N);
    const MbCentre p = mb_centre(A, l, t);
    MbSum s{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = -ln.n; j <= ln.n; j++) {
        if (j == 0) {
            mb_centre_tap(s, p, c);
            continue;
        }
        const MbRec q = f.rec(x + mb_off(j, ln.dx), y + mb_off(j, ln.dy));
        mb_tap(s, p, q.cl, q.t, q.k, (float)mb_absi(j) * ln.ds);
    }
    return mb_resolve(s, c);
}

}  // namespace rtk
