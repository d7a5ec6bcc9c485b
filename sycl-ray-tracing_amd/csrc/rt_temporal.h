// rt_temporal.h — temporal accumulation (include/rt_hip.h rt_temporal_accumulate): the
// per-pixel arithmetic that reprojects the previous frame's accumulated colour, variance and
// history length into the current camera and blends the new frame in (Schied et al. 2017,
// SVGF's first half), written once for the gfx950 kernel (rt_temporal.hip) and the CPU build
// of the same code (rt_hostsim.cpp). Both are compiled with -ffp-contract=off, divide with
// IEEE division and take rt_sqrtf and floorf, as rt_dnv.h does, so the two builds give the
// same bits. No expf is evaluated.
//
// Pixel p = (x, y) of a w x h frame; c = rgba_in[p], g = normal_depth[p] = {n, t}:
//   1  v_c = dnv_variance(sigma_in[p])            (a NaN gives 0, an infinity the largest float)
//   2  carry: out = {c.rgb, 1}, sigma_out = rt_sqrtf(v_c), len_out = 1, when c.rgb is not finite,
//      any of g's four floats is a NaN, or there is no history (first frame; steps 4 and 5)
//   3  (o, d) = feature_ray(current camera, x, y); hit (t > 0): P = o + t d, t_exp = |P - o_prev|;
//      miss: P = o_prev + d (the environment is at infinity: only the rotation counts)
//   4  q = xform_point(prev_inv, P); ratio = q.z / prev_fov_dist; no history unless ratio > 0
//      fx = (((q.x / ratio) / aspect + 1) * 0.5) * (float)w     fy = ((q.y / ratio + 1) * 0.5) * (float)h
//      ix = floorf(fx), tx = fx - ix, the same for y
//   5  taps (ix + dx, iy + dy), dy outer, b = (dy ? ty : 1 - ty) * (dx ? tx : 1 - tx); skipped when
//      b == 0, outside the image, hist_len not > 0, colour or sigma not finite, hit state differs
//      from p's, and for hits unless |t_q - t_exp| <= depth_tol * t_exp and dot(n_p, n_q) >= normal_cos
//      S = sum b; no history unless S > min_weight; c_h = sum b c_q / S, len_h = sum b len_q / S,
//      v_h = min(sum b (sigma_q sigma_q) / S, largest float)
//   6  len = min(len_h + 1, max_len), a = 1 / len, rgb = c_h + a (c - c_h), alpha 1,
//      v = min(((1 - a) (1 - a)) v_h + a (a v_c), largest float), sigma_out = rt_sqrtf(v), len_out = len
// Decisions the list above leaves open, made here:
//   position range     a pixel whose fx is not inside (-1, w) or whose fy is not inside (-1, h) has no
//                      history. All four taps of such a position lie outside the image, so S would be 0:
//                      the test changes no result and keeps a NaN or huge fx away from the float -> int
//                      conversion, which differs between the builds there.
//   the order of b     the y weight times the x weight; the sums run in tap order, dy outer.
//   a tap's guide      is read only through the comparisons above: a NaN t_q makes the tap a miss (t_q > 0
//                      is false), a NaN n_q or t_q fails the hit tests, so the tap is skipped for a hit p.
//   a centre miss      takes every miss tap that passes the colour, sigma and len tests: no depth, no normal.
//   t_exp              rt_sqrtf of the squared distance (rt_trace.h length), not a projection on the view axis:
//                      t is the ray parameter of a unit direction, so the two are the same measure.
//   an infinite len_q  counts (len_q > 0): len_h is then infinite and len = max_len.
//   overflow           b c_q of a finite colour may overflow; the colour is then what the arithmetic gives.
//                      sigma_q sigma_q and the sums over it may: v_h and v are clamped to the largest float.
//   alpha              rgba_in's and hist_rgba's alpha play no part; rgba_out's is 1.
#pragma once

#include "rt_dnv.h"

namespace rtk {

struct TemporalFrame {
    CamView cur;         // this frame's camera (cam_view of the context's camera)
    RtCamera prev_inv;   // m: the inverse of the history's view matrix; fov_dist: the history's
    float o_prev[3];     // xform_point(history's camera, 0)
    float depth_tol, normal_cos, min_weight, max_len;
    const float4_* in;   // this frame: colour, sigma, guide
    const float* sigma;
    const float4_* nd;
    const float4_* h_rgba;  // the history (all null: the first frame)
    const float* h_sigma;
    const float* h_len;
    const float4_* h_nd;
};

struct TemporalOut {
    float4_ rgba;
    float sigma, len;
};

RT_HD bool tp_finite(float v) { return (rt_asuint(v) & 0x7f800000u) != 0x7f800000u; }

RT_HD TemporalOut temporal_pixel(const TemporalFrame& T, int x, int y)
{
    const int w = T.cur.W, h = T.cur.H;
    const size_t p = (size_t)y * w + x;
    const float4_ c = T.in[p];
    const float4_ g = T.nd[p];
    const float vc = dnv_variance(T.sigma[p]);
    const TemporalOut carry{float4_{c.x, c.y, c.z, 1.0f}, rt_sqrtf(vc), 1.0f};
    if (!T.h_rgba || !dn_finite3(c) || rt_isnan(g.x) || rt_isnan(g.y) || rt_isnan(g.z) || rt_isnan(g.w)) return carry;

    V3 o, d;
    feature_ray(T.cur, x, y, o, d);
    const V3 op = v3(T.o_prev[0], T.o_prev[1], T.o_prev[2]);
    const bool hit_p = g.w > 0.0f;
    const V3 P = hit_p ? add(o, mul(g.w, d)) : add(op, d);
    const float t_exp = hit_p ? length(sub(P, op)) : 0.0f;
    const V3 np = v3(g.x, g.y, g.z);

    const V3 q = xform_point(T.prev_inv, P);
    const float ratio = q.z / T.prev_inv.fov_dist;
    if (!(ratio > 0.0f)) return carry;
    const float fx = (((q.x / ratio) / T.cur.aspect + 1.0f) * 0.5f) * (float)w;
    const float fy = ((q.y / ratio + 1.0f) * 0.5f) * (float)h;
    if (!(fx > -1.0f && fx < (float)w && fy > -1.0f && fy < (float)h)) return carry;
    const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
    const int ix = (int)flx, iy = (int)fly;
    const float tx = fx - flx, ty = fy - fly;

    float S = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f, sv = 0.0f;
    for (int dy = 0; dy <= 1; dy++) {
        const int qy = iy + dy;
        if (qy < 0 || qy >= h) continue;
        const float by = dy ? ty : 1.0f - ty;
        for (int dx = 0; dx <= 1; dx++) {
            const int qx = ix + dx;
            if (qx < 0 || qx >= w) continue;
            const float b = by * (dx ? tx : 1.0f - tx);
            if (b == 0.0f) continue;
            const size_t k = (size_t)qy * w + qx;
            const float lq = T.h_len[k];
            const float sq = T.h_sigma[k];
            const float4_ cq = T.h_rgba[k];
            const float4_ gq = T.h_nd[k];
            if (!(lq > 0.0f) || !tp_finite(sq) || !dn_finite3(cq)) continue;
            if ((gq.w > 0.0f) != hit_p) continue;
            if (hit_p) {
                const float dt = gq.w - t_exp;
                if (!((dt < 0.0f ? -dt : dt) <= T.depth_tol * t_exp)) continue;
                if (!(dot(np, v3(gq.x, gq.y, gq.z)) >= T.normal_cos)) continue;
            }
            S = S + b;
            sr = sr + b * cq.x;
            sg = sg + b * cq.y;
            sb = sb + b * cq.z;
            sl = sl + b * lq;
            sv = sv + b * (sq * sq);
        }
    }
    if (!(S > T.min_weight)) return carry;
    const float hr = sr / S, hg = sg / S, hb = sb / S;
    const float len_h = sl / S;
    const float vh = rt_min(sv / S, DNV_VMAX);
    const float len = rt_min(len_h + 1.0f, T.max_len);
    const float a = 1.0f / len;
    const float k1 = 1.0f - a;
    const float v = rt_min((k1 * k1) * vh + a * (a * vc), DNV_VMAX);
    return TemporalOut{float4_{hr + a * (c.x - hr), hg + a * (c.y - hg), hb + a * (c.z - hb), 1.0f}, rt_sqrtf(v), len};
}

}  // namespace rtk
