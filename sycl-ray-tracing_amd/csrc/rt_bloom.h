// rt_bloom.h — the bloom stage for linear frames (include/rt_hip.h rt_bloom): the energy above a
// luminance threshold is spread by a Gaussian pyramid (Burt and Adelson's REDUCE, a bilinear EXPAND)
// and added back before the tone-map. Written once for the gfx950 kernels (rt_bloom.hip) and the CPU
// build of the same code (rt_hostsim.cpp). Both are compiled with -ffp-contract=off and divide with
// IEEE division, as rt_firefly.h does, so the two builds give the same bits. No expf and no square
// root is evaluated.
//
// A w x h frame c, parameters threshold, knee, intensity, levels (validated: levels 1..8, the three
// floats finite and >= 0, knee <= threshold):
//   1  bright pass, per pixel. L = ff_lum(c) (rt_firefly.h: the same constants and operation order)
//        s = min(max((L - threshold) + knee, 0), knee + knee)
//        q = knee > 0 ? (s * s) / (4 * knee) : 0
//        e = max(q, L - threshold)
//        b = e > 0 ? c.rgb * (e / L) : 0        (f = e / L once, then three products)
//      A pixel whose rgb is not all finite, or whose L is not finite, gives b = 0. Because
//      0 <= knee <= threshold, e > 0 implies L > threshold - knee >= 0, and e / L lies in [0, 1].
//   2  reduce, k = 1..levels: w_k = (w_{k-1} + 1) / 2, h_k likewise; level 0 is b at frame size.
//        g_k(x, y) = sum over n of W[n] * row_n,  row_n = sum over m of W[m] * g_{k-1}(cx(2x + m), cy(2y + n))
//      m, n = -2..2, W = {0.0625, 0.25, 0.375, 0.25, 0.0625}, cx / cy clamp to the edge of level k-1.
//      The five row sums first, each in ascending m, then the column sum in ascending n; every sum is
//      bl_wsum5: five rounded products added left to right. One rounding sequence everywhere.
//   3  expand and accumulate: u_levels = g_levels; k = levels-1 .. 1: u_k = g_k + expand(u_{k+1}).
//      expand at (x, y) from a w' x h' level: xs = x >> 1, xn = clamp(xs + ((x & 1) ? 1 : -1), 0, w' - 1),
//      ys and yn likewise; row(yy) = 0.75 * g(xs, yy) + 0.25 * g(xn, yy); value = 0.75 * row(ys) + 0.25 * row(yn).
//   4  composite: B = expand(u_1) at frame size; scale = intensity / levels, divided once on the host
//      as a float; out.rgb = c.rgb + scale * B, out.a = c.a. A centre whose rgb is not all finite is
//      copied bit for bit, as the other stages do; its b is 0, so it does not leak into its neighbours.
//   5  layer (optional second output) = {scale * B, 0}, for a bad centre too.
// The pyramid's texels are float4 records with w = 0: one 16-B access per texel.
// Decisions the list above leaves open, made here:
//   a luminance that overflows   with finite rgb needs channels at the largest float and weights that sum
//                      above 1; should it happen, L is +inf and the pixel gives b = 0 (rule 1), and it still
//                      receives its neighbours' glow like any finite centre. A huge finite L is not special:
//                      at L = 3e38, e / L rounds to 1 and b = c.
//   overflow further on  is not caught: the reduce is an average and stays finite, but the sum over the
//                      levels or c + scale * B can pass the largest float and is then +/-inf, as the
//                      arithmetic gives.
//   a negative colour  with L <= threshold - knee gives b = 0. A pixel above the threshold with one negative
//                      channel spreads that channel as negative glow: nothing is clamped to 0.
//   intensity 0        scale is 0 and nothing is added: the term is the literal 0, not 0 * B (an infinite B
//                      would make it a NaN). The frame comes back equal to its input as values, the layer is 0.
//   intensity +inf     is refused with the other non-finite parameters (rt_capi_stages.cpp).
//   the sign of a zero a channel of -0 comes back as +0 when the term added is +0 (-0 + +0): equal as values,
//                      not as bits. Only a bad centre is copied bit for bit. Alpha is always copied.
//   nothing above threshold - knee: every b is +0, every level and B are +0, out = c + 0: the input as values.
#pragma once

#include "rt_firefly.h"

namespace rtk {

constexpr int BL_MAX_LEVELS = 8;
constexpr float BL_W0 = 0.0625f, BL_W1 = 0.25f, BL_W2 = 0.375f;  // W = {W0, W1, W2, W1, W0}

struct BloomArgs {
    int w, h, levels;
    float threshold, knee, scale;  // validated; scale = intensity / levels
    const float4_* in;
};

RT_HD int bl_half(int n) { return (n + 1) / 2; }
RT_HD int bl_clampi(int v, int hi) { return rt_mini(rt_maxi(v, 0), hi); }

// Texels of levels 1..levels of a w x h frame (the pyramid's size in float4 records).
RT_HD size_t bl_pyramid_texels(int w, int h, int levels)
{
    size_t n = 0;
    for (int k = 1; k <= levels; k++) {
        w = bl_half(w), h = bl_half(h);
        n += (size_t)w * h;
    }
    return n;
}

// Step 1: what pixel c hands to level 0.
RT_HD float4_ bl_bright(const BloomArgs& A, const float4_& c)
{
    const float L = ff_lum(c);
    if (!dn_finite3(c) || (rt_asuint(L) & 0x7f800000u) == 0x7f800000u) return float4_{0.0f, 0.0f, 0.0f, 0.0f};
    const float d = L - A.threshold;
    const float s = rt_min(rt_max(d + A.knee, 0.0f), A.knee + A.knee);
    const float q = A.knee > 0.0f ? (s * s) / (4.0f * A.knee) : 0.0f;
    const float e = rt_max(q, d);
    if (!(e > 0.0f)) return float4_{0.0f, 0.0f, 0.0f, 0.0f};
    const float f = e / L;
    return float4_{c.x * f, c.y * f, c.z * f, 0.0f};
}

// The one weighted sum of step 2, for a row of five taps and for the column of five row sums.
RT_HD float bl_wsum5(float a0, float a1, float a2, float a3, float a4)
{
    return (((BL_W0 * a0 + BL_W1 * a1) + BL_W2 * a2) + BL_W1 * a3) + BL_W0 * a4;
}
// (w rides along: it is 0 at level 0 and a sum of zeroes after. Summed, a texel is one whole 16-B record to
// the compiler, an LDS read of ds_read_b128; with w dropped the tile's reads become ds_read_b96, which the
// LDS serves in eight lane groups instead of four.)
RT_HD float4_ bl_wsum5(const float4_& a0, const float4_& a1, const float4_& a2, const float4_& a3, const float4_& a4)
{
    return float4_{bl_wsum5(a0.x, a1.x, a2.x, a3.x, a4.x), bl_wsum5(a0.y, a1.y, a2.y, a3.y, a4.y),
                   bl_wsum5(a0.z, a1.z, a2.z, a3.z, a4.z), bl_wsum5(a0.w, a1.w, a2.w, a3.w, a4.w)};
}

// A level in memory, and the frame seen through the bright pass (level 0, never stored): at(x, y)
// clamps to the edge. The LDS tile of rt_bloom.hip stages the same clamped texels.
struct BlLevel {
    const float4_* g;
    int w, h;
    RT_HD float4_ at(int x, int y) const { return g[(size_t)bl_clampi(y, h - 1) * w + bl_clampi(x, w - 1)]; }
};
struct BlFrame {
    const BloomArgs& A;
    RT_HD float4_ at(int x, int y) const
    {
        return bl_bright(A, A.in[(size_t)bl_clampi(y, A.h - 1) * A.w + bl_clampi(x, A.w - 1)]);
    }
};

// Step 2 for one texel (x, y) of the next level, straight from the source (hostsim, k_bloom_reduce_direct).
template <class F>
RT_HD float4_ bl_reduce_texel(const F& f, int x, int y)
{
    float4_ row[5];
#pragma unroll
    for (int n = 0; n < 5; n++) {
        const int yy = 2 * y + n - 2, x2 = 2 * x;
        row[n] = bl_wsum5(f.at(x2 - 2, yy), f.at(x2 - 1, yy), f.at(x2, yy), f.at(x2 + 1, yy), f.at(x2 + 2, yy));
    }
    return bl_wsum5(row[0], row[1], row[2], row[3], row[4]);
}

RT_HD float4_ bl_mix(const float4_& a, const float4_& b)
{
    return float4_{0.75f * a.x + 0.25f * b.x, 0.75f * a.y + 0.25f * b.y, 0.75f * a.z + 0.25f * b.z, 0.0f};
}

// Step 3's expand at (x, y) of the finer level, from the coarser level u.
RT_HD float4_ bl_expand(const BlLevel& u, int x, int y)
{
    const int xs = x >> 1, xn = bl_clampi(xs + ((x & 1) ? 1 : -1), u.w - 1);
    const int ys = y >> 1, yn = bl_clampi(ys + ((y & 1) ? 1 : -1), u.h - 1);
    const float4_* r0 = u.g + (size_t)ys * u.w;
    const float4_* r1 = u.g + (size_t)yn * u.w;
    return bl_mix(bl_mix(r0[xs], r0[xn]), bl_mix(r1[xs], r1[xn]));
}

// u_k(x, y) = g_k(x, y) + expand(u_{k+1})(x, y)
RT_HD float4_ bl_accumulate(const float4_& g, const BlLevel& u, int x, int y)
{
    const float4_ e = bl_expand(u, x, y);
    return float4_{g.x + e.x, g.y + e.y, g.z + e.z, 0.0f};
}

// Steps 4 and 5 for one pixel: the composited pixel, and the layer through `layer`.
RT_HD float4_ bl_composite(const BloomArgs& A, const float4_& c, const BlLevel& u1, int x, int y, float4_& layer)
{
    layer = float4_{0.0f, 0.0f, 0.0f, 0.0f};
    if (A.scale > 0.0f) {
        const float4_ B = bl_expand(u1, x, y);
        layer = float4_{A.scale * B.x, A.scale * B.y, A.scale * B.z, 0.0f};
    }
    if (!dn_finite3(c)) return c;
    return float4_{c.x + layer.x, c.y + layer.y, c.z + layer.z, c.w};
}

}  // namespace rtk
