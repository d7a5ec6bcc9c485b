// rt_firefly.h — firefly rejection for linear frames (include/rt_hip.h rt_firefly): a pixel's
// luminance is limited to a multiple of a high rank of its neighbours' luminances, and its colour
// and noise figure are scaled together. Written once for the gfx950 kernels (rt_firefly.hip) and
// the CPU build of the same code (rt_hostsim.cpp). Both are compiled with -ffp-contract=off and
// divide with IEEE division, as rt_dnv.h and rt_temporal.h do, so the two builds give the same
// bits. No expf and no square root is evaluated.
//
// Pixel p = (x, y) of a w x h frame; c = rgba_in[p], s = sigma_in[p] (0 without a sigma_in):
//   1  L(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b, the Rec. 709 weights as floats, the
//      three products rounded, then the two sums in that order
//   2  the neighbours are the (2R + 1)^2 - 1 pixels q != p with |q.x - p.x| <= R and |q.y - p.y| <= R,
//      R = radius, visited dy outer, dx inner, both ascending. A neighbour outside the image or whose
//      rgb is not all finite is dropped.
//   3  M = the rank-th largest L(q) over the neighbours kept; fewer than `rank` of them: p is untouched
//   4  limit = gain * M + floor
//   5  clamped when c.rgb is all finite, limit > 0 and L(c) > limit:
//        f = limit / L(c), out = {f c.r, f c.g, f c.b, c.a}, sigma_out = f s, scale_out = f
//      untouched otherwise: out = c and sigma_out = s bit for bit, scale_out = 1
// A centre whose rgb is not finite is kept as it is, with scale 1: rt_denoise_var's rule for such a
// centre (dn_filter_pixel returns it unfiltered), so the chain hands it on unchanged.
// Decisions the list above leaves open, made here:
//   a limit not > 0    leaves p untouched: f would be zero or negative, and a scale is in (0, 1]. Neighbours
//                      of zero or negative luminance therefore limit nothing at floor 0; a spike over black
//                      is what `floor` is for. A NaN limit (gain 0 times an infinite M, or infinities of both
//                      signs) fails both comparisons and leaves p untouched as well.
//   a negative centre  luminance is never above a limit > 0: untouched. Negative colours count as neighbours
//                      with the luminance the arithmetic gives them.
//   the ranked value   of a neighbour kept is max(L(q), -FLT_MAX): three huge negative channels can sum to
//                      -inf, which is the value a dropped neighbour takes in the insertion below; raised to
//                      the most negative finite float the neighbour still counts towards `rank`. A sum that
//                      overflows to +inf stays +inf: M and the limit are then infinite and nothing is clamped.
//   a clamped sigma    that is a NaN or an infinity is copied bit for bit: scaled by f in (0, 1] a NaN stays a
//                      NaN and an infinity an infinity, and the copy keeps a NaN's payload the same in both builds.
//   underflow          f is what the division gives: limit / L(c) below 2^-150 is 0 and the pixel goes black.
//   gain = +inf        limit is +inf or a NaN for every M: the identity. floor = +/-inf likewise clamps nothing
//                      or is met by the limit > 0 rule.
//   alpha              is copied; it plays no part.
// The selection: t[0..K-1], K = rank, start at -inf; each neighbour's value v is passed down the K
// registers with one comparison per register, hi = t[k] < v ? v : t[k] (rt_max), lo the other one
// (what rt_min gives but for the sign of a zero among equals, which no output depends on), t[k] = hi,
// v = lo. No branch, no data-dependent loop, no sort: a dropped neighbour's -inf leaves every register
// as it was, and t[K-1] > -inf says that K neighbours were kept. K is a template argument picked by
// a switch on the caller's `rank`, uniform over the call, so that rank 2 does not pay for eight registers.
#pragma once

#include "rt_denoise.h"

namespace rtk {

constexpr float FF_LR = 0.2126f, FF_LG = 0.7152f, FF_LB = 0.0722f;
constexpr float FF_FMAX = 3.4028234663852886e38f;  // the largest finite float
constexpr int FF_MAX_RANK = 8;

struct FireflyArgs {
    int w, h;
    int radius, rank;  // validated: 1..2, 1..FF_MAX_RANK
    float gain, floor;
    const float4_* in;
    const float* sigma;  // (null: no sigma_in)
};

struct FireflyOut {
    float4_ rgba;
    float sigma, scale;
};

RT_HD float ff_neg_inf() { return rt_asfloat(0xff800000u); }

RT_HD float ff_lum(const float4_& c) { return (FF_LR * c.x + FF_LG * c.y) + FF_LB * c.z; }

// What a pixel contributes as a neighbour: -inf when dropped, else its luminance, at least -FLT_MAX.
RT_HD float ff_rank_value(const float4_& c) { return dn_finite3(c) ? rt_max(ff_lum(c), -FF_FMAX) : ff_neg_inf(); }

// Neighbours straight from the frame (hostsim, k_firefly_direct). The LDS tile of rt_firefly.hip
// answers value(x, y) the same way from the values it staged.
struct FfDirect {
    const FireflyArgs& A;
    RT_HD float value(int qx, int qy) const
    {
        if (qx < 0 || qx >= A.w || qy < 0 || qy >= A.h) return ff_neg_inf();
        return ff_rank_value(A.in[(size_t)qy * A.w + qx]);
    }
};

template <int R, int K, class F>
RT_HD float ff_rank_of_neighbours(int x, int y, const F& f)
{
    float t[K];
#pragma unroll
    for (int k = 0; k < K; k++) t[k] = ff_neg_inf();
#pragma unroll
    for (int dy = -R; dy <= R; dy++) {
#pragma unroll
        for (int dx = -R; dx <= R; dx++) {
            if (dx == 0 && dy == 0) continue;
            float v = f.value(x + dx, y + dy);
#pragma unroll
            for (int k = 0; k < K; k++) {
                const bool lt = t[k] < v;
                const float hi = lt ? v : t[k];
                v = lt ? t[k] : v;
                t[k] = hi;
            }
        }
    }
    return t[K - 1];
}

template <int R, class F>
RT_HD float ff_rank_switch(int rank, int x, int y, const F& f)
{
    switch (rank) {
    case 1: return ff_rank_of_neighbours<R, 1>(x, y, f);
    case 2: return ff_rank_of_neighbours<R, 2>(x, y, f);
    case 3: return ff_rank_of_neighbours<R, 3>(x, y, f);
    case 4: return ff_rank_of_neighbours<R, 4>(x, y, f);
    case 5: return ff_rank_of_neighbours<R, 5>(x, y, f);
    case 6: return ff_rank_of_neighbours<R, 6>(x, y, f);
    case 7: return ff_rank_of_neighbours<R, 7>(x, y, f);
    default: return ff_rank_of_neighbours<R, 8>(x, y, f);
    }
}

// One output pixel. c and s are p's own record and sigma (the caller has loaded them once); F as
// above, asked for every position of the neighbourhood, inside the image or not.
template <int R, class F>
RT_HD FireflyOut firefly_pixel(const FireflyArgs& A, int x, int y, const float4_& c, float s, const F& f)
{
    const float M = ff_rank_switch<R>(A.rank, x, y, f);
    const float limit = A.gain * M + A.floor;
    const float Lp = ff_lum(c);
    // (M > -inf: `rank` neighbours were kept)
    if (!(M > ff_neg_inf()) || !dn_finite3(c) || !(limit > 0.0f) || !(Lp > limit)) return FireflyOut{c, s, 1.0f};
    const float fs = limit / Lp;
    const bool s_finite = (rt_asuint(s) & 0x7f800000u) != 0x7f800000u;
    return FireflyOut{float4_{fs * c.x, fs * c.y, fs * c.z, c.w}, s_finite ? fs * s : s, fs};
}

}  // namespace rtk
