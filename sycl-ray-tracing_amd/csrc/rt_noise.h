// rt_noise.h — the noise estimate of a tracked progression (include/rt_hip.h
// rt_progress_noise_track, rt_progress_noise): the per-pixel arithmetic, written once for the
// gfx950 kernels (rt_noise.hip) and the CPU build of the same code (rt_hostsim.cpp). Both are
// compiled with -ffp-contract=off, divide with IEEE division and take rt_sqrtf, so the two
// builds give the same bits.
//
// A tracked progression keeps `half`, the rgb sum of the samples its A passes (the even-numbered
// ones) rendered, beside the state's sum of all of them. The fold is in two parts around an A
// pass, with no snapshot of the state:
//     before the pass   half.c = half.c - state.c
//     after the pass    half.c = half.c + state.c
// (fold_pixel with sign -1 and +1). The fourth word of half is written as 0 by both.
//
// Per pixel, with N = nA + nB samples in the state and nA of them in half:
//     m.c = state.c / (float)N        a.c = half.c / (float)nA
//     d   = (|m.r - a.r| + |m.g - a.g|) + |m.b - a.b|
//     e   = (k * d) / rt_sqrtf(0.01f + ((m.r + m.g) + m.b)),   k = rt_sqrtf((float)nA / (float)nB)
// m - a = (nB / N)(b - a) for the B half's mean b, so k brings its variance to that of the
// frame's mean whatever the split.
//
// A tile is 8x8 pixels of the shard's local rows; lane l of a wave owns pixel (8tx + l % 8,
// 8ty + l / 8). Lanes outside the frame and lanes whose e is not finite contribute 0; the 64
// values are summed by the pairwise tree (level j adds elements l and l ^ (1 << j)) and divided
// by the tile's in-frame pixel count.
#pragma once

#include "rt_device.h"

namespace rtk {

constexpr int NOISE_TILE = 8;  // pixels per tile side: one wave64 per tile

// The arguments of a noise query the host works out once (rt_capi_host.cpp).
struct NoiseArgs {
    float n_all, n_a;  // (float)N, (float)nA
    float k;           // rt_sqrtf((float)nA / (float)nB)
    float threshold;
    int samples_a, samples_b, passes;  // the stat words 4..6
};

RT_HD float4_ fold_pixel(const float4_& half, const float4_& state, bool add)
{
    float4_ h;
    h.x = add ? half.x + state.x : half.x - state.x;
    h.y = add ? half.y + state.y : half.y - state.y;
    h.z = add ? half.z + state.z : half.z - state.z;
    h.w = 0.0f;
    return h;
}

RT_HD float noise_abs(float x) { return rt_asfloat(rt_asuint(x) & 0x7fffffffu); }

RT_HD bool noise_finite(float x) { return (rt_asuint(x) & 0x7f800000u) != 0x7f800000u; }

RT_HD float noise_pixel(const float4_& state, const float4_& half, const NoiseArgs& A)
{
    const float mr = state.x / A.n_all, mg = state.y / A.n_all, mb = state.z / A.n_all;
    const float ar = half.x / A.n_a, ag = half.y / A.n_a, ab = half.z / A.n_a;
    const float d = (noise_abs(mr - ar) + noise_abs(mg - ag)) + noise_abs(mb - ab);
    return (A.k * d) / rt_sqrtf(0.01f + ((mr + mg) + mb));
}

// In-frame pixels of tile (tx, ty) of a w x rows shard.
RT_HD int noise_tile_count(int tx, int ty, int w, int rows)
{
    const int cw = w - NOISE_TILE * tx < NOISE_TILE ? w - NOISE_TILE * tx : NOISE_TILE;
    const int ch = rows - NOISE_TILE * ty < NOISE_TILE ? rows - NOISE_TILE * ty : NOISE_TILE;
    return cw * ch;
}

// The pairwise tree over a tile's 64 values (v is overwritten): v[0::2] + v[1::2] six times.
inline float noise_tree64(float* v)
{
    for (int n = 32; n >= 1; n >>= 1)
        for (int i = 0; i < n; i++) v[i] = v[2 * i] + v[2 * i + 1];
    return v[0];
}

}  // namespace rtk
