// rt_adapt.h — adaptive progressions (include/rt_hip.h rt_progress_advance_adaptive): the per-tile
// decisions and arithmetic, written once for the gfx950 kernels (rt_adapt.hip) and the CPU build
// of the same code (rt_hostsim.cpp). Compiled like rt_noise.h (no contraction, IEEE division,
// rt_sqrtf), so the two builds give the same bits.
//
// An adaptive progression is a tracked one plus two int32 per 8x8 tile (rt_noise.h's tiles, over
// the shard's local rows, t = ty * tw + tx): tile_n[t], the samples every pixel of the tile has
// done, and tile_nA[t], how many of them fell in A passes. A tile's error is rt_noise.h's tile value
// computed with the tile's own counts (adapt_tile_args). A pass of s samples at threshold T:
//     fits    tile_n[t] + s <= total
//     over    passes < 2 (no estimate yet), or tile_err[t] > T (a NaN compares false)
//     active  fits and over            capped  an estimate exists, tile_err[t] > T, not fits
// Active tiles are listed in ascending t; tile_off is the exclusive prefix sum of their in-frame
// pixel counts, so the compact pixel list is a pure function of the state. Within a tile the
// pixels are in row-major order (rank of lane l = y * 8 + x among the tile's in-frame lanes).
#pragma once

#include "rt_noise.h"

namespace rtk {

constexpr int ADAPT_ACTIVE = 1, ADAPT_CAPPED = 2;

// What rt_noise.h's NoiseArgs holds for the whole frame, from one tile's counts.
RT_HD NoiseArgs adapt_tile_args(int n, int n_a, const NoiseArgs& frame)
{
    NoiseArgs A = frame;  // (threshold and the stat words are the frame's)
    A.n_all = (float)n;
    A.n_a = (float)n_a;
    A.k = rt_sqrtf((float)n_a / (float)(n - n_a));
    return A;
}

// estimate: the progression has done two passes, so err holds the tile's error.
RT_HD int adapt_flags(int n, int s, int total, bool estimate, float err, float threshold)
{
    const bool fits = n <= total && s <= total - n;
    const bool over = !estimate || err > threshold;
    if (fits) return over ? ADAPT_ACTIVE : 0;
    return estimate && over ? ADAPT_CAPPED : 0;
}

// Tile of pixel i of a shard of width w (tw tiles per tile row).
RT_HD int adapt_tile_of(int i, int w, int tw)
{
    const int y = i / w, x = i - y * w;
    return (y / NOISE_TILE) * tw + x / NOISE_TILE;
}

// The header a selection writes and rt_progress_advance_adaptive returns as info[8].
enum { AD_TILES_ACTIVE, AD_PIXELS, AD_CAPPED, AD_MIN, AD_MAX, AD_TILES, AD_WORDS = 8 };

}  // namespace rtk
