// rt_display.h — the display stage (include/rt_hip.h rt_display, rt_progress_resolve_linear):
// the per-pixel arithmetic that takes a linear radiance frame to the displayed one, written
// once for the gfx950 kernels (rt_display.hip) and the CPU build of the same code
// (rt_hostsim.cpp). Both are compiled with -ffp-contract=off and use rt_libm's expf / powf,
// so the two builds give the same bits.
//
// The render ends a pixel in two parts (rt_wave.h finish_pixel, tonemap_pixel): the linear
// frame is what the framebuffer holds between them, the reference's hdrColor
// (render_kernel.cpp:173). display_pixel is tonemap_pixel's operations in its order with
// the exposure and 1 / gamma as arguments where that function has the literals 1.5f and
// 1.0f / 2.2f: at (1.5f, 1.0f / 2.2f) it gives tonemap_pixel's words. tonemap_pixel,
// resolve_pixel and tonemap_into themselves stay as they are (the render's kernels compile
// from them).
#pragma once

#include "rt_device.h"
#include "rt_libm.h"

namespace rtk {

// rgb: (1 - expf(-x exposure)) ^ inv_gamma; alpha: 1 - (-(a + 0)) exposure (render_kernel.cpp:171-180)
RT_HD float4_ display_pixel(float4_ linear, float exposure, float inv_gamma)
{
    float4_ px = linear;
    float* v = &px.x;
    const float a = v[3] + 0.0f;
    v[3] = 1.0f + (-((-a) * exposure));
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float e = rt_expf((-v[c]) * exposure);
        float tm = 1.0f + (-e);
        v[c] = rt_powf(tm, inv_gamma);
    }
    return px;
}

// A progression's linear frame after `done` samples: resolve_pixel's true division and sum
// (rt_wave.h), stopped before its alpha and exposure lines. The alpha is the base's.
RT_HD float4_ resolve_linear_pixel(const float4_& base, const float4_& state, int done)
{
    const float k = (float)done;
    float r = state.x, g = state.y, b = state.z;
    r /= k;
    g /= k;
    b /= k;
    float4_ px = base;
    px.x += r;
    px.y += g;
    px.z += b;
    return px;
}

// One channel of write_image_png's 8-bit conversion (image_io.cpp:156-177): x * 255, clamp
// to [0, 255] with image_io.cpp's clamp (NaN passes through it), float -> unsigned char as
// g++ on x86-64 converts it (cvttss2si, low byte: rt_f2i).
RT_HD unsigned char to_u8(float x)
{
    float s = x * 255;
    if (s < 0.0f) s = 0.0f;
    else if (s > 255.0f) s = 255.0f;
    return (unsigned char)rt_f2i(s);
}

// The four bytes r, g, b, a of a pixel in memory order, as one little-endian word.
RT_HD uint32_t pack_rgba8(const float4_& px)
{
    return (uint32_t)to_u8(px.x) | ((uint32_t)to_u8(px.y) << 8) | ((uint32_t)to_u8(px.z) << 16) |
           ((uint32_t)to_u8(px.w) << 24);
}

}  // namespace rtk
