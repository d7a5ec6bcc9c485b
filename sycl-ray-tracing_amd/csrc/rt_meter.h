// rt_meter.h — exposure metering for linear frames (include/rt_hip.h rt_meter): every pixel's
// luminance is classified into a 256-bin log histogram, eight bins per octave over [2^-20, 2^12),
// plus seven stat words. Written once for the gfx950 kernels (rt_meter.hip) and the CPU build of
// the same code (rt_hostsim.cpp). Every object is compiled with -ffp-contract=off, so the
// luminance has the same bits in both builds; everything behind it is integer arithmetic on those
// bits, so the histogram is the same in any execution order.
//
// Pixel c of the frame (alpha ignored):
//   1  L = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b: rt_firefly.h's ff_lum, shared
//   2  r, g or b not finite, or L not finite (finite channels can sum past FLT_MAX): nonfinite
//   3  else L <= 0 (which -0 is): nonpositive
//   4  else k = bits(L) >> 20: the 8 exponent bits and the top 3 mantissa bits, so k counts
//      eighth-octaves: k = 8 * (e + 127) + m for L = 2^e * (1 + (m + f) / 8), 0 <= f < 1.
//      bin = clamp(k - 856, 0, 255); 856 = 8 * (127 - 20), the bin of 2^-20; 1111 = 856 + 255 ends
//      just below 2^12. k < 856 (denormals too) counts `under` and lands in bin 0, k > 1111 counts
//      `over` and lands in bin 255. `counted` goes up, bits(L) is folded into max_bits and min_bits.
// No libm call: log2f would differ between glibc and the device's, at the bin edges of all places;
// the bits are the logarithm already, to an eighth of an octave, and cost one shift.
#pragma once

#include "rt_firefly.h"

namespace rtk {

constexpr int MT_BINS = 256;
constexpr int MT_WORDS = 264;  // rt_meter_hist: bins, then the words below
constexpr int MT_COUNTED = 256, MT_UNDER = 257, MT_OVER = 258, MT_NONPOSITIVE = 259, MT_NONFINITE = 260, MT_MAX_BITS = 261,
              MT_MIN_BITS = 262;
constexpr uint32_t MT_K0 = 856, MT_K1 = 1111;  // k of bin 0 and of bin 255

// What a pixel is: bin >= 0 with its luminance's bits, or one of the two classes that are not binned.
constexpr int MT_IS_NONPOSITIVE = -1, MT_IS_NONFINITE = -2;
struct MeterPixel {
    int bin;
    uint32_t bits;  // bits(L); k = bits >> 20 says under / over
};

RT_HD MeterPixel meter_pixel(const float4_& c)
{
    const float L = ff_lum(c);
    const uint32_t bits = rt_asuint(L);
    if (!dn_finite3(c) || (bits & 0x7f800000u) == 0x7f800000u) return MeterPixel{MT_IS_NONFINITE, bits};
    if (L <= 0.0f) return MeterPixel{MT_IS_NONPOSITIVE, bits};
    const uint32_t k = bits >> 20;
    return MeterPixel{k < MT_K0 ? 0 : k > MT_K1 ? MT_BINS - 1 : (int)(k - MT_K0), bits};
}

// One pixel into a histogram of MT_WORDS words (hostsim; min_bits seeded with 0xFFFFFFFF).
inline void meter_count(uint32_t* hist, const float4_& c)
{
    const MeterPixel m = meter_pixel(c);
    if (m.bin == MT_IS_NONFINITE) {
        hist[MT_NONFINITE]++;
        return;
    }
    if (m.bin == MT_IS_NONPOSITIVE) {
        hist[MT_NONPOSITIVE]++;
        return;
    }
    const uint32_t k = m.bits >> 20;
    hist[m.bin]++;
    hist[MT_COUNTED]++;
    if (k < MT_K0) hist[MT_UNDER]++;
    if (k > MT_K1) hist[MT_OVER]++;
    if (m.bits > hist[MT_MAX_BITS]) hist[MT_MAX_BITS] = m.bits;
    if (m.bits < hist[MT_MIN_BITS]) hist[MT_MIN_BITS] = m.bits;
}

}  // namespace rtk
