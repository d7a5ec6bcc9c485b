// rt_digest.h — the digest that holds a build of rt_libm.h to glibc over whole float sweeps
// (tests/golden/libm_digests.npz), written once for its three evaluators: glibc and the host
// build of rt_libm.h in tests/native/libm_check.cpp, and the gfx950 build in rt_probe.hip
// (k_libm_digest). TEST ONLY: no render includes this file.
//
// A sweep is a function code, a fixed second argument (its bits) and a stride; index i is the
// bit pattern of the swept argument. The 2^32 indices form 1024 blocks of 2^22, and
//   digest[b] = sum over the block's indices i with i % stride == 0 of
//               mix(((uint64)canon(f(i)) << 32) | i)          (mod 2^64)
// The sum makes the order of evaluation irrelevant; the index inside the mix keeps two
// results that swapped places from cancelling.
#pragma once

#include "rt_libm.h"

namespace rtdigest {

constexpr int BLOCK_BITS = 22;
constexpr int BLOCKS = 1 << (32 - BLOCK_BITS);  // 1024

// the sweeps' function codes (x = float(i), p = the fixed argument)
enum Fn {
    FN_EXPF = 0,
    FN_SINF = 1,
    FN_COSF = 2,
    FN_ACOSF = 3,
    FN_ASINF = 4,
    FN_SQRTF = 5,
    FN_SINCOSF_S = 6,  // the sine result of rt_sincosf(x), against glibc sinf
    FN_SINCOSF_C = 7,  // the cosine result of rt_sincosf(x), against glibc cosf
    FN_POWF_Y = 8,     // powf(x, p)
    FN_POWF_X = 9,     // powf(p, x)
    FN_ATAN2F_Y = 10,  // atan2f(p, x)
    FN_ATAN2F_X = 11,  // atan2f(x, p)
    FN_COUNT = 12
};

// every NaN is one NaN; every other pattern is kept, the sign of zero included
RT_HD uint32_t canon(float r)
{
    const uint32_t u = rt_asuint(r);
    return (u & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : u;
}

RT_HD uint64_t mix(uint64_t v)
{
    v *= 0x9E3779B97F4A7C15ull;
    v ^= v >> 29;
    v *= 0xBF58476D1CE4E5B9ull;
    v ^= v >> 32;
    return v;
}

// one index's term of its block's sum
RT_HD uint64_t term(uint32_t i, float r) { return mix(((uint64_t)canon(r) << 32) | i); }

// rt_libm's value of sweep FN at index i (device: after rtlibm::lds_tables_init())
template <int FN>
RT_HD float eval(uint32_t i, float p)
{
    const float x = rt_asfloat(i);
    float s, c;
    switch (FN) {
        case FN_EXPF: return rt_expf(x);
        case FN_SINF: return rt_sinf(x);
        case FN_COSF: return rt_cosf(x);
        case FN_ACOSF: return rt_acosf(x);
        case FN_ASINF: return rt_asinf(x);
        case FN_SQRTF: return rt_sqrtf(x);
        case FN_SINCOSF_S: rt_sincosf(x, s, c); return s;
        case FN_SINCOSF_C: rt_sincosf(x, s, c); return c;
        case FN_POWF_Y: return rt_powf(x, p);
        case FN_POWF_X: return rt_powf(p, x);
        case FN_ATAN2F_Y: return rt_atan2f(p, x);
        default: return rt_atan2f(x, p);
    }
}

}  // namespace rtdigest
