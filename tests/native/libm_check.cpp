// libm_check — compares rt_libm.h (the device libm restatement, compiled for
// the host here) against this machine's glibc, bit for bit.
//
// usage: libm_check [stride] [function]
//   stride 1 = exhaustive over all 2^32 float inputs (about 10 s/function
//   on 8 threads); the pytest CPU suite uses a larger stride.
//   function: expf sinf cosf sincosf acosf asinf powf5 powfg powfy atan2f, and the digest's other
//   sweeps: sqrtf, powfys (every x at the six other fixed exponents), atan2fx (y swept at fixed x).
// Exit status 0 iff no mismatch. NaN outputs match any NaN (the kernel only
// ever compares NaN, never inspects its payload).
//
// The digest modes (rt_digest.h; tools/gen_golden_libm.py writes tests/golden/libm_digests.npz
// from them, tests/test_numerics.py and tests/test_gpu_libm.py read it):
//   libm_check --list                          the sweep table: name, function code, fixed argument's bits, stride
//   libm_check --digest SWEEP                  1024 lines "block glibc's word rt_libm's word" (hex)
//   libm_check --digest-blocks SWEEP b0,b1,..  the same for the named blocks
//   libm_check --digest-values IN FIRST        one word: the sum of the terms of the raw float32 results in
//                                              IN, taken as f(FIRST), f(FIRST + 1), ...
//   libm_check --eval SWEEP IN OUT             glibc's results for the raw float32 swept arguments in IN
//                                              (the sweep's fixed argument in its place), raw float32 to OUT
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <string>
#include <vector>

#include "rt_digest.h"
#include "rt_libm.h"

static inline bool same(float a, float b)
{
    if (std::isnan(a) && std::isnan(b)) return true;
    return rt_asuint(a) == rt_asuint(b);
}

template <class F, class G>
static long check_unary(const char* name, long stride, F ref, G mine)
{
    long bad = 0, first = -1;
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (long i = 0; i < (1L << 32); i += stride) {
        const float x = rt_asfloat((uint32_t)i);
        volatile float xv = x;
        const float r = ref(xv), m = mine(x);
        if (!same(r, m)) {
            bad++;
#pragma omp critical
            if (first < 0) {
                first = i;
                std::printf("  %s(%a [0x%08x]) glibc=%a mine=%a\n", name, x, (uint32_t)i, r, m);
            }
        }
    }
    std::printf("%-8s stride %-6ld mismatches %ld\n", name, stride, bad);
    return bad;
}

static long check_atan2(long stride)
{
    // Structured pairs: every x from a strided sweep against y drawn from a
    // set covering each binade, signs, zeros, infinities and NaN, plus the
    // pairs that occur in the kernel (unit-vector components).
    long bad = 0;
    const float ys[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, -0.3f, 1e-30f, -1e-30f, 3e30f, -7e20f,
                        INFINITY, -INFINITY, NAN, 0x1p-149f, -0x1p-126f, 0.70710677f, 2.4375f, -1.1875f};
    for (float y : ys) {
#pragma omp parallel for reduction(+ : bad) schedule(static)
        for (long i = 0; i < (1L << 32); i += stride * 8) {
            const float x = rt_asfloat((uint32_t)i);
            volatile float xv = x, yv = y;
            const float r = atan2f(yv, xv), m = rt_atan2f(y, x);
            if (!same(r, m)) bad++;
        }
    }
    // random unit-ish pairs
    uint32_t s = 12345;
    long bad2 = 0;
    for (long k = 0; k < 20000000 / (stride > 64 ? 8 : 1); k++) {
        s ^= s << 13; s ^= s >> 17; s ^= s << 5;
        uint32_t t = s * 2654435761u;
        const float y = (float)((int32_t)s) * 0x1p-31f, x = (float)((int32_t)t) * 0x1p-31f;
        volatile float xv = x, yv = y;
        if (!same(atan2f(yv, xv), rt_atan2f(y, x))) bad2++;
    }
    std::printf("%-8s stride %-6ld mismatches %ld (+%ld random)\n", "atan2f", stride, bad, bad2);
    return bad + bad2;
}

// ------------------------------------------------------------------ the sweeps (rt_digest.h)
struct Sweep {
    std::string name;
    int fn;
    uint32_t param;  // the fixed argument's bits (0 where there is none)
    int stride;
};

// the fixed arguments of the two-argument sweeps
static const float POW_YS[] = {5.0f, 1.0f / 2.2f, 1.0f / 2.4f, 1.0f / 1.8f, 1.0f, 0.5f, 2.0f, 3.0f};
static const float POW_XS[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, -2.0f, 3.7f, INFINITY, -INFINITY, NAN, 0x1p-140f, -0x1p-140f};
static const float ATAN2_FIXED[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, -0.3f, 1e-30f, -1e-30f, 3e30f, -7e20f,
                                    INFINITY, -INFINITY, NAN, 0x1p-149f, -0x1p-126f, 0.70710677f, 2.4375f, -1.1875f};

static std::vector<Sweep> sweep_table()
{
    using namespace rtdigest;
    std::vector<Sweep> t = {{"expf", FN_EXPF, 0, 1},   {"sinf", FN_SINF, 0, 1},           {"cosf", FN_COSF, 0, 1},
                            {"acosf", FN_ACOSF, 0, 1}, {"asinf", FN_ASINF, 0, 1},         {"sqrtf", FN_SQRTF, 0, 1},
                            {"sincosf.s", FN_SINCOSF_S, 0, 1}, {"sincosf.c", FN_SINCOSF_C, 0, 1}};
    int k = 0;
    for (float y : POW_YS) t.push_back({"powf.y" + std::to_string(k++), FN_POWF_Y, rt_asuint(y), 1});
    k = 0;
    for (float x : POW_XS) t.push_back({"powf.x" + std::to_string(k++), FN_POWF_X, rt_asuint(x), 4});
    k = 0;
    for (float y : ATAN2_FIXED) t.push_back({"atan2f.y" + std::to_string(k++), FN_ATAN2F_Y, rt_asuint(y), 8});
    k = 0;
    for (float x : ATAN2_FIXED) t.push_back({"atan2f.x" + std::to_string(k++), FN_ATAN2F_X, rt_asuint(x), 8});
    return t;
}

static float glibc_eval(int fn, uint32_t i, float p)
{
    using namespace rtdigest;
    volatile float x = rt_asfloat(i), pv = p;
    switch (fn) {
        case FN_EXPF: return expf(x);
        case FN_SINF: case FN_SINCOSF_S: return sinf(x);
        case FN_COSF: case FN_SINCOSF_C: return cosf(x);
        case FN_ACOSF: return acosf(x);
        case FN_ASINF: return asinf(x);
        case FN_SQRTF: return sqrtf(x);
        case FN_POWF_Y: return powf(x, pv);
        case FN_POWF_X: return powf(pv, x);
        case FN_ATAN2F_Y: return atan2f(pv, x);
        default: return atan2f(x, pv);
    }
}

typedef float (*RtEval)(uint32_t, float);
static const RtEval RT_EVAL[rtdigest::FN_COUNT] = {
    rtdigest::eval<0>, rtdigest::eval<1>, rtdigest::eval<2>, rtdigest::eval<3>, rtdigest::eval<4>,  rtdigest::eval<5>,
    rtdigest::eval<6>, rtdigest::eval<7>, rtdigest::eval<8>, rtdigest::eval<9>, rtdigest::eval<10>, rtdigest::eval<11>};

// glibc's and rt_libm's digest words of the named blocks, in chunks of 2^16 indices
static void digest_blocks(const Sweep& sw, const std::vector<int>& blocks, std::vector<uint64_t>& g, std::vector<uint64_t>& m)
{
    const int CH = 1 << (rtdigest::BLOCK_BITS - 16);
    const long tasks = (long)blocks.size() * CH;
    std::vector<uint64_t> pg(tasks), pm(tasks);
    const float p = rt_asfloat(sw.param);
    const RtEval mine = RT_EVAL[sw.fn];
#pragma omp parallel for schedule(dynamic, 4)
    for (long t = 0; t < tasks; t++) {
        const uint32_t base = ((uint32_t)blocks[t / CH] << rtdigest::BLOCK_BITS) + ((uint32_t)(t % CH) << 16);
        uint64_t sg = 0, sm = 0;
        for (uint32_t k = 0; k < (1u << 16); k += (uint32_t)sw.stride) {
            const uint32_t i = base + k;
            sg += rtdigest::term(i, glibc_eval(sw.fn, i, p));
            sm += rtdigest::term(i, mine(i, p));
        }
        pg[t] = sg;
        pm[t] = sm;
    }
    g.assign(blocks.size(), 0);
    m.assign(blocks.size(), 0);
    for (long t = 0; t < tasks; t++) {
        g[t / CH] += pg[t];
        m[t / CH] += pm[t];
    }
}

// a sweep in the ordinary mode: every mult-th index of the sweep's own
static long check_sweep(const Sweep& sw, long mult)
{
    long bad = 0, first = -1;
    const float p = rt_asfloat(sw.param);
    const RtEval mine = RT_EVAL[sw.fn];
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (long i = 0; i < (1L << 32); i += mult * sw.stride) {
        const float r = glibc_eval(sw.fn, (uint32_t)i, p), m = mine((uint32_t)i, p);
        if (!same(r, m)) {
            bad++;
#pragma omp critical
            if (first < 0) {
                first = i;
                std::printf("  %s [fixed 0x%08x] at 0x%08x glibc=%a mine=%a\n", sw.name.c_str(), sw.param, (uint32_t)i, r, m);
            }
        }
    }
    std::printf("%-10s stride %-6ld mismatches %ld\n", sw.name.c_str(), mult * sw.stride, bad);
    return bad;
}

static bool read_floats(const char* path, std::vector<float>& v)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f) / 4;
    std::fseek(f, 0, SEEK_SET);
    v.resize(n);
    const bool ok = std::fread(v.data(), 4, n, f) == (size_t)n;
    std::fclose(f);
    return ok;
}

static int digest_main(int argc, char** argv)
{
    const std::vector<Sweep> table = sweep_table();
    const std::string mode = argv[1];
    if (mode == "--list") {
        for (const Sweep& s : table) std::printf("%s %d 0x%08x %d\n", s.name.c_str(), s.fn, s.param, s.stride);
        return 0;
    }
    if (mode == "--digest-values" && argc == 4) {
        std::vector<float> v;
        if (!read_floats(argv[2], v)) return 2;
        const uint32_t first = (uint32_t)std::strtoul(argv[3], nullptr, 0);
        uint64_t s = 0;
        for (size_t k = 0; k < v.size(); k++) s += rtdigest::term(first + (uint32_t)k, v[k]);
        std::printf("%016llx\n", (unsigned long long)s);
        return 0;
    }
    const Sweep* sw = nullptr;
    for (const Sweep& s : table)
        if (argc > 2 && s.name == argv[2]) sw = &s;
    if (!sw) {
        std::fprintf(stderr, "libm_check %s: no such sweep (see --list)\n", mode.c_str());
        return 2;
    }
    if (mode == "--eval" && argc == 5) {
        std::vector<float> v;
        if (!read_floats(argv[3], v)) return 2;
        for (float& x : v) x = glibc_eval(sw->fn, rt_asuint(x), rt_asfloat(sw->param));
        FILE* f = std::fopen(argv[4], "wb");
        if (!f) return 2;
        const bool ok = std::fwrite(v.data(), 4, v.size(), f) == v.size();
        return std::fclose(f) == 0 && ok ? 0 : 2;
    }
    std::vector<int> blocks;
    if (mode == "--digest" && argc == 3) {
        for (int b = 0; b < rtdigest::BLOCKS; b++) blocks.push_back(b);
    } else if (mode == "--digest-blocks" && argc == 4) {
        for (const char* s = argv[3]; *s;) {
            char* e;
            const long b = std::strtol(s, &e, 10);
            if (e == s || b < 0 || b >= rtdigest::BLOCKS) return 2;
            blocks.push_back((int)b);
            s = *e == ',' ? e + 1 : e;
        }
    } else {
        std::fprintf(stderr, "libm_check: bad arguments to %s\n", mode.c_str());
        return 2;
    }
    std::vector<uint64_t> g, m;
    digest_blocks(*sw, blocks, g, m);
    for (size_t k = 0; k < blocks.size(); k++)
        std::printf("%d %016llx %016llx\n", blocks[k], (unsigned long long)g[k], (unsigned long long)m[k]);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strncmp(argv[1], "--", 2)) return digest_main(argc, argv);
    const long stride = argc > 1 ? std::atol(argv[1]) : 1;
    const char* only = argc > 2 ? argv[2] : nullptr;
    auto want = [&](const char* n) { return !only || !std::strcmp(only, n); };
    long bad = 0;
    if (want("expf")) bad += check_unary("expf", stride, [](float x) { return expf(x); }, rt_expf);
    if (want("sinf")) bad += check_unary("sinf", stride, [](float x) { return sinf(x); }, rt_sinf);
    if (want("cosf")) bad += check_unary("cosf", stride, [](float x) { return cosf(x); }, rt_cosf);
    if (want("sincosf")) {  // both results of the shared-reduction form, against glibc sinf / cosf
        bad += check_unary("sincos.s", stride, [](float x) { return sinf(x); },
                           [](float x) { float s, c; rt_sincosf(x, s, c); return s; });
        bad += check_unary("sincos.c", stride, [](float x) { return cosf(x); },
                           [](float x) { float s, c; rt_sincosf(x, s, c); return c; });
    }
    if (want("acosf")) bad += check_unary("acosf", stride, [](float x) { return acosf(x); }, rt_acosf);
    if (want("asinf")) bad += check_unary("asinf", stride, [](float x) { return asinf(x); }, rt_asinf);
    if (want("powf5"))
        bad += check_unary("powf5", stride, [](float x) { return powf(x, 5.0f); },
                           [](float x) { return rt_powf(x, 5.0f); });
    if (want("powfg")) {
        const float g = 1.0f / 2.2f;
        bad += check_unary("powfg", stride, [g](float x) { return powf(x, g); },
                           [g](float x) { return rt_powf(x, g); });
    }
    if (want("powfy")) {
        // sweep y at fixed x values (covers the special-case lattice)
        const float xs[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, -2.0f, 3.7f, INFINITY, -INFINITY, NAN, 0x1p-140f, -0x1p-140f};
        long b = 0;
        for (float x : xs) {
            b += check_unary("powf(x,y)", stride * 4, [x](float y) { return powf(x, y); },
                             [x](float y) { return rt_powf(x, y); });
        }
        bad += b;
    }
    if (want("atan2f")) bad += check_atan2(stride);
    // the digest's sweeps that the checks above do not walk: sqrtf, powf over every x at the other fixed
    // exponents, atan2f over y at fixed x
    for (const Sweep& s : sweep_table()) {
        const bool other_y = s.fn == rtdigest::FN_POWF_Y && s.name != "powf.y0" && s.name != "powf.y1";
        if ((s.fn == rtdigest::FN_SQRTF && want("sqrtf")) || (other_y && want("powfys")) ||
            (s.fn == rtdigest::FN_ATAN2F_X && want("atan2fx")))
            bad += check_sweep(s, stride);
    }
    std::printf("TOTAL mismatches %ld\n", bad);
    return bad ? 1 : 0;
}
