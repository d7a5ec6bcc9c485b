// rt_atrous_hip.h — the gfx950 side of the à-trous filter (rt_denoise.h dn_filter_pixel<M>), once
// for its two stages: rt_denoise.hip (M = DnFixed: k_dn_direct, k_dn_lds) and rt_dnv.hip (M = DnVar:
// k_dnv_direct, k_dnv_lds). Each unit includes this and defines its four entry points over the two
// bodies below, so each compiles its own mode alone and neither's code generation depends on the
// other's:
//   dn_direct_body   one pixel per thread, 64 x 4 pixels per block (a wave = 64 neighbouring
//                    pixels of one row, so every tap row is one coalesced 1-KB load); the 25 taps
//                    (and DnVar's 9 variances of the 3x3) read from global memory (L2 absorbs
//                    the 25x re-read)
//   dn_lds_body      TW x TH pixels with their halo of 2 S pixels, records and both guides, staged
//                    in LDS first (steps 1, 2 and 4: 26 / 41 / 55 KB per block); the halo holds the
//                    3x3's ring as well, since 2 S >= 1
// Both fill rt_libm's LDS tables first (rt_expf reads them) and call dn_filter_pixel, so the sums
// run in tap order in either; the entry points store the result: the last pass blends with the caller's
// input and writes the optional sigma_out (dn_store). Which kernel a step takes: dn_use_lds.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_backend_hip.h"
#include "rt_denoise.h"

namespace {

#define DN_TW 64  // direct kernel: tile width (one wave per row) ...
#define DN_TH 4   // ... and height

// Both bodies: false for a thread outside the image, else the thread's pixel q and the filter's output
// for it, which the entry point stores (dn_store). The direct body takes the pass by value and the LDS
// body by reference: with these forms the kernels keep the instruction order they had as two separate
// copies (profiles/atrous_unify_codegen.json).
template <class M>
__device__ __forceinline__ bool dn_direct_body(const rtk::DnPass P, float4_& f, size_t& q)
{
    rtlibm::lds_tables_init();  // (rt_expf reads its table from LDS; before any thread leaves: it has a barrier)
    const int x = blockIdx.x * DN_TW + (threadIdx.x & (DN_TW - 1));
    const int y = blockIdx.y * DN_TH + (threadIdx.x / DN_TW);
    if (x >= P.w || y >= P.h) return false;
    const rtk::DnDirect F{P};
    f = rtk::dn_filter_pixel<M>(P, x, y, F);
    q = (size_t)y * P.w + x;
    return true;
}

// The tile's records and halo in LDS; (x0, y0) is the image position of entry 0.
template <int LW>
struct DnTile {
    const float4_* c;
    const float4_* n;
    const float4_* a;
    int x0, y0;
    __device__ __forceinline__ float4_ color(int x, int y) const { return c[(y - y0) * LW + (x - x0)]; }
    __device__ __forceinline__ float var(int x, int y) const { return c[(y - y0) * LW + (x - x0)].w; }
    __device__ __forceinline__ float4_ nd(int x, int y) const { return n[(y - y0) * LW + (x - x0)]; }
    __device__ __forceinline__ float4_ alb(int x, int y) const { return a[(y - y0) * LW + (x - x0)]; }
};

// TW x TH pixels per block of 256 threads, step S = P.step, halo 2 S on every side.
template <class M, int TW, int TH, int S>
__device__ __forceinline__ bool dn_lds_body(const rtk::DnPass& P, float4_& f, size_t& q)
{
    static_assert(TW * TH == 256, "one pixel per thread");
    static_assert(2 * S >= 1, "the halo holds the 3x3's ring");
    constexpr int LW = TW + 4 * S, LH = TH + 4 * S;
    __shared__ float4_ s_c[LW * LH];
    __shared__ float4_ s_n[LW * LH];
    __shared__ float4_ s_a[LW * LH];
    rtlibm::lds_tables_init();  // (rt_expf's table, beside the tile)
    const int x0 = blockIdx.x * TW - 2 * S, y0 = blockIdx.y * TH - 2 * S;
    const bool guides = P.nd != nullptr;
    // entries outside the image stay unwritten: dn_filter_pixel never asks for them
    for (int i = threadIdx.x; i < LW * LH; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx < 0 || gx >= P.w || gy < 0 || gy >= P.h) continue;
        const size_t g = (size_t)gy * P.w + gx;
        s_c[i] = P.in[g];
        if (guides) {
            s_n[i] = P.nd[g];
            s_a[i] = P.alb[g];
        }
    }
    __syncthreads();
    const int x = blockIdx.x * TW + (int)(threadIdx.x % TW);
    const int y = blockIdx.y * TH + (int)(threadIdx.x / TW);
    if (x >= P.w || y >= P.h) return false;
    const DnTile<LW> F{s_c, s_n, s_a, x0, y0};
    f = rtk::dn_filter_pixel<M>(P, x, y, F);
    q = (size_t)y * P.w + x;
    return true;
}

// Which kernel a step takes, in both stages. dn_variant (rt_test_schedule): 1 direct loads everywhere,
// 2 the LDS tile wherever one is built (steps 1, 2, 4), 0 the faster of the two as measured on the
// MI355X, direct / LDS ms per pass at 1920x1080 (3840x2160):
//   rt_denoise (profiles/denoise_bench.json)
//     step 1 0.182 / 0.116, step 2 0.184 / 0.177, step 4 0.188 / 0.250
//     (0.710 / 0.421, 0.710 / 0.691, 0.709 / 0.962)
//   rt_denoise_var (profiles/denoise_var_bench.json)
//     step 1 0.197 / 0.126, step 2 0.201 / 0.188, step 4 0.208 / 0.264
//     (0.767 / 0.441, 0.775 / 0.711, 0.776 / 0.998)
// The tile wins while its halo is small against the tile. The variance terms cost both kernels about
// 0.02 ms at 1080p and leave the order standing: the tile up to step 2, direct loads from step 4.
inline bool dn_use_lds(int variant, int step)
{
    return step <= 4 && rt_use_lds(variant, step <= 2);
}

// A stage's entry points, in dn_launch_pass's order; A: what they take after the pass.
template <class... A>
struct DnKernels {
    void (*lds4)(rtk::DnPass, A...);  // <32, 8, 4>
    void (*lds1)(rtk::DnPass, A...);  // <64, 4, 1>
    void (*lds2)(rtk::DnPass, A...);  // <64, 4, 2>
    void (*direct)(rtk::DnPass, A...);
};

template <class... A>
int dn_launch_pass(rt_context* c, const DnKernels<A...>& K, const rtk::DnPass& P, bool lds, hipStream_t s, A... a)
{
    if (lds && P.step == 4) {
        const dim3 grid((P.w + 31) / 32, (P.h + 7) / 8);
        hipLaunchKernelGGL(K.lds4, grid, dim3(256), 0, s, P, a...);
    } else if (lds) {
        const dim3 grid((P.w + 63) / 64, (P.h + 3) / 4);
        hipLaunchKernelGGL(P.step == 1 ? K.lds1 : K.lds2, grid, dim3(256), 0, s, P, a...);
    } else {
        const dim3 grid((P.w + DN_TW - 1) / DN_TW, (P.h + DN_TH - 1) / DN_TH);
        hipLaunchKernelGGL(K.direct, grid, dim3(256), 0, s, P, a...);
    }
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

inline Post* dn_post(std::unique_ptr<Post>& p)  // (created on first use)
{
    if (!p) p.reset(new Post());
    return p.get();
}

// A call's passes on stream s, each between two of post's events when it times them: `lead` launches
// of the stage's own went before the first pass (rt_denoise_var's prep, which recorded pev[0] itself).
// launch(P, dst, last) is the stage's dn_launch_pass.
template <class Params, class Launch>
int dn_run_timed(rt_context* c, Post* post, int lead, hipStream_t s, int w, int h, const Params& p, const float4_* first,
                 int o, float4_* out, const float4_* nd, const float4_* alb, Launch launch)
{
    const size_t n = (size_t)w * h;
    float4_* const pp[2] = {(float4_*)post->pp.p, (float4_*)post->pp.p + n};
    int i = lead;
    if (int r = rtk::dn_run_passes(w, h, p, first, pp, o, out, nd, alb, [&](const rtk::DnPass& P, float4_* dst, bool last) {
            if (post->timing) HIPCHK(c, hipEventRecord(post->pev[i++], s));
            return launch(P, dst, last);
        }))
        return r;
    if (post->timing) {
        HIPCHK(c, hipEventRecord(post->pev[lead + p.passes], s));
        post->timed_passes = p.passes;
    }
    return RT_OK;
}

// The body of the two measurement hooks (rt_device_denoise_pass_ms, rt_device_denoise_var_pass_ms): enable
// 1 / 0 turns the events around the later calls' launches on / off, -1 leaves it; with out_ms, the GPU time
// of each launch of the last timed call, its `lead` launches first (waits for them). Returns the number written.
inline int dn_pass_ms(rt_context* c, std::unique_ptr<Post> Backend::*which, int lead, int enable, double* out_ms, int n)
{
    if (!c || !c->backend) return RT_ERR_ARG;
    Backend* b = rt_backend_dev0(c);
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    Post* post = dn_post(b->*which);
    if (enable == 1 && !post->pev[0])
        for (Event& e : post->pev) HIPCHK(c, hipEventCreate(&e.h));
    if (enable >= 0) {
        post->timing = enable == 1;
        if (!post->timing) post->timed_passes = 0;
    }
    if (!out_ms) return 0;
    const int launches = post->timed_passes ? post->timed_passes + lead : 0;
    const int m = launches < n ? launches : n;
    if (m > 0) HIPCHK(c, hipEventSynchronize(post->pev[launches]));
    for (int i = 0; i < m; i++) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, post->pev[i], post->pev[i + 1]));
        out_ms[i] = ms;
    }
    return m;
}

}  // namespace
