// rt_dnv.hip — gfx950 kernels and launches of the variance-guided post stage (rt_dnv.h): the noise
// figure, the prep and rt_denoise_var's entry points to the à-trous filter (rt_atrous_hip.h, which
// rt_denoise.hip shares). Its own translation unit, so that the render kernels of rt_render.hip and
// the kernels of rt_denoise.hip compile exactly as they do without it.
//
//   k_dnv_sigma    one pixel per thread: one 16-B load of the state and of half, the tile's
//                  counts in an adaptive progression (two 4-B loads, the same words for the 8
//                  neighbouring lanes of a tile row), dnv_noise_sigma, one 4-B store
//   k_dnv_prep     one pixel per thread: the 16-B colour and the 4-B sigma in, the 16-B
//                  record {r, g, b, v} out
//   k_dnv_direct   rt_atrous_hip.h's direct body with the variance-guided filter (DnVar)
//   k_dnv_lds      its LDS-tile body with the same (steps 1, 2 and 4)
#include <hip/hip_runtime.h>

#include <string>

#include "rt_atrous_hip.h"
#include "rt_dnv.h"

namespace {

constexpr int threads = 256;

// tile_n / tile_nA null: the frame's counts (F) in every pixel. n = w * rows.
__global__ __launch_bounds__(256) void k_dnv_sigma(const float4_* __restrict__ state, const float4_* __restrict__ half,
                                                   const int32_t* __restrict__ tile_n, const int32_t* __restrict__ tile_nA,
                                                   int n, int w, int tw, rtk::NoiseArgs F, float* __restrict__ sigma)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rtk::NoiseArgs A = F;
    if (tile_n) {
        const int t = rtk::adapt_tile_of(i, w, tw);
        A = rtk::adapt_tile_args(tile_n[t], tile_nA[t], F);
    }
    sigma[i] = rtk::dnv_noise_sigma(state[i], half[i], A);
}

__global__ __launch_bounds__(256) void k_dnv_prep(const float4_* __restrict__ in, const float* __restrict__ sigma, int n,
                                                  float4_* __restrict__ rec)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rec[i] = rtk::dnv_prep(in[i], sigma[i]);
}

__global__ __launch_bounds__(256) void k_dnv_direct(rtk::DnPass P, float4_* __restrict__ out,
                                                    const float4_* __restrict__ orig, float blend,
                                                    float* __restrict__ sigma_out)
{
    float4_ f;
    size_t q;
    if (dn_direct_body<rtk::DnVar>(P, f, q)) rtk::dn_store(f, q, out, orig, blend, sigma_out);
}

template <int TW, int TH, int S>
__global__ __launch_bounds__(256) void k_dnv_lds(rtk::DnPass P, float4_* __restrict__ out,
                                                 const float4_* __restrict__ orig, float blend,
                                                 float* __restrict__ sigma_out)
{
    float4_ f;
    size_t q;
    if (dn_lds_body<rtk::DnVar, TW, TH, S>(P, f, q)) rtk::dn_store(f, q, out, orig, blend, sigma_out);
}

const DnKernels<float4_*, const float4_*, float, float*> dnv_kernels{k_dnv_lds<32, 8, 4>, k_dnv_lds<64, 4, 1>, k_dnv_lds<64, 4, 2>,
                                                                     k_dnv_direct};

}  // namespace

int rt_backend_denoise_var(rt_context* c, int w, int h, const void* in, const void* sigma, const void* alb, const void* nd,
                           const rt_denoise_var_params& p, float blend, void* out, void* sigma_out, bool device,
                           void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    Post* post = dn_post(b->post_var);
    const size_t n = (size_t)w * h, bytes = n * sizeof(float4_), fbytes = st.pad(n * sizeof(float));
    if (int r = ensure(c, post->pp, 2 * bytes)) return r;
    if (int r = st.staging(post->io, 4 * bytes + 2 * fbytes)) return r;
    const float4_* d_in = (const float4_*)st.in(in, bytes);
    const float* d_sigma = (const float*)st.in(sigma, n * sizeof(float));
    const float4_* d_alb = (const float4_*)st.in(alb, bytes);  // (both null: colour and variance only)
    const float4_* d_nd = (const float4_*)st.in(nd, bytes);
    float4_* d_out = (float4_*)st.out(out, bytes);
    float* d_sout = (float*)st.out(sigma_out, n * sizeof(float));
    hipStream_t s = st.s;
    float4_* rec0 = (float4_*)post->pp.p;
    if (int r = st.begin()) return r;
    if (post->timing) HIPCHK(c, hipEventRecord(post->pev[0], s));
    hipLaunchKernelGGL(k_dnv_prep, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, s, d_in, d_sigma, (int)n,
                       rec0);
    HIPCHK(c, hipGetLastError());
    // (the prep took the first of the two buffers: pass i writes the other one of pass i - 1's)
    if (int r = dn_run_timed(c, post, 1, s, w, h, p, rec0, 1, d_out, d_nd, d_alb,
                             [&](const rtk::DnPass& P, float4_* dst, bool last) {
                                 return dn_launch_pass(c, dnv_kernels, P, dn_use_lds(c->sched.variant[RT_VAR_DN], P.step), s, dst,
                                                       last ? d_in : nullptr, blend, last ? d_sout : nullptr);
                             }))
        return r;
    return st.end();
}

// rt_backend_progress_noise's staged call (rt_noise.hip) around k_dnv_sigma: the same streams,
// waits and marker, the query's one output in the noise query's staging buffer.
int rt_backend_progress_noise_sigma(rt_context* c, const rtk::NoiseArgs& A, float* sigma, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    const RtProgress& P = c->prog;
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, b->own)) return r;
    const size_t n = P.npx();
    if (int r = st.staging(b->pg_noise, st.pad(4 * n))) return r;
    float* d_sigma = (float*)st.out(sigma, 4 * n);
    if (int r = b->ev_done.wait(c, st.s)) return r;  // (the last pass, its scatter and fold)
    if (device)
        if (int r = b->ev_pg.wait(c, st.s)) return r;
    if (int r = st.begin()) return r;
    const int32_t* tn = P.adaptive ? (const int32_t*)b->adapt->tile_n.p : nullptr;
    const int32_t* tna = P.adaptive ? (const int32_t*)b->adapt->tile_nA.p : nullptr;
    hipLaunchKernelGGL(k_dnv_sigma, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, st.s,
                       (const float4_*)b->pg_state.p, (const float4_*)b->pg_half.p, tn, tna, (int)n, P.w, P.tiles_w(), A,
                       d_sigma);
    HIPCHK(c, hipGetLastError());
    return st.end(&b->ev_pg);  // (device form: the next pass writes what this reads)
}

// MEASUREMENT HOOK, like rt_device_denoise_pass_ms of rt_denoise.hip: exported by the gfx950
// library only, not part of include/rt_hip.h, never called by the product paths.
// GPU time of the stage's launches (tools/denoise_var_bench.py): enable 1 / 0 turns the events
// around the prep and each pass of the later rt_denoise_var calls on / off, -1 leaves it; with
// out_ms, the last timed call's launches, the prep first (waits for them). Returns the number written.
extern "C" int rt_device_denoise_var_pass_ms(rt_context* c, int enable, double* out_ms, int n)
{
    return dn_pass_ms(c, &Backend::post_var, 1, enable, out_ms, n);
}
