// rt_denoise.hip — gfx950 kernels and launches of the post stage (rt_denoise.h): the
// first-hit feature pass and rt_denoise's entry points to the à-trous filter (rt_atrous_hip.h, which
// rt_dnv.hip shares). Its own translation unit, so that the render kernels of rt_render.hip compile
// exactly as they do without it.
//
//   k_features     one pixel per thread: the exact closest-hit query of k_intersect on the
//                  pixel's centre ray, then the two 16-B feature records
//   k_dn_direct    rt_atrous_hip.h's direct body with the fixed filter (DnFixed)
//   k_dn_lds       its LDS-tile body with the same (steps 1, 2 and 4)
#include <hip/hip_runtime.h>

#include <string>

#include "rt_atrous_hip.h"

namespace {

__global__ __launch_bounds__(256) void k_features(RtSceneView S, rtk::CamView V, float4_* __restrict__ alb,
                                                  float4_* __restrict__ nd)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V.W * V.H) return;
    rtk::StackEnt stack[RT_STACK_CAP];
    const int y = i / V.W, x = i - y * V.W;
    float4_ n, a;
    rtk::feature_pixel(S, V, x, y, stack, n, a);
    nd[i] = n;
    alb[i] = a;
}

__global__ __launch_bounds__(256) void k_dn_direct(rtk::DnPass P, float4_* __restrict__ out,
                                                   const float4_* __restrict__ orig, float blend)
{
    float4_ f;
    size_t q;
    if (dn_direct_body<rtk::DnFixed>(P, f, q)) rtk::dn_store(f, q, out, orig, blend, nullptr);
}

template <int TW, int TH, int S>
__global__ __launch_bounds__(256) void k_dn_lds(rtk::DnPass P, float4_* __restrict__ out,
                                                const float4_* __restrict__ orig, float blend)
{
    float4_ f;
    size_t q;
    if (dn_lds_body<rtk::DnFixed, TW, TH, S>(P, f, q)) rtk::dn_store(f, q, out, orig, blend, nullptr);
}

const DnKernels<float4_*, const float4_*, float> dn_kernels{k_dn_lds<32, 8, 4>, k_dn_lds<64, 4, 1>, k_dn_lds<64, 4, 2>,
                                                            k_dn_direct};

}  // namespace

int rt_backend_features(rt_context* c, int w, int h, void* albedo, void* normal_depth, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const size_t n = (size_t)w * h, bytes = n * sizeof(float4_);
    if (int r = st.staging(dn_post(b->post)->io, 4 * bytes)) return r;  // (rt_denoise's four regions: one size for both)
    float4_* d_alb = (float4_*)st.out(albedo, bytes);
    float4_* d_nd = (float4_*)st.out(normal_depth, bytes);
    const rtk::CamView V = rtk::cam_view(c->cam, w, h);
    if (int r = st.begin()) return r;
    hipLaunchKernelGGL(k_features, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st.s, b->view, V, d_alb, d_nd);
    HIPCHK(c, hipGetLastError());
    return st.end();
}

int rt_backend_denoise(rt_context* c, int w, int h, const void* in, const void* alb, const void* nd,
                       const rt_denoise_params& p, float blend, void* out, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    Post* post = dn_post(b->post);
    const size_t bytes = (size_t)w * h * sizeof(float4_);
    if (int r = ensure(c, post->pp, 2 * bytes)) return r;
    if (int r = st.staging(post->io, 4 * bytes)) return r;
    const float4_* d_in = (const float4_*)st.in(in, bytes);
    float4_* d_out = (float4_*)st.out(out, bytes);
    const float4_* d_alb = (const float4_*)st.in(alb, bytes);  // (both null: colour only)
    const float4_* d_nd = (const float4_*)st.in(nd, bytes);
    if (int r = st.begin()) return r;
    if (int r = dn_run_timed(c, post, 0, st.s, w, h, p, d_in, 0, d_out, d_nd, d_alb,
                             [&](const rtk::DnPass& P, float4_* dst, bool last) {
                                 return dn_launch_pass(c, dn_kernels, P, dn_use_lds(c->sched.variant[RT_VAR_DN], P.step), st.s, dst,
                                                       last ? d_in : nullptr, blend);
                             }))
        return r;
    return st.end();
}

// MEASUREMENT HOOK, like rt_device_libm / rt_device_queries of rt_probe.hip: exported by the
// gfx950 library only, not part of include/rt_hip.h, never called by the product paths.
// Per-pass GPU time of the filter (tools/denoise_bench.py): enable 1 / 0 turns the events
// around each pass of the later rt_denoise calls on / off, -1 leaves it; with out_ms, the
// last timed call's passes (waits for them). Returns the number of passes written.
extern "C" int rt_device_denoise_pass_ms(rt_context* c, int enable, double* out_ms, int n)
{
    return dn_pass_ms(c, &Backend::post, 0, enable, out_ms, n);
}
