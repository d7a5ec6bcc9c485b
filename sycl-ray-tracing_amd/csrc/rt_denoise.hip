// rt_denoise.hip — gfx950 kernels and launches of the post stage (rt_denoise.h): the
// first-hit feature pass and the edge-avoiding à-trous filter. Its own translation unit,
// so that the render kernels of rt_render.hip compile exactly as they do without it.
//
//   k_features     one pixel per thread: the exact closest-hit query of k_intersect on the
//                  pixel's centre ray, then the two 16-B feature records
//   k_dn_direct    one pixel per thread, 64 x 4 pixels per block (a wave = 64 neighbouring
//                  pixels of one row, so every tap row is one coalesced 1-KB load); taps
//                  read from global memory (L2 absorbs the 25x re-read)
//   k_dn_lds       the same tile with its halo of 2 s pixels staged in LDS first (steps
//                  1, 2 and 4: 26 / 41 / 55 KB per block)
// Both filter kernels fill rt_libm's LDS tables first (rt_expf reads them) and call
// dn_filter_pixel, so the sums run in tap order in either; the last pass blends with the
// input (dn_blend). Which kernel a step takes: dn_use_lds.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "rt_backend_hip.h"
#include "rt_denoise.h"

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

#define DN_TW 64  // direct kernel: tile width (one wave per row) ...
#define DN_TH 4   // ... and height

// orig != null: the last pass (blend with the input)
__global__ __launch_bounds__(256) void k_dn_direct(rtk::DnPass P, float4_* __restrict__ out,
                                                   const float4_* __restrict__ orig, float blend)
{
    rtlibm::lds_tables_init();  // (rt_expf reads its table from LDS; before any thread leaves: it has a barrier)
    const int x = blockIdx.x * DN_TW + (threadIdx.x & (DN_TW - 1));
    const int y = blockIdx.y * DN_TH + (threadIdx.x / DN_TW);
    if (x >= P.w || y >= P.h) return;
    const rtk::DnDirect F{P};
    const float4_ f = rtk::dn_filter_pixel(P, x, y, F);
    const size_t q = (size_t)y * P.w + x;
    out[q] = orig ? rtk::dn_blend(f, orig[q], blend) : f;
}

// The tile's pixels and halo in LDS; (x0, y0) is the image position of entry 0.
template <int LW>
struct DnTile {
    const float4_* c;
    const float4_* n;
    const float4_* a;
    int x0, y0;
    __device__ __forceinline__ float4_ color(int x, int y) const { return c[(y - y0) * LW + (x - x0)]; }
    __device__ __forceinline__ float4_ nd(int x, int y) const { return n[(y - y0) * LW + (x - x0)]; }
    __device__ __forceinline__ float4_ alb(int x, int y) const { return a[(y - y0) * LW + (x - x0)]; }
};

// TW x TH pixels per block of 256 threads, step S = P.step, halo 2 S on every side.
template <int TW, int TH, int S>
__global__ __launch_bounds__(256) void k_dn_lds(rtk::DnPass P, float4_* __restrict__ out,
                                                const float4_* __restrict__ orig, float blend)
{
    static_assert(TW * TH == 256, "one pixel per thread");
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
    if (x >= P.w || y >= P.h) return;
    const DnTile<LW> F{s_c, s_n, s_a, x0, y0};
    const float4_ f = rtk::dn_filter_pixel(P, x, y, F);
    const size_t q = (size_t)y * P.w + x;
    out[q] = orig ? rtk::dn_blend(f, orig[q], blend) : f;
}

// Which kernel a step takes. dn_variant (rt_test_schedule): 1 direct loads everywhere, 2 the
// LDS tile wherever one is built (steps 1, 2, 4), 0 the faster of the two as measured on the
// MI355X (profiles/denoise_bench.json), direct / LDS ms per pass at 1920x1080:
// step 1 0.182 / 0.116, step 2 0.184 / 0.177, step 4 0.188 / 0.250 (3840x2160: 0.710 / 0.421,
// 0.710 / 0.691, 0.709 / 0.962): the tile wins while its halo is small against the tile.
bool dn_use_lds(int variant, int step)
{
    if (step > 4) return false;
    if (variant == 1) return false;
    if (variant == 2) return true;
    return step <= 2;
}

int launch_pass(rt_context* c, const rtk::DnPass& P, float4_* out, const float4_* orig, float blend, bool lds,
                hipStream_t s)
{
    if (lds && P.step == 4) {
        const dim3 grid((P.w + 31) / 32, (P.h + 7) / 8);
        hipLaunchKernelGGL((k_dn_lds<32, 8, 4>), grid, dim3(256), 0, s, P, out, orig, blend);
    } else if (lds) {
        const dim3 grid((P.w + 63) / 64, (P.h + 3) / 4);
        if (P.step == 1) hipLaunchKernelGGL((k_dn_lds<64, 4, 1>), grid, dim3(256), 0, s, P, out, orig, blend);
        else hipLaunchKernelGGL((k_dn_lds<64, 4, 2>), grid, dim3(256), 0, s, P, out, orig, blend);
    } else {
        const dim3 grid((P.w + DN_TW - 1) / DN_TW, (P.h + DN_TH - 1) / DN_TH);
        hipLaunchKernelGGL(k_dn_direct, grid, dim3(256), 0, s, P, out, orig, blend);
    }
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

}  // namespace

// The post stage's buffers on the root device, cached across calls like the render's.
struct Post {
    DevBuf io;    // host-pointer calls: input, output, albedo, normal_depth
    DevBuf pp;    // ping-pong colour buffers between passes
    // optional per-pass timing (rt_device_denoise_pass_ms): an event before each pass and after the last
    bool timing = false;
    Event pev[11];
    int timed_passes = 0;
};

void PostDelete::operator()(Post* p) const { delete p; }

static Post* post_of(Backend* b)  // (created on first use)
{
    if (!b->post) b->post.reset(new Post());
    return b->post.get();
}

int rt_backend_features(rt_context* c, int w, int h, void* albedo, void* normal_depth, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const size_t n = (size_t)w * h, bytes = n * sizeof(float4_);
    if (int r = st.staging(post_of(b)->io, 4 * bytes)) return r;  // (rt_denoise's four regions: one size for both)
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
    Post* post = post_of(b);
    const size_t n = (size_t)w * h, bytes = n * sizeof(float4_);
    if (int r = ensure(c, post->pp, 2 * bytes)) return r;
    if (int r = st.staging(post->io, 4 * bytes)) return r;
    const float4_* d_in = (const float4_*)st.in(in, bytes);
    float4_* d_out = (float4_*)st.out(out, bytes);
    const float4_* d_alb = (const float4_*)st.in(alb, bytes);  // (both null: colour only)
    const float4_* d_nd = (const float4_*)st.in(nd, bytes);
    hipStream_t s = st.s;
    float4_* pp[2] = {(float4_*)post->pp.p, (float4_*)post->pp.p + n};
    const float4_* src = d_in;
    if (int r = st.begin()) return r;
    for (int i = 0; i < p.passes; i++) {
        const bool last = i + 1 == p.passes;
        const rtk::DnPass P{w,
                            h,
                            1 << i,
                            rtk::dn_inv_sigma2(std::ldexp((double)p.sigma_color, -i)),
                            rtk::dn_inv_sigma2(p.sigma_normal),
                            rtk::dn_inv_sigma2(p.sigma_albedo),
                            rtk::dn_inv_sigma2(p.sigma_depth),
                            src,
                            d_nd,
                            d_alb};
        float4_* dst = last ? d_out : pp[i & 1];
        if (post->timing) HIPCHK(c, hipEventRecord(post->pev[i], s));
        if (int r = launch_pass(c, P, dst, last ? d_in : nullptr, blend, dn_use_lds(c->sched.dn_variant, P.step), s))
            return r;
        src = dst;
    }
    if (post->timing) {
        HIPCHK(c, hipEventRecord(post->pev[p.passes], s));
        post->timed_passes = p.passes;
    }
    return st.end();
}

// MEASUREMENT HOOK, like rt_device_libm / rt_device_queries of rt_probe.hip: exported by the
// gfx950 library only, not part of include/rt_hip.h, never called by the product paths.
// Per-pass GPU time of the filter (tools/denoise_bench.py): enable 1 / 0 turns the events
// around each pass of the later rt_denoise calls on / off, -1 leaves it; with out_ms, the
// last timed call's passes (waits for them). Returns the number of passes written.
extern "C" int rt_device_denoise_pass_ms(rt_context* c, int enable, double* out_ms, int n)
{
    if (!c || !c->backend) return RT_ERR_ARG;
    Backend* b = rt_backend_dev0(c);
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    Post* post = post_of(b);
    if (enable == 1 && !post->pev[0])
        for (Event& e : post->pev) HIPCHK(c, hipEventCreate(&e.h));
    if (enable >= 0) {
        post->timing = enable == 1;
        if (!post->timing) post->timed_passes = 0;
    }
    if (!out_ms) return 0;
    const int m = post->timed_passes < n ? post->timed_passes : n;
    if (m > 0) HIPCHK(c, hipEventSynchronize(post->pev[post->timed_passes]));
    for (int i = 0; i < m; i++) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, post->pev[i], post->pev[i + 1]));
        out_ms[i] = ms;
    }
    return m;
}
