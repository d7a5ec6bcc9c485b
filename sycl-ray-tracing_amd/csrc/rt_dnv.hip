// rt_dnv.hip — gfx950 kernels and launches of the variance-guided post stage (rt_dnv.h). Its
// own translation unit, so that the render kernels of rt_render.hip and the filter kernels of
// rt_denoise.hip compile exactly as they do without it.
//
//   k_dnv_sigma    one pixel per thread: one 16-B load of the state and of half, the tile's
//                  counts in an adaptive progression (two 4-B loads, the same words for the 8
//                  neighbouring lanes of a tile row), dnv_noise_sigma, one 4-B store
//   k_dnv_prep     one pixel per thread: the 16-B colour and the 4-B sigma in, the 16-B
//                  record {r, g, b, v} out
//   k_dnv_direct   k_dn_direct's shape: 64 x 4 pixels per block, a wave per row; the 25 taps
//                  and the 9 variances of the 3x3 read from global memory
//   k_dnv_lds      k_dn_lds's shape: the tile of records and both guides with a halo of 2 S
//                  pixels staged in LDS (steps 1, 2 and 4, k_dn_lds's sizes); the halo holds
//                  the 3x3's ring as well, since 2 S >= 1
// Both filter kernels fill rt_libm's LDS tables first and call dnv_filter_pixel, so the sums
// run in tap order in either; the last pass blends with the caller's input (dn_blend) and
// writes the optional sigma_out. Which kernel a step takes: dnv_use_lds.
#include <hip/hip_runtime.h>

#include <string>

#include "rt_backend_hip.h"
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

#define DNV_TW 64  // direct kernel: tile width (one wave per row) ...
#define DNV_TH 4   // ... and height

// The end of a pass for pixel q: a record for the next pass, or (orig != null: the last pass)
// the blend with the caller's input and the optional sigma_out.
__device__ __forceinline__ void dnv_store(const float4_& f, size_t q, float4_* __restrict__ out,
                                          const float4_* __restrict__ orig, float blend, float* __restrict__ sigma_out)
{
    if (!orig) {
        out[q] = f;
        return;
    }
    out[q] = rtk::dn_blend(f, orig[q], blend);
    if (sigma_out) sigma_out[q] = rt_sqrtf(f.w);
}

__global__ __launch_bounds__(256) void k_dnv_direct(rtk::DnvPass P, float4_* __restrict__ out,
                                                    const float4_* __restrict__ orig, float blend,
                                                    float* __restrict__ sigma_out)
{
    rtlibm::lds_tables_init();  // (rt_expf reads its table from LDS; before any thread leaves: it has a barrier)
    const int x = blockIdx.x * DNV_TW + (threadIdx.x & (DNV_TW - 1));
    const int y = blockIdx.y * DNV_TH + (threadIdx.x / DNV_TW);
    if (x >= P.w || y >= P.h) return;
    const rtk::DnvDirect F{P};
    dnv_store(rtk::dnv_filter_pixel(P, x, y, F), (size_t)y * P.w + x, out, orig, blend, sigma_out);
}

// The tile's records and halo in LDS; (x0, y0) is the image position of entry 0.
template <int LW>
struct DnvTile {
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
template <int TW, int TH, int S>
__global__ __launch_bounds__(256) void k_dnv_lds(rtk::DnvPass P, float4_* __restrict__ out,
                                                 const float4_* __restrict__ orig, float blend,
                                                 float* __restrict__ sigma_out)
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
    // entries outside the image stay unwritten: dnv_filter_pixel never asks for them
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
    const DnvTile<LW> F{s_c, s_n, s_a, x0, y0};
    dnv_store(rtk::dnv_filter_pixel(P, x, y, F), (size_t)y * P.w + x, out, orig, blend, sigma_out);
}

// Which kernel a step takes. dn_variant (rt_test_schedule): 1 direct loads everywhere, 2 the LDS
// tile wherever one is built (steps 1, 2, 4), 0 the faster of the two as measured on the MI355X
// (profiles/denoise_var_bench.json), direct / LDS ms per pass at 1920x1080:
// step 1 0.197 / 0.126, step 2 0.201 / 0.188, step 4 0.208 / 0.264 (3840x2160: 0.767 / 0.441,
// 0.775 / 0.711, 0.776 / 0.998). The variance terms cost both kernels about 0.02 ms at 1080p and
// leave rt_denoise's order standing: the tile up to step 2, direct loads from step 4.
bool dnv_use_lds(int variant, int step)
{
    if (step > 4) return false;
    if (variant == 1) return false;
    if (variant == 2) return true;
    return step <= 2;
}

int launch_pass(rt_context* c, const rtk::DnvPass& P, float4_* out, const float4_* orig, float blend, float* sigma_out,
                bool lds, hipStream_t s)
{
    if (lds && P.step == 4) {
        const dim3 grid((P.w + 31) / 32, (P.h + 7) / 8);
        hipLaunchKernelGGL((k_dnv_lds<32, 8, 4>), grid, dim3(256), 0, s, P, out, orig, blend, sigma_out);
    } else if (lds) {
        const dim3 grid((P.w + 63) / 64, (P.h + 3) / 4);
        if (P.step == 1) hipLaunchKernelGGL((k_dnv_lds<64, 4, 1>), grid, dim3(256), 0, s, P, out, orig, blend, sigma_out);
        else hipLaunchKernelGGL((k_dnv_lds<64, 4, 2>), grid, dim3(256), 0, s, P, out, orig, blend, sigma_out);
    } else {
        const dim3 grid((P.w + DNV_TW - 1) / DNV_TW, (P.h + DNV_TH - 1) / DNV_TH);
        hipLaunchKernelGGL(k_dnv_direct, grid, dim3(256), 0, s, P, out, orig, blend, sigma_out);
    }
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

}  // namespace

// This stage's buffers on the root device, a sibling of rt_denoise.hip's Post, cached across calls.
struct PostVar {
    DevBuf io;  // host-pointer calls: input, sigma, albedo, normal_depth, output, sigma_out
    DevBuf pp;  // the two record buffers the passes alternate between
    // optional timing (rt_device_denoise_var_pass_ms): an event before the prep, before each pass and after the last
    bool timing = false;
    Event pev[12];
    int timed_passes = 0;
};

void PostVarDelete::operator()(PostVar* p) const { delete p; }

static PostVar* post_var_of(Backend* b)  // (created on first use)
{
    if (!b->post_var) b->post_var.reset(new PostVar());
    return b->post_var.get();
}

int rt_backend_denoise_var(rt_context* c, int w, int h, const void* in, const void* sigma, const void* alb, const void* nd,
                           const rt_denoise_var_params& p, float blend, void* out, void* sigma_out, bool device,
                           void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    PostVar* post = post_var_of(b);
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
    float4_* pp[2] = {(float4_*)post->pp.p, (float4_*)post->pp.p + n};
    if (int r = st.begin()) return r;
    if (post->timing) HIPCHK(c, hipEventRecord(post->pev[0], s));
    hipLaunchKernelGGL(k_dnv_prep, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, s, d_in, d_sigma, (int)n,
                       pp[0]);
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < p.passes; i++) {
        const bool last = i + 1 == p.passes;
        const rtk::DnvPass P{w,
                             h,
                             1 << i,
                             rtk::dn_inv_sigma2(p.sigma_color),
                             rtk::dn_inv_sigma2(p.sigma_normal),
                             rtk::dn_inv_sigma2(p.sigma_albedo),
                             rtk::dn_inv_sigma2(p.sigma_depth),
                             p.var_floor,
                             pp[i & 1],
                             d_nd,
                             d_alb};
        if (post->timing) HIPCHK(c, hipEventRecord(post->pev[i + 1], s));
        if (int r = launch_pass(c, P, last ? d_out : pp[(i + 1) & 1], last ? d_in : nullptr, blend, last ? d_sout : nullptr,
                                dnv_use_lds(c->sched.dn_variant, P.step), s))
            return r;
    }
    if (post->timing) {
        HIPCHK(c, hipEventRecord(post->pev[p.passes + 1], s));
        post->timed_passes = p.passes;
    }
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
    if (!c || !c->backend) return RT_ERR_ARG;
    Backend* b = rt_backend_dev0(c);
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    PostVar* post = post_var_of(b);
    if (enable == 1 && !post->pev[0])
        for (Event& e : post->pev) HIPCHK(c, hipEventCreate(&e.h));
    if (enable >= 0) {
        post->timing = enable == 1;
        if (!post->timing) post->timed_passes = 0;
    }
    if (!out_ms) return 0;
    const int launches = post->timed_passes ? post->timed_passes + 1 : 0;
    const int m = launches < n ? launches : n;
    if (m > 0) HIPCHK(c, hipEventSynchronize(post->pev[launches]));
    for (int i = 0; i < m; i++) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, post->pev[i], post->pev[i + 1]));
        out_ms[i] = ms;
    }
    return m;
}
