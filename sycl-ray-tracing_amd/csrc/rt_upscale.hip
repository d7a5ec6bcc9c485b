// rt_upscale.hip — gfx950 kernels and launch of the guided upscale stage (rt_upscale.h). Its own
// translation unit, so that the render kernels of rt_render.hip and the kernels of the other stages
// compile exactly as they do without it.
//
// Both kernels take k_dn_direct's shape: 64 x 4 output pixels per block, a wave per output row, one
// pixel per thread; the pixel's two full-size guide records are coalesced 16-B loads and the outputs
// coalesced stores of 16 and 4 B. Both fill rt_libm's LDS tables first (rt_expf reads them).
//   k_upscale_direct  every tap's records are global loads (16 B colour, 4 B sigma, 2 x 16 B guides).
//                     Neighbouring lanes read the same or neighbouring low pixels, so the loads
//                     coalesce and the caches absorb the re-reads. The yardstick.
//   k_upscale_lds     the block's low-resolution footprint, tier 2's ring included, is staged first:
//                     because w_lo <= w a 64 x 4 block covers at most 67 x 7 low pixels whatever the
//                     ratio. Three arrays of 16-B records with a pitch of 67 records: {r, g, b, sigma},
//                     normal_depth, albedo: 3 x 7504 B = 22.0 KB beside rt_libm's 512 B. A tap is
//                     three 16-B LDS reads (ds_read_b128: banked by 16-B slot over a 256-B row, in
//                     groups of 16 lanes); a row's lanes read the same slot (a broadcast) or the
//                     next one, so a group's addresses fall on distinct slots of at most two bank
//                     rows, and the odd pitch keeps the two tap rows of a wave apart. Packing sigma
//                     into the colour record's fourth float saves the 4-B read per tap. An entry
//                     outside the low frame stays unwritten: up_tap never asks for it.
//                     The bound of 67 x 7 holds in exact arithmetic; in float32 (a frame wider than
//                     2^24 / 64 pixels, where fx is rounded) the first and the last pixel's x0 can lie
//                     64 apart, so the block measures its footprint (up_footprint) and, when it does
//                     not fit, reads from global memory like the direct kernel: a uniform branch.
// Which kernel a call takes: rt_backend_upscale.
#include <hip/hip_runtime.h>

#include <string>

#include "rt_backend_hip.h"
#include "rt_upscale.h"

namespace {

#define UP_TW 64  // block width in output pixels (one wave per row) ...
#define UP_TH 4   // ... and height
#define UP_LW 67  // the staged footprint's largest width (its pitch) ...
#define UP_LH 7   // ... and height

__device__ __forceinline__ void up_store(const rtk::UpOut& r, size_t p, float4_* __restrict__ rgba_out,
                                         float* __restrict__ sigma_out)
{
    rgba_out[p] = r.rgba;
    if (sigma_out) sigma_out[p] = r.sigma;
}

__global__ __launch_bounds__(256) void k_upscale_direct(rtk::UpArgs A, float4_* __restrict__ rgba_out,
                                                        float* __restrict__ sigma_out)
{
    rtlibm::lds_tables_init();  // (rt_expf reads its table from LDS; before any thread leaves: it has a barrier)
    const int X = blockIdx.x * UP_TW + (threadIdx.x & (UP_TW - 1));
    const int Y = blockIdx.y * UP_TH + (threadIdx.x / UP_TW);
    if (X >= A.w || Y >= A.h) return;
    const size_t p = (size_t)Y * A.w + X;
    const rtk::UpDirect F{A};
    up_store(rtk::up_pixel(A, X, Y, A.nd_hi[p], A.alb_hi[p], F), p, rgba_out, sigma_out);
}

// The staged footprint; (x0, y0) is the low-frame position of entry 0.
struct UpTile {
    const float4_* c;
    const float4_* n;
    const float4_* a;
    int x0, y0;
    __device__ __forceinline__ float4_ rec(int x, int y) const { return c[(y - y0) * UP_LW + (x - x0)]; }
    __device__ __forceinline__ float4_ nd(int x, int y) const { return n[(y - y0) * UP_LW + (x - x0)]; }
    __device__ __forceinline__ float4_ alb(int x, int y) const { return a[(y - y0) * UP_LW + (x - x0)]; }
};

__global__ __launch_bounds__(256) void k_upscale_lds(rtk::UpArgs A, float4_* __restrict__ rgba_out,
                                                     float* __restrict__ sigma_out)
{
    __shared__ float4_ s_c[UP_LW * UP_LH];
    __shared__ float4_ s_n[UP_LW * UP_LH];
    __shared__ float4_ s_a[UP_LW * UP_LH];
    rtlibm::lds_tables_init();  // (rt_expf's table, beside the tile)
    const int X0 = blockIdx.x * UP_TW, Y0 = blockIdx.y * UP_TH;  // (inside the frame: the grid is cut to it)
    const rtk::UpFoot T = rtk::up_footprint(A, X0, Y0, rt_mini(X0 + UP_TW, A.w) - 1, rt_mini(Y0 + UP_TH, A.h) - 1);
    const bool fits = T.w <= UP_LW && T.h <= UP_LH;  // (uniform over the block)
    if (fits) {
        const rtk::UpDirect G{A};
        for (int i = threadIdx.x; i < T.w * T.h; i += 256) {
            const int ly = i / T.w, lx = i - ly * T.w;
            const int gx = T.x0 + lx, gy = T.y0 + ly;
            if (gx < 0 || gx >= A.w_lo || gy < 0 || gy >= A.h_lo) continue;
            const int k = ly * UP_LW + lx;
            s_c[k] = G.rec(gx, gy);
            s_n[k] = G.nd(gx, gy);
            s_a[k] = G.alb(gx, gy);
        }
    }
    __syncthreads();
    const int X = X0 + (int)(threadIdx.x & (UP_TW - 1));
    const int Y = Y0 + (int)(threadIdx.x / UP_TW);
    if (X >= A.w || Y >= A.h) return;
    const size_t p = (size_t)Y * A.w + X;
    const float4_ np = A.nd_hi[p], ap = A.alb_hi[p];
    if (fits) {
        const UpTile F{s_c, s_n, s_a, T.x0, T.y0};
        up_store(rtk::up_pixel(A, X, Y, np, ap, F), p, rgba_out, sigma_out);
    } else {
        const rtk::UpDirect F{A};
        up_store(rtk::up_pixel(A, X, Y, np, ap, F), p, rgba_out, sigma_out);
    }
}

void up_launch(const rtk::UpArgs& A, bool lds, float4_* d_out, float* d_sout, hipStream_t s)
{
    const dim3 grid((A.w + UP_TW - 1) / UP_TW, (A.h + UP_TH - 1) / UP_TH);
    if (lds) hipLaunchKernelGGL(k_upscale_lds, grid, dim3(256), 0, s, A, d_out, d_sout);
    else hipLaunchKernelGGL(k_upscale_direct, grid, dim3(256), 0, s, A, d_out, d_sout);
}

}  // namespace

int rt_backend_upscale(rt_context* c, rtk::UpArgs A, void* rgba_out, void* sigma_out, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const size_t n_lo = (size_t)A.w_lo * A.h_lo, n = (size_t)A.w * A.h;
    const size_t b_lo = n_lo * sizeof(float4_), b_hi = n * sizeof(float4_);
    if (int r = st.staging(b->upscale_io, 3 * b_lo + st.pad(n_lo * sizeof(float)) + 3 * b_hi + st.pad(n * sizeof(float)))) return r;
    A.rgba_lo = (const float4_*)st.in(A.rgba_lo, b_lo);
    A.sigma_lo = (const float*)st.in(A.sigma_lo, n_lo * sizeof(float));  // (null: no sigma)
    A.alb_lo = (const float4_*)st.in(A.alb_lo, b_lo);
    A.nd_lo = (const float4_*)st.in(A.nd_lo, b_lo);
    A.alb_hi = (const float4_*)st.in(A.alb_hi, b_hi);
    A.nd_hi = (const float4_*)st.in(A.nd_hi, b_hi);
    float4_* d_out = (float4_*)st.out(rgba_out, b_hi);
    float* d_sout = (float*)st.out(sigma_out, n * sizeof(float));  // (null exactly when A.sigma_lo is)
    if (int r = st.begin()) return r;
    // Which kernel the call takes (up_variant, rt_use_lds): the faster of the two as measured on the MI355X with a
    // sigma map at 960x540 -> 1920x1080 and at 1920x1080 -> 3840x2160 (the figures: profiles/upscale_bench.json,
    // DESIGN.md §18): the footprint wins at both sizes, by a tenth at the first and by a quarter at the second.
    up_launch(A, rt_use_lds(c->sched.variant[RT_VAR_UP], true), d_out, d_sout, st.s);
    HIPCHK(c, hipGetLastError());
    return st.end();
}

// MEASUREMENT HOOK, like rt_device_noise_kernel_ms of rt_noise.hip: exported by the gfx950 library
// only, not part of include/rt_hip.h, never called by the product paths.
// GPU time of the two kernels on one footing (tools/upscale_bench.py): for each of reps rounds each
// kernel runs alone on the default stream between two events recorded immediately before and after
// it. A: device pointers, validated by the caller as rt_upscale_device validates them (the bench
// goes through rt_upscale_device first). Round r runs kernel (r + first) & 1 before the other, so a caller
// that asks for one round per call passes its own round number. out_ms[k * reps + r]: k = 0 k_upscale_direct,
// 1 k_upscale_lds.
extern "C" int rt_device_upscale_kernel_ms(rt_context* c, int w_lo, int h_lo, int w, int h, const void* d_rgba_lo,
                                           const void* d_sigma_lo, const void* d_alb_lo, const void* d_nd_lo,
                                           const void* d_alb_hi, const void* d_nd_hi, void* d_rgba_out, void* d_sigma_out,
                                           int reps, int first, double* out_ms)
{
    TimedRounds T;
    if (int r = T.enter(c, "rt_device_upscale_kernel_ms", reps, out_ms)) return r;
    // the product's validation and parameters: one product call, whose arguments the loop then reuses
    if (int r = rt_upscale_device(c, w_lo, h_lo, w, h, d_rgba_lo, d_sigma_lo, d_alb_lo, d_nd_lo, d_alb_hi, d_nd_hi, nullptr,
                                  d_rgba_out, d_sigma_out, nullptr))
        return r;
    rt_upscale_params p;
    rt_upscale_default_params(&p);
    const rtk::UpArgs A{w_lo, h_lo, w, h, (float)w_lo / (float)w, (float)h_lo / (float)h, rtk::dn_inv_sigma2(p.sigma_normal),
                        rtk::dn_inv_sigma2(p.sigma_albedo), rtk::dn_inv_sigma2(p.sigma_depth), p.min_weight,
                        (const float4_*)d_rgba_lo, (const float*)d_sigma_lo, (const float4_*)d_alb_lo, (const float4_*)d_nd_lo,
                        (const float4_*)d_alb_hi, (const float4_*)d_nd_hi};
    auto kernel = [&](bool lds) {
        return [&, lds]() -> int {
            up_launch(A, lds, (float4_*)d_rgba_out, (float*)d_sigma_out, nullptr);
            HIPCHK(c, hipGetLastError());
            return RT_OK;
        };
    };
    // (rotated: the order alternates round by round, neither kernel always runs second)
    return T.run(first, {TimedKernel::turns(0, kernel(false)), TimedKernel::turns(1, kernel(true))});
}
