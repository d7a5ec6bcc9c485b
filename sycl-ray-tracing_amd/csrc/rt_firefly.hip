// rt_firefly.hip — gfx950 kernels and launch of the firefly rejection stage (rt_firefly.h). Its own
// translation unit, so that the render kernels of rt_render.hip and the kernels of rt_denoise.hip,
// rt_dnv.hip and rt_temporal.hip compile exactly as they do without it.
//
// Both kernels take k_dn_direct's shape: 64 x 4 pixels per block, a wave per row, one pixel per
// thread; the pixel's own 16-B record and 4-B sigma are loaded once, coalesced along the row, and
// the three outputs are coalesced stores of 16, 4 and 4 B.
//   k_firefly_lds<R>     only the neighbours' ranked values (rt_firefly.h ff_rank_value, one float per
//                        pixel) go to an LDS tile of (64 + 2 R) x (4 + 2 R) floats: 1584 B at R = 1,
//                        2176 B at R = 2. A thread stores its own pixel's value from the record it
//                        holds; the 140 (R = 1) or 288 (R = 2) halo entries are loaded by the first
//                        threads of the block, a 16-B record each. An entry outside the image, or of
//                        a dropped neighbour, holds -inf, which the insertion ignores, so every entry
//                        is written and the 8 or 24 taps are plain LDS reads: a row's lanes read
//                        consecutive floats, no bank conflict.
//   k_firefly_direct<R>  no LDS: each tap is a bounds test, a 16-B global load and the luminance
//                        recomputed. The yardstick that shows whether the tile pays.
// firefly_pixel evaluates no expf, so rtlibm::lds_tables_init() is not called here.
// Which kernel a call takes: rt_backend_firefly.
#include <hip/hip_runtime.h>

#include <string>

#include "rt_backend_hip.h"
#include "rt_firefly.h"

namespace {

#define FF_TW 64  // tile width (one wave per row) ...
#define FF_TH 4   // ... and height

__device__ __forceinline__ void ff_store(const rtk::FireflyOut& r, size_t p, float4_* __restrict__ rgba_out,
                                         float* __restrict__ sigma_out, float* __restrict__ scale_out)
{
    rgba_out[p] = r.rgba;
    if (sigma_out) sigma_out[p] = r.sigma;
    if (scale_out) scale_out[p] = r.scale;
}

template <int R>
__global__ __launch_bounds__(256) void k_firefly_direct(rtk::FireflyArgs A, float4_* __restrict__ rgba_out,
                                                        float* __restrict__ sigma_out, float* __restrict__ scale_out)
{
    const int x = blockIdx.x * FF_TW + (threadIdx.x & (FF_TW - 1));
    const int y = blockIdx.y * FF_TH + (threadIdx.x / FF_TW);
    if (x >= A.w || y >= A.h) return;
    const size_t p = (size_t)y * A.w + x;
    const float4_ c = A.in[p];
    const float s = A.sigma ? A.sigma[p] : 0.0f;
    const rtk::FfDirect F{A};
    ff_store(rtk::firefly_pixel<R>(A, x, y, c, s, F), p, rgba_out, sigma_out, scale_out);
}

// The tile of ranked values; (x0, y0) is the image position of entry 0.
template <int LW>
struct FfTile {
    const float* v;
    int x0, y0;
    __device__ __forceinline__ float value(int x, int y) const { return v[(y - y0) * LW + (x - x0)]; }
};

template <int R>
__global__ __launch_bounds__(256) void k_firefly_lds(rtk::FireflyArgs A, float4_* __restrict__ rgba_out,
                                                     float* __restrict__ sigma_out, float* __restrict__ scale_out)
{
    constexpr int LW = FF_TW + 2 * R, LH = FF_TH + 2 * R;
    constexpr int ROWS = 2 * R * LW;               // halo entries in the R rows above and the R below
    constexpr int HALO = ROWS + FF_TH * 2 * R;     // ... and the R columns left and right of the 4 rows
    __shared__ float s_v[LW * LH];
    const int tx = threadIdx.x & (FF_TW - 1), ty = threadIdx.x / FF_TW;
    const int x0 = blockIdx.x * FF_TW - R, y0 = blockIdx.y * FF_TH - R;
    const int x = x0 + R + tx, y = y0 + R + ty;
    const bool inside = x < A.w && y < A.h;
    const size_t p = (size_t)y * A.w + x;
    float4_ c = float4_{0, 0, 0, 0};
    float s = 0.0f;
    if (inside) {
        c = A.in[p];
        if (A.sigma) s = A.sigma[p];
    }
    s_v[(ty + R) * LW + (tx + R)] = inside ? rtk::ff_rank_value(c) : rtk::ff_neg_inf();
    for (int i = threadIdx.x; i < HALO; i += 256) {
        int lx, ly;
        if (i < ROWS) {
            const int row = i / LW;
            lx = i - row * LW;
            ly = row < R ? row : row + FF_TH;
        } else {
            const int j = i - ROWS, k = j % (2 * R);
            ly = R + j / (2 * R);
            lx = k < R ? k : k + FF_TW;
        }
        const int gx = x0 + lx, gy = y0 + ly;
        float v = rtk::ff_neg_inf();
        if (gx >= 0 && gx < A.w && gy >= 0 && gy < A.h) v = rtk::ff_rank_value(A.in[(size_t)gy * A.w + gx]);
        s_v[ly * LW + lx] = v;
    }
    __syncthreads();
    if (!inside) return;
    const FfTile<LW> F{s_v, x0, y0};
    ff_store(rtk::firefly_pixel<R>(A, x, y, c, s, F), p, rgba_out, sigma_out, scale_out);
}

}  // namespace

int rt_backend_firefly(rt_context* c, rtk::FireflyArgs A, void* rgba_out, void* sigma_out, void* scale_out, bool device,
                       void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const size_t n = (size_t)A.w * A.h, bytes = n * sizeof(float4_), fbytes = st.pad(n * sizeof(float));
    if (int r = st.staging(b->firefly_io, 2 * bytes + 3 * fbytes)) return r;
    A.in = (const float4_*)st.in(A.in, bytes);
    A.sigma = (const float*)st.in(A.sigma, n * sizeof(float));  // (null: no sigma_in)
    float4_* d_out = (float4_*)st.out(rgba_out, bytes);
    float* d_sout = (float*)st.out(sigma_out, n * sizeof(float));  // (either may be null)
    float* d_fout = (float*)st.out(scale_out, n * sizeof(float));
    if (int r = st.begin()) return r;
    const dim3 grid((A.w + FF_TW - 1) / FF_TW, (A.h + FF_TH - 1) / FF_TH);
    // Which kernel the call takes (ff_variant, rt_use_lds): the faster of the two as measured on the MI355X
    // (profiles/firefly_bench.json), LDS / direct ms at rank 2, 1920x1080: radius 1 0.023 / 0.059,
    // radius 2 0.032 / 0.143 (3840x2160: 0.080 / 0.220, 0.109 / 0.555). The tile wins at both radii and both sizes,
    // at rank 8 as well.
    const bool lds = rt_use_lds(c->sched.variant[RT_VAR_FF], true);
    if (lds && A.radius == 1) hipLaunchKernelGGL(k_firefly_lds<1>, grid, dim3(256), 0, st.s, A, d_out, d_sout, d_fout);
    else if (lds) hipLaunchKernelGGL(k_firefly_lds<2>, grid, dim3(256), 0, st.s, A, d_out, d_sout, d_fout);
    else if (A.radius == 1) hipLaunchKernelGGL(k_firefly_direct<1>, grid, dim3(256), 0, st.s, A, d_out, d_sout, d_fout);
    else hipLaunchKernelGGL(k_firefly_direct<2>, grid, dim3(256), 0, st.s, A, d_out, d_sout, d_fout);
    HIPCHK(c, hipGetLastError());
    return st.end();
}
