// rt_temporal.hip — gfx950 kernel and launch of temporal accumulation (rt_temporal.h). Its own
// translation unit, so that the render kernels of rt_render.hip and the filter kernels of
// rt_denoise.hip and rt_dnv.hip compile exactly as they do without it.
//
//   k_temporal   k_dn_direct's shape: 64 x 4 pixels per block, a wave per row, one pixel per
//                thread. This frame's colour and guide are two 16-B loads and its sigma one 4-B
//                load, all coalesced along the row. The four taps of the history are gathered
//                straight from global memory: per tap two 16-B records (colour, guide) and two
//                4-B words (sigma, len). Where a tile of the current frame lands in the previous
//                one under a free camera move is not bounded, so no LDS tile is built; for any
//                smooth motion neighbouring lanes' positions differ by about a pixel, so a wave's
//                taps fall in the same or neighbouring lines and the two taps of a row share them.
//                Three coalesced stores: 16 B, 4 B, 4 B.
// temporal_pixel evaluates no expf, so rtlibm::lds_tables_init() is not called here (the filter
// kernels need it for rt_expf's table; this kernel has no LDS and no barrier).
#include <hip/hip_runtime.h>

#include <string>

#include "rt_backend_hip.h"
#include "rt_temporal.h"

namespace {

#define TP_TW 64  // tile width (one wave per row) ...
#define TP_TH 4   // ... and height

__global__ __launch_bounds__(256) void k_temporal(rtk::TemporalFrame T, float4_* __restrict__ rgba_out,
                                                  float* __restrict__ sigma_out, float* __restrict__ len_out)
{
    const int x = blockIdx.x * TP_TW + (threadIdx.x & (TP_TW - 1));
    const int y = blockIdx.y * TP_TH + (threadIdx.x / TP_TW);
    if (x >= T.cur.W || y >= T.cur.H) return;
    const rtk::TemporalOut r = rtk::temporal_pixel(T, x, y);
    const size_t p = (size_t)y * T.cur.W + x;
    rgba_out[p] = r.rgba;
    sigma_out[p] = r.sigma;
    len_out[p] = r.len;
}

}  // namespace

int rt_backend_temporal(rt_context* c, rtk::TemporalFrame T, void* rgba_out, void* sigma_out, void* len_out, bool device,
                        void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const int w = T.cur.W, h = T.cur.H;
    const size_t n = (size_t)w * h, bytes = n * sizeof(float4_), fbytes = st.pad(n * sizeof(float));
    if (int r = st.staging(b->temporal_io, 5 * bytes + 5 * fbytes)) return r;
    T.in = (const float4_*)st.in(T.in, bytes);
    T.sigma = (const float*)st.in(T.sigma, n * sizeof(float));
    T.nd = (const float4_*)st.in(T.nd, bytes);
    T.h_rgba = (const float4_*)st.in(T.h_rgba, bytes);  // (all four null: the first frame)
    T.h_sigma = (const float*)st.in(T.h_sigma, n * sizeof(float));
    T.h_len = (const float*)st.in(T.h_len, n * sizeof(float));
    T.h_nd = (const float4_*)st.in(T.h_nd, bytes);
    float4_* d_out = (float4_*)st.out(rgba_out, bytes);
    float* d_sout = (float*)st.out(sigma_out, n * sizeof(float));
    float* d_lout = (float*)st.out(len_out, n * sizeof(float));
    if (int r = st.begin()) return r;
    const dim3 grid((w + TP_TW - 1) / TP_TW, (h + TP_TH - 1) / TP_TH);
    hipLaunchKernelGGL(k_temporal, grid, dim3(256), 0, st.s, T, d_out, d_sout, d_lout);
    HIPCHK(c, hipGetLastError());
    return st.end();
}
