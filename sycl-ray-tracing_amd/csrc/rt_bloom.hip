// rt_bloom.hip — gfx950 kernels and launch of the bloom stage (rt_bloom.h). Its own translation unit,
// so that the render kernels of rt_render.hip and the kernels of the other stages compile exactly as
// they do without it.
//
// A call of `levels` levels is 2 * levels launches on one stream: a reduce per level (the first one
// with the bright pass folded in: PRE), an expand-and-accumulate per level but the last, a composite.
// The pyramid's texels are float4 records (w = 0), levels 1..levels back to back in one buffer.
//   k_bloom_reduce_lds<PRE>     a block of 256 threads makes a 32 x 8 tile of level k from the 67 x 19
//                        texels of level k-1 under it, which it stages first: 16-B global loads along
//                        the rows, coordinates clamped to the level's edge, so every entry is written
//                        and a partial tile reads valid texels. With PRE the source is the frame and
//                        bl_bright is applied on the way in: the full-size bright-pass image is never
//                        written to memory. The tile is split by column parity: a row holds its 34 even
//                        columns, then its 33 odd ones (the footprint starts at column 2 * X0 - 2, which
//                        is even). The taps of output x sit at columns 2x .. 2x + 4 of the footprint, so
//                        they are entries x, x + 1, x + 2 of the even half and x, x + 1 of the odd half:
//                        the lanes of a row read consecutive 16-B records (ds_read_b128, banked by dword
//                        over 64 banks in groups of 16 lanes: 16 consecutive records are 64 distinct
//                        banks), where the same taps in one interleaved row sit two records apart, 8 lanes
//                        to a bank row and two lanes of every 16-lane group on the same banks: a 2-way
//                        conflict on each of the five reads. The horizontal pass (32 x 19 row sums, three
//                        rounds of the block) goes to a second array, the vertical pass reads five
//                        of its rows at unit stride. 67 * 19 + 32 * 19 records = 30096 B of LDS: five
//                        blocks to a CU. No thread returns before the last barrier; a thread outside
//                        the level computes from staged texels and does not store.
//   k_bloom_reduce_direct<PRE>  no LDS: a thread's 25 taps are clamped 16-B global loads (and with PRE 25
//                        bright passes). The yardstick that shows whether the tile pays.
//   k_bloom_expand       u_k = g_k + expand(u_{k+1}), in place on g_k: one 16-B load and store of the
//                        thread's own texel and four taps of the coarser level, a quarter of its size
//                        and in L2 from the launch before.
//   k_bloom_composite    the frame's pixel, four taps of u_1, the output pixel and, when given, the layer.
// The last two take k_firefly_direct's shape: 64 x 4 texels per block, a wave per row.
// Which reduce kernel a call takes: rt_backend_bloom.
#include <hip/hip_runtime.h>

#include <string>

#include "rt_backend_hip.h"
#include "rt_bloom.h"

namespace {

#define BL_TW 32                  // reduce: tile width in output texels ...
#define BL_TH 8                   // ... and height
#define BL_FW (2 * BL_TW + 3)     // the staged footprint's width (its pitch) ...
#define BL_FH (2 * BL_TH + 3)     // ... and height
#define BL_ODD (BL_TW + 2)        // where a row's odd columns start: behind its BL_TW + 2 even ones
#define BL_PW 64                  // expand and composite: block width (one wave per row) ...
#define BL_PH 4                   // ... and height

// One level of the pyramid on the device (level 0: the frame, read through bl_bright).
struct BlDev {
    float4_* g;
    int w, h;
};

template <bool PRE>
__device__ __forceinline__ float4_ bl_src(const rtk::BloomArgs& A, const float4_* __restrict__ src, int sw, int sh, int x, int y)
{
    const float4_ v = src[(size_t)rtk::bl_clampi(y, sh - 1) * sw + rtk::bl_clampi(x, sw - 1)];
    return PRE ? rtk::bl_bright(A, v) : v;
}

// What bl_reduce_texel asks of its source, over bl_src.
template <bool PRE>
struct BlGlobal {
    const rtk::BloomArgs& A;
    const float4_* __restrict__ src;
    int sw, sh;
    __device__ __forceinline__ float4_ at(int x, int y) const { return bl_src<PRE>(A, src, sw, sh, x, y); }
};

template <bool PRE>
__global__ __launch_bounds__(256) void k_bloom_reduce_direct(rtk::BloomArgs A, const float4_* __restrict__ src, int sw, int sh,
                                                             float4_* __restrict__ dst, int dw, int dh)
{
    const int x = blockIdx.x * BL_TW + (threadIdx.x & (BL_TW - 1));
    const int y = blockIdx.y * BL_TH + (threadIdx.x / BL_TW);
    if (x >= dw || y >= dh) return;
    const BlGlobal<PRE> F{A, src, sw, sh};
    dst[(size_t)y * dw + x] = rtk::bl_reduce_texel(F, x, y);
}

template <bool PRE>
__global__ __launch_bounds__(256) void k_bloom_reduce_lds(rtk::BloomArgs A, const float4_* __restrict__ src, int sw, int sh,
                                                          float4_* __restrict__ dst, int dw, int dh)
{
    __shared__ float4_ s_f[BL_FW * BL_FH];  // the footprint, each row its even columns then its odd ones
    __shared__ float4_ s_h[BL_TW * BL_FH];  // the row sums
    const int X0 = blockIdx.x * BL_TW, Y0 = blockIdx.y * BL_TH;
    const int sx0 = 2 * X0 - 2, sy0 = 2 * Y0 - 2;  // (even: a footprint column's parity is its source column's)
    for (int i = threadIdx.x; i < BL_FW * BL_FH; i += 256) {
        const int ly = i / BL_FW, lx = i - ly * BL_FW;
        s_f[ly * BL_FW + (lx & 1) * BL_ODD + (lx >> 1)] = bl_src<PRE>(A, src, sw, sh, sx0 + lx, sy0 + ly);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BL_TW * BL_FH; i += 256) {
        const int ly = i / BL_TW, xl = i & (BL_TW - 1);
        const float4_* e = s_f + ly * BL_FW + xl;  // footprint columns 2 xl, 2 xl + 2, 2 xl + 4 ...
        const float4_* o = e + BL_ODD;             // ... and 2 xl + 1, 2 xl + 3
        s_h[i] = rtk::bl_wsum5(e[0], o[0], e[1], o[1], e[2]);
    }
    __syncthreads();
    const int tx = threadIdx.x & (BL_TW - 1), ty = threadIdx.x / BL_TW;
    const float4_* col = s_h + (2 * ty) * BL_TW + tx;
    const float4_ v = rtk::bl_wsum5(col[0], col[BL_TW], col[2 * BL_TW], col[3 * BL_TW], col[4 * BL_TW]);
    const int x = X0 + tx, y = Y0 + ty;
    if (x < dw && y < dh) dst[(size_t)y * dw + x] = v;
}

__global__ __launch_bounds__(256) void k_bloom_expand(float4_* __restrict__ g, int w, int h, const float4_* __restrict__ u, int uw,
                                                      int uh)
{
    const int x = blockIdx.x * BL_PW + (threadIdx.x & (BL_PW - 1));
    const int y = blockIdx.y * BL_PH + (threadIdx.x / BL_PW);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    g[p] = rtk::bl_accumulate(g[p], rtk::BlLevel{u, uw, uh}, x, y);
}

__global__ __launch_bounds__(256) void k_bloom_composite(rtk::BloomArgs A, const float4_* __restrict__ u1, int uw, int uh,
                                                         float4_* __restrict__ out, float4_* __restrict__ layer_out)
{
    const int x = blockIdx.x * BL_PW + (threadIdx.x & (BL_PW - 1));
    const int y = blockIdx.y * BL_PH + (threadIdx.x / BL_PW);
    if (x >= A.w || y >= A.h) return;
    const size_t p = (size_t)y * A.w + x;
    float4_ layer;
    out[p] = rtk::bl_composite(A, A.in[p], rtk::BlLevel{u1, uw, uh}, x, y, layer);
    if (layer_out) layer_out[p] = layer;
}

template <bool PRE>
void bl_reduce(const rtk::BloomArgs& A, bool lds, const float4_* src, int sw, int sh, const BlDev& d, hipStream_t s)
{
    const dim3 grid((d.w + BL_TW - 1) / BL_TW, (d.h + BL_TH - 1) / BL_TH);
    if (lds) hipLaunchKernelGGL(k_bloom_reduce_lds<PRE>, grid, dim3(256), 0, s, A, src, sw, sh, d.g, d.w, d.h);
    else hipLaunchKernelGGL(k_bloom_reduce_direct<PRE>, grid, dim3(256), 0, s, A, src, sw, sh, d.g, d.w, d.h);
}

// The call's 2 * levels launches on s; A.in, out, layer (or null) and pyr are device pointers. ev, when
// given (the measurement hook), holds 2 * levels + 1 events: one recorded before each launch and one after the last.
int bl_run(rt_context* c, const rtk::BloomArgs& A, bool lds, float4_* out, float4_* layer, float4_* pyr, hipStream_t s,
           hipEvent_t* ev)
{
    BlDev L[rtk::BL_MAX_LEVELS + 1];
    L[0] = BlDev{nullptr, A.w, A.h};
    for (int k = 1; k <= A.levels; k++) {
        L[k] = BlDev{pyr, rtk::bl_half(L[k - 1].w), rtk::bl_half(L[k - 1].h)};
        pyr += (size_t)L[k].w * L[k].h;
    }
    int n_ev = 0;
    for (int k = 1; k <= A.levels; k++) {
        if (ev) HIPCHK(c, hipEventRecord(ev[n_ev++], s));
        if (k == 1) bl_reduce<true>(A, lds, A.in, A.w, A.h, L[1], s);
        else bl_reduce<false>(A, lds, L[k - 1].g, L[k - 1].w, L[k - 1].h, L[k], s);
    }
    for (int k = A.levels - 1; k >= 1; k--) {
        if (ev) HIPCHK(c, hipEventRecord(ev[n_ev++], s));
        const dim3 grid((L[k].w + BL_PW - 1) / BL_PW, (L[k].h + BL_PH - 1) / BL_PH);
        hipLaunchKernelGGL(k_bloom_expand, grid, dim3(256), 0, s, L[k].g, L[k].w, L[k].h, L[k + 1].g, L[k + 1].w, L[k + 1].h);
    }
    if (ev) HIPCHK(c, hipEventRecord(ev[n_ev++], s));
    const dim3 grid((A.w + BL_PW - 1) / BL_PW, (A.h + BL_PH - 1) / BL_PH);
    hipLaunchKernelGGL(k_bloom_composite, grid, dim3(256), 0, s, A, L[1].g, L[1].w, L[1].h, out, layer);
    if (ev) HIPCHK(c, hipEventRecord(ev[n_ev++], s));
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

}  // namespace

int rt_backend_bloom(rt_context* c, rtk::BloomArgs A, void* rgba_out, void* layer_out, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const size_t bytes = (size_t)A.w * A.h * sizeof(float4_);
    const size_t pyr_bytes = rtk::bl_pyramid_texels(A.w, A.h, A.levels) * sizeof(float4_);
    // One buffer: the pyramid and, in the host form, the frame and the two outputs in front of it. A device-form
    // call that has to grow it frees the old one first, which waits for the device: no earlier call still reads it.
    if (device) {
        if (int r = ensure(c, b->bloom, pyr_bytes)) return r;
    } else if (int r = st.staging(b->bloom, 3 * bytes + pyr_bytes)) return r;
    A.in = (const float4_*)st.in(A.in, bytes);
    float4_* d_out = (float4_*)st.out(rgba_out, bytes);
    float4_* d_layer = (float4_*)st.out(layer_out, bytes);  // (may be null)
    float4_* pyr = (float4_*)(device ? b->bloom.p : st.base + 3 * bytes);
    if (int r = st.begin()) return r;
    // Which reduce kernel the call takes (bloom_variant, rt_use_lds): the faster of the two as measured on the MI355X
    // (profiles/bloom_bench.json), LDS / direct ms: the first reduce (PRE, the frame to level 1) 0.015 /
    // 0.032 at 1920x1080 and 0.047 / 0.104 at 3840x2160, the second 0.007 / 0.008 and 0.013 / 0.015; from the third
    // level on both sit on the floor of a launch between two events, 0.0064. The whole call at 5 levels: 0.067 / 0.080
    // and 0.178 / 0.235. The tile wins wherever the two differ.
    const bool lds = rt_use_lds(c->sched.variant[RT_VAR_BLOOM], true);
    if (int r = bl_run(c, A, lds, d_out, d_layer, pyr, st.s, nullptr)) return r;
    return st.end();
}

// MEASUREMENT HOOK, like rt_device_upscale_kernel_ms of rt_upscale.hip: exported by the gfx950 library
// only, not part of include/rt_hip.h, never called by the product paths.
// GPU time of the call's launches (tools/bloom_bench.py): the product's sequence on the default stream with
// an event in front of each launch and one behind the last, reps times with the reduce kernel given by lds
// (0 direct, 1 the LDS tile). The arguments are validated by one rt_bloom_device call first.
// out_ms[r * 2 * levels + j]: launch j of round r, in launch order: `levels` reduces, levels - 1 expands
// from the coarsest level down, the composite.
extern "C" int rt_device_bloom_kernel_ms(rt_context* c, int w, int h, const void* d_in, const rt_bloom_params* params,
                                         void* d_out, void* d_layer, int lds, int reps, double* out_ms)
{
    // (not TimedRounds: the launches are timed in sequence, not alone, and laid out by round)
    if (!c || !c->backend || reps <= 0 || !out_ms) return rt_fail(c, RT_ERR_ARG, "rt_device_bloom_kernel_ms: bad arguments");
    if (int r = rt_bloom_device(c, w, h, d_in, params, d_out, d_layer, nullptr)) return r;
    rt_bloom_params p;
    if (params) p = *params;
    else rt_bloom_default_params(&p);
    Backend* b = rt_backend_dev0(c);
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    HIPCHK(c, hipStreamSynchronize(nullptr));
    const rtk::BloomArgs A{w, h, p.levels, p.threshold, p.knee, p.intensity / (float)p.levels, (const float4_*)d_in};
    const int n = 2 * p.levels;
    Event ev[2 * rtk::BL_MAX_LEVELS + 1];
    hipEvent_t raw[2 * rtk::BL_MAX_LEVELS + 1];
    for (int j = 0; j <= n; j++) {
        HIPCHK(c, hipEventCreate(&ev[j].h));
        raw[j] = ev[j].h;
    }
    for (int r = 0; r < reps; r++) {
        if (int e = bl_run(c, A, lds != 0, (float4_*)d_out, (float4_*)d_layer, (float4_*)b->bloom.p, nullptr, raw)) return e;
        HIPCHK(c, hipEventSynchronize(raw[n]));
        for (int j = 0; j < n; j++) {
            float ms = 0;
            HIPCHK(c, hipEventElapsedTime(&ms, raw[j], raw[j + 1]));
            out_ms[(size_t)r * n + j] = ms;
        }
    }
    return RT_OK;
}
