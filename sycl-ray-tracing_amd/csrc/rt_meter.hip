// rt_meter.hip — gfx950 kernels and launch of the exposure metering stage (rt_meter.h). Its own
// translation unit, so that the render kernels of rt_render.hip and the kernels of the other post
// stages compile exactly as they do without it.
//
// The first whole-frame reduction of the post stack. Both kernels walk the frame grid-stride with a
// capped grid of 256-thread blocks, one 16-B load per pixel, coalesced along the row; every
// accumulator is an integer, so no order of the adds changes a word of the result.
//   k_meter_lds     each wave owns a copy of the 256 bins in LDS (4 x 256 x 4 B = 4 KB a block, plus 8
//                   stat words). The five counters are kept per wave as the population counts of ballots
//                   (scalar registers, no atomics); max_bits / min_bits per thread, reduced across the
//                   wave once after the walk. The bin add is one LDS atomic add of 1 per lane. A flat
//                   image sends all 64 lanes of a wave to one bin; counting the lanes that share the
//                   first binned lane's bin with a ballot, so that one lane adds the count, was built
//                   (MT_PEEL rounds of it in front of the per-lane add) and measured: it is slower on
//                   the rendered and the noise frame and within 4 % on the constant one, so it is
//                   compiled out (MT_PEEL 0). After the walk and a barrier thread t sums
//                   bin t of the four copies and issues one global atomicAdd if the sum is not zero;
//                   seven threads flush the stat words (atomicMax / atomicMin for the two bit words).
//                   The flush is at most blocks x 263 global atomics, bounded by the grid cap.
//   k_meter_direct  the yardstick: no LDS, a global atomicAdd per pixel on its bin and on the stat
//                   words; the compiler's per-wave coalescing of a uniform-address atomicAdd(p, 1) is
//                   all the help it gets. 600 to 1700 times slower on a rendered or a constant frame.
// meter_pixel evaluates no expf, so rtlibm::lds_tables_init() is not called here.
// Which kernel a call takes: rt_backend_meter; the grid: mt_grid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "rt_backend_hip.h"
#include "rt_meter.h"

namespace {

constexpr int threads = 256, waves = threads / 64;
#ifndef MT_PEEL
#define MT_PEEL 0  // ballot rounds in front of the per-lane LDS add (0, 1 and 2 measured)
#endif
#ifndef MT_BLOCKS_PER_CU
#define MT_BLOCKS_PER_CU 2  // the grid cap (the flush against the walk)
#endif

// n = w * h pixels (at most 2^27 - 1: rt_capi_stages.cpp) and at most 65536 blocks (mt_grid), so
// base + gridDim.x * 256 stays below 2^28.
__global__ __launch_bounds__(256) void k_meter_direct(const float4_* __restrict__ in, unsigned n, uint32_t* __restrict__ hist)
{
    for (unsigned base = blockIdx.x * (unsigned)threads; base < n; base += gridDim.x * (unsigned)threads) {
        const unsigned i = base + threadIdx.x;
        if (i >= n) continue;
        const rtk::MeterPixel m = rtk::meter_pixel(in[i]);
        if (m.bin == rtk::MT_IS_NONFINITE) {
            atomicAdd(&hist[rtk::MT_NONFINITE], 1u);
        } else if (m.bin == rtk::MT_IS_NONPOSITIVE) {
            atomicAdd(&hist[rtk::MT_NONPOSITIVE], 1u);
        } else {
            const uint32_t k = m.bits >> 20;
            atomicAdd(&hist[m.bin], 1u);
            atomicAdd(&hist[rtk::MT_COUNTED], 1u);
            if (k < rtk::MT_K0) atomicAdd(&hist[rtk::MT_UNDER], 1u);
            if (k > rtk::MT_K1) atomicAdd(&hist[rtk::MT_OVER], 1u);
            atomicMax(&hist[rtk::MT_MAX_BITS], m.bits);
            atomicMin(&hist[rtk::MT_MIN_BITS], m.bits);
        }
    }
}

__device__ __forceinline__ uint32_t mt_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__global__ __launch_bounds__(256) void k_meter_lds(const float4_* __restrict__ in, unsigned n, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_bins[waves][rtk::MT_BINS];
    __shared__ uint32_t s_stat[8];  // the words behind the bins, in rt_meter_hist's order
    const int t = threadIdx.x, lane = t & 63;
    uint32_t* const mine = s_bins[t >> 6];
    for (int j = t; j < waves * rtk::MT_BINS; j += threads) (&s_bins[0][0])[j] = 0;
    if (t < 8) s_stat[t] = t == rtk::MT_MIN_BITS - rtk::MT_BINS ? 0xffffffffu : 0u;
    __syncthreads();
    uint32_t counted = 0, under = 0, over = 0, nonpositive = 0, nonfinite = 0;  // (the same in every lane of a wave)
    uint32_t vmax = 0, vmin = 0xffffffffu;
    // (the trip count is the block's, so every ballot is taken with the wave's 64 lanes together)
    for (unsigned base = blockIdx.x * (unsigned)threads; base < n; base += gridDim.x * (unsigned)threads) {
        const unsigned i = base + t;
        const bool valid = i < n;
        rtk::MeterPixel m{rtk::MT_IS_NONFINITE, 0};
        if (valid) m = rtk::meter_pixel(in[i]);
        const bool binned = valid && m.bin >= 0;
        const uint32_t k = m.bits >> 20;
        nonfinite += mt_count(valid && m.bin == rtk::MT_IS_NONFINITE);
        nonpositive += mt_count(valid && m.bin == rtk::MT_IS_NONPOSITIVE);
        under += mt_count(binned && k < rtk::MT_K0);
        over += mt_count(binned && k > rtk::MT_K1);
        if (binned) {
            vmax = m.bits > vmax ? m.bits : vmax;
            vmin = m.bits < vmin ? m.bits : vmin;
        }
        unsigned long long todo = __ballot(binned);
        counted += (uint32_t)__popcll(todo);
#pragma unroll
        for (int r = 0; r < MT_PEEL; r++) {
            if (!todo) break;
            const int first = __ffsll((long long)todo) - 1;
            const int lead = __builtin_amdgcn_readlane(m.bin, first);
            const unsigned long long same = __ballot(binned && m.bin == lead);
            if (lane == first) atomicAdd(&mine[lead], (uint32_t)__popcll(same));
            todo &= ~same;
        }
        if ((todo >> lane) & 1ull) atomicAdd(&mine[m.bin], 1u);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t a = (uint32_t)__shfl_xor((int)vmax, d), b = (uint32_t)__shfl_xor((int)vmin, d);
        vmax = a > vmax ? a : vmax;
        vmin = b < vmin ? b : vmin;
    }
    if (lane == 0) {
        if (counted) {
            atomicAdd(&s_stat[0], counted);
            atomicMax(&s_stat[5], vmax);
            atomicMin(&s_stat[6], vmin);
        }
        if (under) atomicAdd(&s_stat[1], under);
        if (over) atomicAdd(&s_stat[2], over);
        if (nonpositive) atomicAdd(&s_stat[3], nonpositive);
        if (nonfinite) atomicAdd(&s_stat[4], nonfinite);
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int v = 0; v < waves; v++) sum += s_bins[v][t];
    if (sum) atomicAdd(&hist[t], sum);
    if (t < 5) {
        if (s_stat[t]) atomicAdd(&hist[rtk::MT_BINS + t], s_stat[t]);
    } else if (t == 5) {
        if (s_stat[0]) atomicMax(&hist[rtk::MT_MAX_BITS], s_stat[5]);
    } else if (t == 6) {
        if (s_stat[0]) atomicMin(&hist[rtk::MT_MIN_BITS], s_stat[6]);
    }
}

// The grid. A block costs its flush (up to 263 global atomics on words every block adds to) and a
// round of 256 pixels costs a block its time, so with R rounds in the frame the time is about
// a R / B + b B and smallest at B = sqrt(a R / b). Measured on the MI355X (profiles/meter_bench.json,
// the forced block counts): 1920x1080 (R = 8100) is fastest at 256 blocks of {128, 256, 512, 1024} and
// 3840x2160 (R = 32400) at 512; B = sqrt(8 R) gives 254 and 509. Capped at MT_BLOCKS_PER_CU blocks a
// CU, which bounds the flush for any frame size. mt_blocks > 0 (rt_test_schedule) forces the count.
unsigned mt_grid(size_t n, int cus, int forced)
{
    const size_t rounds = (n + threads - 1) / threads;
    if (forced > 0) return (unsigned)std::min(forced, 65536);
    const size_t b = (size_t)std::sqrt(8.0 * (double)rounds);  // (at least 2: rounds >= 1)
    return (unsigned)std::min(std::min(rounds, b), (size_t)std::max(cus, 1) * MT_BLOCKS_PER_CU);
}

}  // namespace

// The device's compute units (Backend::cus), asked on first use.
static int meter_cus(rt_context* c, Backend* b)
{
    if (!b->cus) HIPCHK(c, hipDeviceGetAttribute(&b->cus, hipDeviceAttributeMultiprocessorCount, b->device));
    return RT_OK;
}

int rt_backend_meter(rt_context* c, int w, int h, const void* in, void* hist, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    if (int r = meter_cus(c, b)) return r;
    const size_t n = (size_t)w * h, bytes = n * sizeof(float4_), hbytes = rtk::MT_WORDS * sizeof(uint32_t);
    if (int r = st.staging(b->meter_io, bytes + st.pad(hbytes))) return r;
    const float4_* d_in = (const float4_*)st.in(in, bytes);
    uint32_t* d_hist = (uint32_t*)st.out(hist, hbytes);
    if (int r = st.begin()) return r;
    // the histogram starts at zero, min_bits at all ones: the caller need not clear it
    HIPCHK(c, hipMemsetAsync(d_hist, 0, hbytes, st.s));
    HIPCHK(c, hipMemsetAsync(d_hist + rtk::MT_MIN_BITS, 0xff, sizeof(uint32_t), st.s));
    const dim3 grid(mt_grid(n, b->cus, c->sched.mt_blocks));
    // Which kernel the call takes (mt_variant, rt_use_lds): the faster of the two as measured on the MI355X
    // (profiles/meter_bench.json), the LDS kernel.
    if (rt_use_lds(c->sched.variant[RT_VAR_MT], true))
        hipLaunchKernelGGL(k_meter_lds, grid, dim3(threads), 0, st.s, d_in, (unsigned)n, d_hist);
    else
        hipLaunchKernelGGL(k_meter_direct, grid, dim3(threads), 0, st.s, d_in, (unsigned)n, d_hist);
    HIPCHK(c, hipGetLastError());
    return st.end();
}

// MEASUREMENT HOOK, like rt_device_display_kernel_ms of rt_display.hip: exported by the gfx950
// library only, not part of include/rt_hip.h, never called by the product paths.
// GPU time of the two kernels on one footing (tools/meter_bench.py): for each of reps rounds each
// kernel runs alone on the default stream between two events recorded immediately before and after
// it; the histogram is cleared in front of the first event. blocks: 0 the product's cap, n > 0 that
// many blocks. d_in: w*h float4; d_hist: 264 words. out_ms[k * reps + r]: k = 0 k_meter_direct, 1 k_meter_lds.
extern "C" int rt_device_meter_kernel_ms(rt_context* c, int w, int h, const void* d_in, void* d_hist, int blocks, int reps,
                                         double* out_ms)
{
    if (w <= 0 || h <= 0 || (double)w * (double)h > 134217727.0 || !d_in || !d_hist || blocks < 0)
        return rt_fail(c, RT_ERR_ARG, "rt_device_meter_kernel_ms: bad arguments");
    TimedRounds T;
    if (int r = T.enter(c, "rt_device_meter_kernel_ms", reps, out_ms)) return r;
    Backend* b = rt_backend_dev0(c);
    if (int r = meter_cus(c, b)) return r;
    const size_t n = (size_t)w * h;
    const dim3 grid(mt_grid(n, b->cus, blocks));
    uint32_t* hist = (uint32_t*)d_hist;
    auto clear = [&]() -> int {
        HIPCHK(c, hipMemsetAsync(hist, 0, rtk::MT_WORDS * sizeof(uint32_t), nullptr));
        HIPCHK(c, hipMemsetAsync(hist + rtk::MT_MIN_BITS, 0xff, sizeof(uint32_t), nullptr));
        return RT_OK;
    };
    auto kernel = [&](bool lds) {
        return [&, lds]() -> int {
            if (lds) hipLaunchKernelGGL(k_meter_lds, grid, dim3(threads), 0, nullptr, (const float4_*)d_in, (unsigned)n, hist);
            else hipLaunchKernelGGL(k_meter_direct, grid, dim3(threads), 0, nullptr, (const float4_*)d_in, (unsigned)n, hist);
            HIPCHK(c, hipGetLastError());
            return RT_OK;
        };
    };
    return T.run(0, {TimedKernel::fixed(0, kernel(false), clear), TimedKernel::fixed(1, kernel(true), clear)});
}
