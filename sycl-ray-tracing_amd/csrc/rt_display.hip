// rt_display.hip — gfx950 kernels and launches of the display stage (rt_display.h): the
// exposure / gamma tone-map of a linear frame with the 8-bit conversion, and the linear
// resolve of a progression. Its own translation unit, so that the render kernels of
// rt_render.hip compile exactly as they do without it.
//
//   k_display<FLOAT_OUT, BYTE_OUT>  one pixel per thread: one 16-B load, display_pixel, then
//                  one 16-B store of the float pixel and / or one 4-B store of the packed
//                  8-bit pixel (at the mirrored row when the output is flipped). Which
//                  outputs exist is the instantiation, not a branch per thread. The float
//                  output may be the input: a thread reads its pixel before it writes it,
//                  and no thread reads another's.
//   k_resolve_linear  k_resolve (rt_render.hip) stopped before the tone-map: one thread per
//                  pixel of the shard, base and paused state in, base + state / done out.
// k_display fills rt_libm's LDS tables first (rt_expf / rt_powf read them).
#include <hip/hip_runtime.h>

#include <string>

#include "rt_backend_hip.h"
#include "rt_display.h"

namespace {

constexpr int threads = 256;

// n = w * h pixels (at most 2^27 - 1: rt_capi_stages.cpp); in and out may be one buffer
template <bool FLOAT_OUT, bool BYTE_OUT>
__global__ __launch_bounds__(256) void k_display(const float4_* in, float4_* out, uint32_t* out8, int n,
                                                 int w, int h, int flip, float exposure, float inv_gamma)
{
    rtlibm::lds_tables_init();  // (before any thread leaves: it has a barrier)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4_ px = rtk::display_pixel(in[i], exposure, inv_gamma);
    if (FLOAT_OUT) out[i] = px;
    if (BYTE_OUT) {
        int j = i;
        if (flip) {
            const int y = i / w, x = i - y * w;
            j = (h - 1 - y) * w + x;
        }
        out8[j] = rtk::pack_rgba8(px);
    }
}

__global__ __launch_bounds__(256) void k_resolve_linear(const float4_* __restrict__ base,
                                                        const float4_* __restrict__ state, float4_* __restrict__ out,
                                                        int n, int done)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rtk::resolve_linear_pixel(base[i], state[i], done);
}

int launch_display(rt_context* c, const float4_* in, float4_* out, uint32_t* out8, int w, int h, bool flip,
                   float exposure, float inv_gamma, hipStream_t s)
{
    const int n = w * h;
    const dim3 grid((unsigned)((n + threads - 1) / threads)), block(threads);
    const int f = flip ? 1 : 0;
    if (out && out8)
        hipLaunchKernelGGL((k_display<true, true>), grid, block, 0, s, in, out, out8, n, w, h, f, exposure, inv_gamma);
    else if (out)
        hipLaunchKernelGGL((k_display<true, false>), grid, block, 0, s, in, out, out8, n, w, h, f, exposure, inv_gamma);
    else
        hipLaunchKernelGGL((k_display<false, true>), grid, block, 0, s, in, out, out8, n, w, h, f, exposure, inv_gamma);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

}  // namespace

int rt_backend_display(rt_context* c, int w, int h, const void* in, float exposure, float inv_gamma, bool flip,
                       void* out, void* out8, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const size_t n = (size_t)w * h, fbytes = n * sizeof(float4_), bbytes = n * 4;
    if (int r = st.staging(b->disp, fbytes + bbytes)) return r;
    // host form: the frame, tone-mapped in place when the float output is asked for; the bytes behind it
    const float4_* d_in = (const float4_*)st.inout(in, out, fbytes);
    float4_* d_out = device ? (float4_*)out : out ? (float4_*)d_in : nullptr;
    uint32_t* d_out8 = (uint32_t*)st.out(out8, bbytes);
    if (int r = st.begin()) return r;
    if (int r = launch_display(c, d_in, d_out, d_out8, w, h, flip, exposure, inv_gamma, st.s)) return r;
    return st.end();
}

int rt_display_resolve_linear(rt_context* c, const float4_* base, const float4_* state, float4_* out, int n, int done,
                              hipStream_t s)
{
    hipLaunchKernelGGL(k_resolve_linear, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, s, base, state,
                       out, n, done);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

// MEASUREMENT HOOK, like rt_device_denoise_pass_ms of rt_denoise.hip: exported by the gfx950
// library only, not part of include/rt_hip.h, never called by the product paths.
// GPU time of this stage's kernels and of k_resolve on one footing (tools/display_bench.py):
// for each of reps rounds, each of the six launches below runs alone on the default stream
// between two events recorded immediately before and after it, with nothing else between the
// events. d_in, d_state, d_out: w*h float4 each; d_out8: w*h words. out_ms[k * reps + r]:
//   k = 0 k_resolve (d_in as the base, d_state, done 1)   1 k_resolve_linear (the same)
//       2 k_display float out   3 8-bit out   4 8-bit out, flipped   5 both outputs
extern "C" int rt_device_display_kernel_ms(rt_context* c, int w, int h, const void* d_in, const void* d_state,
                                           void* d_out, void* d_out8, int reps, double* out_ms)
{
    if (w <= 0 || h <= 0 || (double)w * (double)h > 134217727.0 || !d_in || !d_state || !d_out || !d_out8)
        return rt_fail(c, RT_ERR_ARG, "rt_device_display_kernel_ms: bad arguments");
    TimedRounds T;
    if (int r = T.enter(c, "rt_device_display_kernel_ms", reps, out_ms)) return r;
    const int n = w * h;
    const float4_ *in = (const float4_*)d_in, *state = (const float4_*)d_state;
    float4_* out = (float4_*)d_out;
    uint32_t* out8 = (uint32_t*)d_out8;
    const float ex = 1.5f, ig = 1.0f / 2.2f;
    using K = TimedKernel;
    return T.run(0, {K::fixed(0, [&] { return rt_wave_resolve(c, in, state, out, n, 1, nullptr); }),
                     K::fixed(1, [&] { return rt_display_resolve_linear(c, in, state, out, n, 1, nullptr); }),
                     K::fixed(2, [&] { return launch_display(c, in, out, nullptr, w, h, false, ex, ig, nullptr); }),
                     K::fixed(3, [&] { return launch_display(c, in, nullptr, out8, w, h, false, ex, ig, nullptr); }),
                     K::fixed(4, [&] { return launch_display(c, in, nullptr, out8, w, h, true, ex, ig, nullptr); }),
                     K::fixed(5, [&] { return launch_display(c, in, out, out8, w, h, false, ex, ig, nullptr); })});
}
