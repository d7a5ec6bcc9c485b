// rt_noise.hip — gfx950 kernels and launches of a tracked progression's noise estimate
// (rt_noise.h). Its own translation unit, so that the render kernels of rt_render.hip compile
// exactly as they do without it.
//
//   k_noise_fold   one pixel per thread: one 16-B load of the state and of half, fold_pixel, one
//                  16-B store of half (48 B per pixel). Launched before an A pass (half -= state)
//                  and behind it (half += state), on the pass's stream.
//   k_noise_tiles  one wave64 per 8x8 tile, four tiles per 256-thread block (the last block may
//                  hold fewer; a wave without a tile leaves as a whole). Lane l owns pixel
//                  (8tx + l % 8, 8ty + l / 8): a tile row is 8 lanes x 16 B = 128 contiguous bytes
//                  of each buffer. The lane computes noise_pixel and writes the optional pixel
//                  map; the wave sums its 64 values by the xor butterfly (level j adds lane
//                  l ^ (1 << j): DPP quad permutes and row mirrors within 16 lanes, wave shuffles
//                  across rows and halves), which is the pairwise tree of rt_noise.h because IEEE
//                  addition is commutative; lane 0 writes the optional tile value and issues the
//                  frame's atomics (only those that change a word). No LDS, no barrier; all 64 lanes stay active through the
//                  butterfly (a lane outside the frame carries 0).
// The eight stat words {tiles, tiles_over, nonfinite, bits of max_tile, nA, nB, passes, 0} are
// zeroed on the stream ahead of k_noise_tiles; its first thread writes words 4..6.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "rt_backend_hip.h"
#include "rt_noise.h"

namespace {

constexpr int threads = 256;
constexpr int tiles_per_block = threads / 64;

__global__ __launch_bounds__(256) void k_noise_fold(float4_* __restrict__ half, const float4_* __restrict__ state, int n,
                                                    int add)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) half[i] = rtk::fold_pixel(half[i], state[i], add != 0);
}

// DPP controls: quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror (lane ^ 7), row_mirror (lane ^ 15)
template <int CTRL>
__device__ __forceinline__ float ndpp(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}

// Sum over the wave, in every lane: level j adds lane l ^ (1 << j). Levels 2 and 3 read lane
// l ^ 7 and l ^ 15: after levels 0..1 (0..2) the value is the same in all lanes of a group of
// 4 (8), so that lane holds what lane l ^ 4 (l ^ 8) holds. All values are >= 0 or +inf: no NaN
// whose payload could tell the operand order.
__device__ __forceinline__ float wave_tree_sum(float v)
{
    v = v + ndpp<0xB1>(v);
    v = v + ndpp<0x4E>(v);
    v = v + ndpp<0x141>(v);
    v = v + ndpp<0x140>(v);
    v = v + __shfl_xor(v, 16, 64);
    v = v + __shfl_xor(v, 32, 64);
    return v;
}

// state, half: w * rows float4 (w * rows <= (2^31 - 1) / 8: rt_capi_host.cpp progress_frame).
// pixel_err (w * rows floats) and tile_err (tw * th floats) may be null. st: 8 words.
__global__ __launch_bounds__(256) void k_noise_tiles(const float4_* __restrict__ state, const float4_* __restrict__ half,
                                                     int w, int rows, int tw, int n_tiles, rtk::NoiseArgs A,
                                                     float* __restrict__ pixel_err, float* __restrict__ tile_err,
                                                     uint32_t* __restrict__ st)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[4] = (uint32_t)A.samples_a;
        st[5] = (uint32_t)A.samples_b;
        st[6] = (uint32_t)A.passes;
    }
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * tiles_per_block + (threadIdx.x >> 6);  // (wave-uniform)
    if (t >= n_tiles) return;
    const int ty = t / tw, tx = t - ty * tw;
    const int x = rtk::NOISE_TILE * tx + (lane & 7), y = rtk::NOISE_TILE * ty + (lane >> 3);
    const bool in = x < w && y < rows;
    float v = 0.0f;
    bool bad = false;
    if (in) {
        const size_t i = (size_t)y * w + x;
        const float e = rtk::noise_pixel(state[i], half[i], A);
        if (pixel_err) pixel_err[i] = e;
        bad = !rtk::noise_finite(e);
        if (!bad) v = e;
    }
    const int n_bad = __popcll(__ballot(bad));
    const float sum = wave_tree_sum(v);
    if (lane == 0) {
        const float tile = sum / (float)rtk::noise_tile_count(tx, ty, w, rows);
        if (tile_err) tile_err[t] = tile;
        // All four words sit in one cache line and every atomic on it is served in turn (measured:
        // four per tile cost 1.1 ms at 1920x1080), so a tile issues only those that
        // change a word: the block's first wave counts the block's tiles, and the max is skipped
        // when the word already holds a value at least as large (it only ever grows, so a stale
        // read costs an atomic, never the answer).
        if ((threadIdx.x >> 6) == 0) {
            const int left = n_tiles - blockIdx.x * tiles_per_block;
            atomicAdd(&st[0], (uint32_t)(left < tiles_per_block ? left : tiles_per_block));
        }
        if (tile > A.threshold) atomicAdd(&st[1], 1u);
        if (n_bad) atomicAdd(&st[2], (uint32_t)n_bad);
        const uint32_t bits = __float_as_uint(tile);  // (tile >= 0: its bits order as the values do)
        if (bits > __atomic_load_n(&st[3], __ATOMIC_RELAXED)) atomicMax(&st[3], bits);
    }
}

int launch_fold(rt_context* c, float4_* half, const float4_* state, int n, bool add, hipStream_t s)
{
    hipLaunchKernelGGL(k_noise_fold, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, s, half, state, n,
                       add ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

int launch_tiles(rt_context* c, const float4_* state, const float4_* half, int w, int rows, const rtk::NoiseArgs& A,
                 float* pixel_err, float* tile_err, uint32_t* st, hipStream_t s)
{
    const int tw = (w + rtk::NOISE_TILE - 1) / rtk::NOISE_TILE, th = (rows + rtk::NOISE_TILE - 1) / rtk::NOISE_TILE;
    const int n_tiles = tw * th;
    HIPCHK(c, hipMemsetAsync(st, 0, 32, s));
    hipLaunchKernelGGL(k_noise_tiles, dim3((unsigned)((n_tiles + tiles_per_block - 1) / tiles_per_block)), dim3(threads),
                       0, s, state, half, w, rows, tw, n_tiles, A, pixel_err, tile_err, st);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

}  // namespace

int rt_noise_fold(rt_context* c, float4_* half, const float4_* state, int n, bool add, hipStream_t s)
{
    return launch_fold(c, half, state, n, add, s);
}

int rt_backend_progress_noise(rt_context* c, const rtk::NoiseArgs& A, int32_t* stats, float* pixel_err, float* tile_err,
                              bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    const RtProgress& P = c->prog;
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, b->own)) return r;
    const size_t n = P.npx(), n_tiles = (size_t)P.tiles_w() * P.tiles_h();
    // host form: the stat words, then the maps asked for
    if (int r = st.staging(b->pg_noise, 32 + (pixel_err ? st.pad(4 * n) : 0) + (tile_err ? 4 * n_tiles : 0))) return r;
    uint32_t* d_st = (uint32_t*)st.out(stats, 32);
    float* d_px = (float*)st.out(pixel_err, 4 * n);
    float* d_tl = (float*)st.out(tile_err, 4 * n_tiles);
    if (int r = b->ev_done.wait(c, st.s)) return r;  // (the last pass and its fold)
    // (a device query re-records ev_pg below: what an earlier device resolve recorded stays ahead of it)
    if (device)
        if (int r = b->ev_pg.wait(c, st.s)) return r;
    if (int r = st.begin()) return r;
    if (int r = launch_tiles(c, (const float4_*)b->pg_state.p, (const float4_*)b->pg_half.p, P.w, P.rows, A, d_px, d_tl,
                             d_st, st.s))
        return r;
    return st.end(&b->ev_pg);  // (device form: the next pass writes what this reads)
}

// MEASUREMENT HOOK, like rt_device_display_kernel_ms of rt_display.hip: exported by the gfx950
// library only, not part of include/rt_hip.h, never called by the product paths.
// GPU time of this stage's kernels (tools/noise_bench.py): for each of reps rounds, each of the
// three launches below runs alone on the default stream between two events recorded immediately
// before and after it. d_state, d_half: w*h float4 each (d_half is folded in place: -state, then
// +state in the next round); d_pixel: w*h floats; d_tile: ceil(w/8)*ceil(h/8) floats; d_stats: 8
// words. out_ms[k * reps + r]:
//   k = 0 k_noise_fold   1 k_noise_tiles without the pixel map   2 k_noise_tiles with it
// (1 and 2 include the 32-byte memset of the stat words ahead of the kernel).
extern "C" int rt_device_noise_kernel_ms(rt_context* c, int w, int h, const void* d_state, void* d_half, void* d_pixel,
                                         void* d_tile, void* d_stats, int reps, double* out_ms)
{
    if (w <= 0 || h <= 0 || (double)w * (double)h > 134217727.0 || !d_state || !d_half || !d_pixel || !d_tile || !d_stats)
        return rt_fail(c, RT_ERR_ARG, "rt_device_noise_kernel_ms: bad arguments");
    TimedRounds T;
    if (int r = T.enter(c, "rt_device_noise_kernel_ms", reps, out_ms)) return r;
    const rtk::NoiseArgs A{4.0f, 2.0f, 1.0f, 0.05f, 2, 2, 2};
    int folds = 0;  // (one a round: -state, then +state in the next)
    auto tiles = [&](float* pixel) {
        return [&, pixel] {
            return launch_tiles(c, (const float4_*)d_state, (const float4_*)d_half, w, h, A, pixel, (float*)d_tile,
                                (uint32_t*)d_stats, nullptr);
        };
    };
    auto fold = [&] { return launch_fold(c, (float4_*)d_half, (const float4_*)d_state, w * h, (folds++ & 1) != 0, nullptr); };
    return T.run(0, {TimedKernel::fixed(0, fold), TimedKernel::fixed(1, tiles(nullptr)), TimedKernel::fixed(2, tiles((float*)d_pixel))});
}
