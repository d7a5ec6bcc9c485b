// rt_adapt.hip — gfx950 kernels and launches of an adaptive progression (rt_adapt.h). Its own
// translation unit, so that the render kernels of rt_render.hip compile exactly as they do
// without it. The pass itself is run_wave over the compact pixel list (rt_backend.hip).
//
//   k_adapt_tiles    k_noise_tiles (rt_noise.hip) with the three count-derived floats worked out per
//                    tile from tile_n / tile_nA instead of passed in: one wave64 per 8x8 tile, lane l
//                    owns pixel (8tx + l % 8, 8ty + l / 8), the same xor butterfly and atomics.
//   k_adapt_select   one block of 1024 threads walks the tiles in steps of 1024: flags (rt_adapt.h
//                    adapt_flags), a block-wide exclusive scan of the active flags and of the active
//                    tiles' pixel counts (ballot / shuffle scan inside a wave, 16 wave totals in LDS,
//                    a running carry), so the list is in ascending t whatever the timing; updates the
//                    counts and writes the header.
//   k_adapt_gather   one wave64 per active tile, k_noise_tiles' lane map: a tile row is 128 contiguous
//                    bytes of the state. In-frame lanes rank themselves by ballot + mbcnt (row-major
//                    within the tile) and write slot tile_off + rank of xy / idx / cstate; on an A pass
//                    the lane also folds half -= state (rt_noise.h fold_pixel).
//   k_adapt_scatter  one thread per slot: state[idx] = cstate; on an A pass half[idx] += cstate.
//   k_adapt_bump     a uniform pass keeps the counts in step.
//   k_adapt_resolve  k_resolve / k_resolve_linear with tile_n[tile of the pixel] for `done`.
// Every index is bounded by construction: slots by the prefix sums over the same flags the list
// holds, pixels by the in-frame test, tiles by n_tiles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "rt_adapt.h"
#include "rt_backend_hip.h"
#include "rt_display.h"
#include "rt_wave.h"

namespace {

constexpr int threads = 256;
constexpr int tiles_per_block = threads / 64;
constexpr int select_threads = 1024;  // one scan step (tests/adapt_cases.py has a frame of more tiles)

// DPP controls: quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror (lane ^ 7), row_mirror (lane ^ 15)
template <int CTRL>
__device__ __forceinline__ float adpp(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}

// rt_noise.hip's wave_tree_sum: level j adds lane l ^ (1 << j), the pairwise tree of rt_noise.h.
__device__ __forceinline__ float wave_tree_sum(float v)
{
    v = v + adpp<0xB1>(v);
    v = v + adpp<0x4E>(v);
    v = v + adpp<0x141>(v);
    v = v + adpp<0x140>(v);
    v = v + __shfl_xor(v, 16, 64);
    v = v + __shfl_xor(v, 32, 64);
    return v;
}

// F: threshold and the stat words 4..6. pixel_err, tile_err and st may be null (the selection
// wants the tile values only).
__global__ __launch_bounds__(256) void k_adapt_tiles(const float4_* __restrict__ state, const float4_* __restrict__ half,
                                                     const int32_t* __restrict__ tile_n, const int32_t* __restrict__ tile_nA,
                                                     int w, int rows, int tw, int n_tiles, rtk::NoiseArgs F,
                                                     float* __restrict__ pixel_err, float* __restrict__ tile_err,
                                                     uint32_t* __restrict__ st)
{
    if (st && blockIdx.x == 0 && threadIdx.x == 0) {
        st[4] = (uint32_t)F.samples_a;
        st[5] = (uint32_t)F.samples_b;
        st[6] = (uint32_t)F.passes;
    }
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * tiles_per_block + (threadIdx.x >> 6);  // (wave-uniform)
    if (t >= n_tiles) return;
    const rtk::NoiseArgs A = rtk::adapt_tile_args(tile_n[t], tile_nA[t], F);
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
        if (!st) return;
        // (only the atomics that change a word, as k_noise_tiles)
        if ((threadIdx.x >> 6) == 0) {
            const int left = n_tiles - blockIdx.x * tiles_per_block;
            atomicAdd(&st[0], (uint32_t)(left < tiles_per_block ? left : tiles_per_block));
        }
        if (tile > F.threshold) atomicAdd(&st[1], 1u);
        if (n_bad) atomicAdd(&st[2], (uint32_t)n_bad);
        const uint32_t bits = __float_as_uint(tile);
        if (bits > __atomic_load_n(&st[3], __ATOMIC_RELAXED)) atomicMax(&st[3], bits);
    }
}

// Inclusive sum over the wave's lanes 0..lane.
__device__ __forceinline__ int wave_scan(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// One block. err: n_tiles floats (read when estimate). list, off: n_tiles int32 each. hdr: AD_WORDS.
__global__ __launch_bounds__(1024) void k_adapt_select(const float* __restrict__ err, int32_t* __restrict__ tile_n,
                                                       int32_t* __restrict__ tile_nA, int n_tiles, int tw, int w, int rows,
                                                       int samples, int total, float threshold, int estimate, int a_pass,
                                                       int32_t* __restrict__ list, int32_t* __restrict__ off,
                                                       int32_t* __restrict__ hdr)
{
    __shared__ int w_tiles[select_threads / 64], w_px[select_threads / 64];
    __shared__ int carry[2], capped, n_min, n_max;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) {
        carry[0] = carry[1] = 0;
        capped = 0;
        n_min = 0x7fffffff;
        n_max = (int)0x80000000;
    }
    __syncthreads();
    for (int first = 0; first < n_tiles; first += select_threads) {
        const int t = first + tid;
        const bool valid = t < n_tiles;
        int flags = 0, px = 0, n = 0;
        if (valid) {
            n = tile_n[t];
            flags = rtk::adapt_flags(n, samples, total, estimate != 0, estimate ? err[t] : 0.0f, threshold);
        }
        const bool active = (flags & rtk::ADAPT_ACTIVE) != 0;
        if (active) {
            const int ty = t / tw, tx = t - ty * tw;
            px = rtk::noise_tile_count(tx, ty, w, rows);
        }
        // the wave's part of the two scans
        const unsigned long long m = __ballot(active);
        const int rank_w = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const int px_incl = wave_scan(px, lane);
        if (lane == 63) {
            w_tiles[wv] = __popcll(m);
            w_px[wv] = px_incl;
        }
        // the counts' update and the header's capped / min / max
        if (valid) {
            if (active) {
                n += samples;
                tile_n[t] = n;
                if (a_pass) tile_nA[t] += samples;
            }
            atomicMin(&n_min, n);
            atomicMax(&n_max, n);
            if (flags & rtk::ADAPT_CAPPED) atomicAdd(&capped, 1);
        }
        __syncthreads();
        int before_t = carry[0], before_p = carry[1];
        for (int k = 0; k < wv; k++) before_t += w_tiles[k], before_p += w_px[k];
        if (active) {
            const int a = before_t + rank_w;  // (< n_tiles: at most one entry per tile)
            list[a] = t;
            off[a] = before_p + px_incl - px;
        }
        __syncthreads();
        if (tid == 0) {
            int st = 0, sp = 0;
            for (int k = 0; k < select_threads / 64; k++) st += w_tiles[k], sp += w_px[k];
            carry[0] += st;
            carry[1] += sp;
        }
        __syncthreads();
    }
    if (tid == 0) {
        hdr[rtk::AD_TILES_ACTIVE] = carry[0];
        hdr[rtk::AD_PIXELS] = carry[1];
        hdr[rtk::AD_CAPPED] = capped;
        hdr[rtk::AD_MIN] = n_min;
        hdr[rtk::AD_MAX] = n_max;
        hdr[rtk::AD_TILES] = n_tiles;
        hdr[6] = 0;
        hdr[7] = 0;
    }
}

// state, half: w * rows float4. list, off: n_active entries. xy: 2 int32 per slot, idx: one, cstate: one float4.
__global__ __launch_bounds__(256) void k_adapt_gather(const float4_* __restrict__ state, float4_* __restrict__ half,
                                                      const int32_t* __restrict__ list, const int32_t* __restrict__ off,
                                                      int n_active, int w, int rows, int tw, int row_off, int row_stride,
                                                      int a_pass, int32_t* __restrict__ xy, int32_t* __restrict__ idx,
                                                      float4_* __restrict__ cstate)
{
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * tiles_per_block + (threadIdx.x >> 6);  // (wave-uniform)
    if (a >= n_active) return;
    const int t = list[a], base = off[a];
    const int ty = t / tw, tx = t - ty * tw;
    const int x = rtk::NOISE_TILE * tx + (lane & 7), y = rtk::NOISE_TILE * ty + (lane >> 3);
    const bool in = x < w && y < rows;
    const unsigned long long m = __ballot(in);
    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (!in) return;
    const int p = y * w + x;
    const size_t slot = (size_t)base + rank;
    const float4_ st = state[p];
    xy[2 * slot] = x;
    xy[2 * slot + 1] = row_off + y * row_stride;  // (the true image row: the seed uses it)
    idx[slot] = p;
    cstate[slot] = st;
    if (a_pass) half[p] = rtk::fold_pixel(half[p], st, false);
}

__global__ __launch_bounds__(256) void k_adapt_scatter(float4_* __restrict__ state, float4_* __restrict__ half,
                                                       const int32_t* __restrict__ idx, const float4_* __restrict__ cstate,
                                                       int n, int a_pass)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = idx[i];
    const float4_ st = cstate[i];
    state[p] = st;
    if (a_pass) half[p] = rtk::fold_pixel(half[p], st, true);
}

__global__ __launch_bounds__(256) void k_adapt_bump(int32_t* __restrict__ tile_n, int32_t* __restrict__ tile_nA, int n_tiles,
                                                    int samples, int a_pass)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    tile_n[t] += samples;
    if (a_pass) tile_nA[t] += samples;
}

template <bool LINEAR>
__global__ __launch_bounds__(256) void k_adapt_resolve(const float4_* __restrict__ base, const float4_* __restrict__ state,
                                                       const int32_t* __restrict__ tile_n, float4_* __restrict__ out, int n,
                                                       int w, int tw)
{
    if (!LINEAR) rtlibm::lds_tables_init();  // (before any thread leaves: it has a barrier)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int done = tile_n[rtk::adapt_tile_of(i, w, tw)];
    out[i] = LINEAR ? rtk::resolve_linear_pixel(base[i], state[i], done) : rtk::resolve_pixel(base[i], state[i], done);
}

dim3 grid_of(size_t n, int per_block) { return dim3((unsigned)((n + per_block - 1) / per_block)); }

int launch_tiles(rt_context* c, const Backend* b, const rtk::NoiseArgs& F, float* pixel_err, float* tile_err, uint32_t* st,
                 hipStream_t s)
{
    const RtProgress& P = c->prog;
    const Adapt& ad = *b->adapt;
    const int n_tiles = P.tiles_w() * P.tiles_h();
    if (st) HIPCHK(c, hipMemsetAsync(st, 0, 32, s));
    hipLaunchKernelGGL(k_adapt_tiles, grid_of(n_tiles, tiles_per_block), dim3(threads), 0, s, (const float4_*)b->pg_state.p,
                       (const float4_*)b->pg_half.p, (const int32_t*)ad.tile_n.p, (const int32_t*)ad.tile_nA.p, P.w, P.rows,
                       P.tiles_w(), n_tiles, F, pixel_err, tile_err, st);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

int launch_select(rt_context* c, const Backend* b, int samples, float threshold, bool estimate, bool a_pass, hipStream_t s)
{
    const RtProgress& P = c->prog;
    const Adapt& ad = *b->adapt;
    hipLaunchKernelGGL(k_adapt_select, dim3(1), dim3(select_threads), 0, s, (const float*)ad.err.p, (int32_t*)ad.tile_n.p,
                       (int32_t*)ad.tile_nA.p, P.tiles_w() * P.tiles_h(), P.tiles_w(), P.w, P.rows, samples, P.total,
                       threshold, estimate ? 1 : 0, a_pass ? 1 : 0, (int32_t*)ad.list.p, (int32_t*)ad.off.p,
                       (int32_t*)ad.hdr.p);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

}  // namespace

int rt_adapt_select(rt_context* c, Backend* b, int samples, float threshold, bool estimate, bool a_pass, int32_t* hdr,
                    hipStream_t s)
{
    const RtProgress& P = c->prog;
    Adapt& ad = *b->adapt;
    const size_t n_tiles = (size_t)P.tiles_w() * P.tiles_h();
    if (int r = ensure(c, ad.err, 4 * n_tiles)) return r;
    if (int r = ensure(c, ad.list, 4 * n_tiles)) return r;
    if (int r = ensure(c, ad.off, 4 * n_tiles)) return r;
    if (int r = ensure(c, ad.hdr, 4 * rtk::AD_WORDS)) return r;
    if (!ad.h_hdr) HIPCHK(c, hipHostMalloc((void**)&ad.h_hdr.h, 4 * rtk::AD_WORDS, hipHostMallocDefault));
    if (estimate) {
        rtk::NoiseArgs F{};
        F.threshold = threshold;
        if (int r = launch_tiles(c, b, F, nullptr, (float*)ad.err.p, nullptr, s)) return r;
    }
    if (int r = launch_select(c, b, samples, threshold, estimate, a_pass, s)) return r;
    HIPCHK(c, hipMemcpyAsync(ad.h_hdr.h, ad.hdr.p, 4 * rtk::AD_WORDS, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (int i = 0; i < rtk::AD_WORDS; i++) hdr[i] = ad.h_hdr.h[i];
    return RT_OK;
}

int rt_adapt_gather(rt_context* c, Backend* b, int n_active, bool a_pass, hipStream_t s)
{
    const RtProgress& P = c->prog;
    const Adapt& ad = *b->adapt;
    hipLaunchKernelGGL(k_adapt_gather, grid_of(n_active, tiles_per_block), dim3(threads), 0, s, (const float4_*)b->pg_state.p,
                       (float4_*)b->pg_half.p, (const int32_t*)ad.list.p, (const int32_t*)ad.off.p, n_active, P.w, P.rows,
                       P.tiles_w(), P.off, P.stride, a_pass ? 1 : 0, (int32_t*)ad.xy.p, (int32_t*)ad.idx.p,
                       (float4_*)ad.cstate.p);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

int rt_adapt_scatter(rt_context* c, Backend* b, int n_pixels, bool a_pass, hipStream_t s)
{
    const Adapt& ad = *b->adapt;
    hipLaunchKernelGGL(k_adapt_scatter, grid_of(n_pixels, threads), dim3(threads), 0, s, (float4_*)b->pg_state.p,
                       (float4_*)b->pg_half.p, (const int32_t*)ad.idx.p, (const float4_*)ad.cstate.p, n_pixels,
                       a_pass ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

int rt_adapt_bump(rt_context* c, Backend* b, int samples, bool a_pass, hipStream_t s)
{
    const RtProgress& P = c->prog;
    const Adapt& ad = *b->adapt;
    const int n_tiles = P.tiles_w() * P.tiles_h();
    hipLaunchKernelGGL(k_adapt_bump, grid_of(n_tiles, threads), dim3(threads), 0, s, (int32_t*)ad.tile_n.p,
                       (int32_t*)ad.tile_nA.p, n_tiles, samples, a_pass ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

int rt_adapt_resolve(rt_context* c, Backend* b, const float4_* base, const float4_* state, float4_* out, bool linear,
                     hipStream_t s)
{
    const RtProgress& P = c->prog;
    const int n = (int)P.npx();
    const int32_t* tn = (const int32_t*)b->adapt->tile_n.p;
    if (linear)
        hipLaunchKernelGGL((k_adapt_resolve<true>), grid_of(n, threads), dim3(threads), 0, s, base, state, tn, out, n, P.w,
                           P.tiles_w());
    else
        hipLaunchKernelGGL((k_adapt_resolve<false>), grid_of(n, threads), dim3(threads), 0, s, base, state, tn, out, n, P.w,
                           P.tiles_w());
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

// rt_backend_progress_noise (rt_noise.hip) for an adaptive progression: the same staged call
// around k_adapt_tiles.
int rt_backend_progress_adapt_noise(rt_context* c, const rtk::NoiseArgs& A, int32_t* stats, float* pixel_err, float* tile_err,
                                    bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    const RtProgress& P = c->prog;
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, b->own)) return r;
    const size_t n = P.npx(), n_tiles = (size_t)P.tiles_w() * P.tiles_h();
    if (int r = st.staging(b->pg_noise, 32 + (pixel_err ? st.pad(4 * n) : 0) + (tile_err ? 4 * n_tiles : 0))) return r;
    uint32_t* d_st = (uint32_t*)st.out(stats, 32);
    float* d_px = (float*)st.out(pixel_err, 4 * n);
    float* d_tl = (float*)st.out(tile_err, 4 * n_tiles);
    if (int r = b->ev_done.wait(c, st.s)) return r;  // (the last pass, its scatter and fold)
    if (device)
        if (int r = b->ev_pg.wait(c, st.s)) return r;
    if (int r = st.begin()) return r;
    if (int r = launch_tiles(c, b, A, d_px, d_tl, d_st, st.s)) return r;
    return st.end(&b->ev_pg);  // (device form: the next pass writes what this reads)
}

// MEASUREMENT HOOK, like rt_device_noise_kernel_ms of rt_noise.hip: exported by the gfx950 library
// only, not part of include/rt_hip.h, never called by the product paths. GPU time of this stage's
// kernels on the context's adaptive progression (tools/adaptive_bench.py): for each of reps
// rounds, each launch runs alone on the default stream between two events. The selection runs
// with samples = 0 (every tile fits and no count moves) at `threshold`, the gather and the scatter
// without the fold over the list that selection left, so the progression is unchanged.
// out_ms[k * reps + r]: k = 0 k_adapt_tiles (tile map only)  1 k_adapt_select  2 k_adapt_gather
// 3 k_adapt_scatter. out_active[2]: the list's tiles and pixels.
extern "C" int rt_device_adapt_kernel_ms(rt_context* c, float threshold, int reps, double* out_ms, int* out_active)
{
    if (!c || !c->prog.active || !c->prog.adaptive || !out_active)
        return rt_fail(c, RT_ERR_ARG, "rt_device_adapt_kernel_ms: bad arguments or no adaptive progression");
    TimedRounds T;
    if (int r = T.enter(c, "rt_device_adapt_kernel_ms", reps, out_ms)) return r;
    Backend* b = rt_backend_dev0(c);
    HIPCHK(c, hipDeviceSynchronize());
    Adapt& ad = *b->adapt;
    int32_t hdr[rtk::AD_WORDS];
    if (int r = rt_adapt_select(c, b, 0, threshold, true, false, hdr, nullptr)) return r;
    const int n_act = hdr[rtk::AD_TILES_ACTIVE], n_px = hdr[rtk::AD_PIXELS];
    out_active[0] = n_act, out_active[1] = n_px;
    if (int r = ensure(c, ad.xy, 8 * (size_t)std::max(n_px, 1))) return r;
    if (int r = ensure(c, ad.idx, 4 * (size_t)std::max(n_px, 1))) return r;
    if (int r = ensure(c, ad.cstate, 16 * (size_t)std::max(n_px, 1))) return r;
    rtk::NoiseArgs F{};
    F.threshold = threshold;
    // (no active tile: the gather and the scatter are timed as an empty interval, not as absent kernels)
    using K = TimedKernel;
    return T.run(0, {K::fixed(0, [&] { return launch_tiles(c, b, F, nullptr, (float*)ad.err.p, nullptr, nullptr); }),
                     K::fixed(1, [&] { return launch_select(c, b, 0, threshold, true, false, nullptr); }),
                     K::fixed(2, [&] { return n_act ? rt_adapt_gather(c, b, n_act, false, nullptr) : RT_OK; }),
                     K::fixed(3, [&] { return n_act ? rt_adapt_scatter(c, b, n_px, false, nullptr) : RT_OK; })});
}
