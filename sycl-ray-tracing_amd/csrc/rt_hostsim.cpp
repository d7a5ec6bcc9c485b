// rt_hostsim.cpp — CPU build of the *product* device code (rt_trace.h),
// linked into librt_hostsim.so for the CPU test suite only.
//
// It lets the container (no GPU) check that the kernel's algorithm — the
// explicit-stack octree walk, the heap-order emulation, the libm
// restatement — reproduces the oracle bit for bit before the same source is
// compiled for gfx950. It is NOT a fallback: the product library
// librt_hip.so has no CPU path and fails loudly without a device.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_adapt.h"
#include "rt_context.h"
#include "rt_denoise.h"
#include "rt_dnv.h"
#include "rt_display.h"
#include "rt_noise.h"
#include "rt_query.h"
#include "rt_gbuffer.h"
#include "rt_temporal.h"
#include "rt_bloom.h"
#include "rt_dof.h"
#include "rt_motion.h"
#include "rt_firefly.h"
#include "rt_upscale.h"
#include "rt_meter.h"
#include "rt_wave.h"

// Stack window and step budget of the host build: smaller than the
// device's so that the CPU tests exercise spilling (dragon rays need up to
// 19 entries) and parking / resuming across iterations all the time.
#ifndef RT_HOSTSIM_SHORT_CAP
#define RT_HOSTSIM_SHORT_CAP 8
#endif
#ifndef RT_HOSTSIM_FAST_CAP
#define RT_HOSTSIM_FAST_CAP 32
#endif
#ifndef RT_HOSTSIM_BUDGET
#define RT_HOSTSIM_BUDGET 24
#endif

int rt_backend_create(rt_context*) { return RT_OK; }
void rt_backend_destroy(rt_context*) {}
int rt_backend_upload(rt_context*) { return RT_OK; }

// adds the per-thread counters into out (callers zero it once per render: a variant sweep sums)
static void merge_stats(unsigned long long* out, const std::vector<rtk::Stats>& s)
{
    for (const auto& t : s)
        for (int i = 0; i < RT_STAT_COUNT; i++) out[i] += t.c[i];
}

// The OpenMP team of one "device" thread of a multi-device render: the caller's thread
// count split over the N devices (each device thread runs its own parallel regions), and
// the caller's own setting restored afterwards (device 0 runs on the caller's thread).
struct OmpShare {
    int all, each;
    explicit OmpShare(int n) : all(omp_get_max_threads()), each(std::max(1, omp_get_max_threads() / std::max(1, n))) {}
    void enter() const { omp_set_num_threads(each); }
    ~OmpShare() { omp_set_num_threads(all); }
};

// The product's wavefront loop (rt_wave_run.hip run_wave) on the host:
// same stage functions, same queues; appends are plain atomics.
template <class E>
static void host_append(const rtk::WaveView& W, int32_t* act_count, int p, const E& e)
{
    for (int k = 0; k < rtk::RK_COUNT; k++)
        if ((e.mask >> k) & 1u) W.q[k][__atomic_fetch_add(&W.counters[k], 1, __ATOMIC_RELAXED)] = e.rec(k, p);
    if (e.active) W.act_out[__atomic_fetch_add(act_count, 1, __ATOMIC_RELAXED)] = p;
}

// prog: a progressive pass (rt_progress_advance): samples first .. spp - 1 of a frame of seed_spp
// samples, every pixel paused into prog (indexed like fb); no tone-map. linear: an ordinary
// render that stops before its tone-map pass (rt_render_linear).
static int run_wave_host(rt_context* c, int w, int h, int spp, int bounces, const rtk::PixSrc& src, int n,
                         float4_* fb, unsigned long long* stats_out, const RtMat* mats = nullptr,
                         float4_* prog = nullptr, int first = 0, int seed_spp = 0, bool linear = false)
{
    if (n <= 0) return RT_OK;
    rtk::WaveView W{};
    W.park_cap = 1 << 14;
    W.spec_cam = c->sched.spec_cam >= 0 ? c->sched.spec_cam : 1;  // (rt_test_schedule; the product's default)
    W.force_fb = c->sched.force_fallback;
    W.spill_lanes = 0;  // the host threads keep their own spill areas
    W.shards = 1;       // one segment per queue (plain atomics on the host)
    W.seg_cap = n;
    std::vector<char> arena(rtk::wave_carve(nullptr, (size_t)n, W));
    rtk::wave_carve(arena.data(), (size_t)n, W);
    W.S = rt_host_view(c);
    if (mats) W.S.mats = mats;  // (rt_render_variants: a variant's table, same size as the bound one)
    W.cam = c->cam;
    W.src = src;
    W.W = w;
    W.H = h;
    W.spp = spp;
    W.bounces = bounces;
    W.prog = prog;
    W.first = prog ? first : 0;
    W.seed_spp = prog ? seed_spp : spp;
    rtk::set_view_consts(W);
    W.n_slots = n;
    W.bl_rays = rt_table_has_emissive_prim(c, W.S.mats) ? 1 : 0;
    W.any_rays = W.S.n_spheres == 0 ? 1 : 0;
    W.fb = fb;
    W.budget = RT_HOSTSIM_BUDGET;
    int32_t counters[rtk::RK_COUNT] = {0};
    int32_t act[2] = {0, 0};
    int32_t parkc[2] = {0, 0}, parka[2] = {0, 0};
    W.counters = counters;
    std::memset(W.r_park, 0, (size_t)n * 4);
    std::memset(W.r_flags, 0, (size_t)n * 4);
    int32_t* lists[2] = {(int32_t*)W.act_in, W.act_out};
    std::vector<rtk::Stats> st(omp_get_max_threads());
    for (auto& s : st) std::memset(&s, 0, sizeof s);

    W.act_out = lists[0];
#pragma omp parallel for schedule(static)
    for (int p = 0; p < n; p++) {
        rtk::Emit e;
        if (W.first > 0) rtk::path_resume(W, p, e);
        else rtk::path_init(W, p, e);
        host_append(W, &act[0], p, e);
    }
    using FAST = rtk::ArrayStack<RT_HOSTSIM_SHORT_CAP>;
    const int last_kind = W.any_rays ? rtk::RK_CAM : rtk::RK_BENV;
    int32_t fbc[2] = {0, 0}, fba[2] = {0, 0};
    for (long it = 0;; it++) {
        const int par = (int)(it & 1);
        // k_trace, exact roles: the walks the last iteration left (parked
        // ones, then its fallback lists); each holds one r_park count of its slot
        const int nrc = std::min(parkc[par], W.park_cap), nra = std::min(parka[par], W.park_cap);
        const int nc = nrc + fbc[par], na = nra + fba[par];
#pragma omp parallel
        {
            std::vector<uint32_t> spr(RT_STACK_CAP);
            std::vector<float> spk(RT_STACK_CAP);
            rtk::SpillStack<FAST> stk{FAST{}, spr.data(), spk.data()};
            rtk::Stats* ps = c->stats_enabled ? &st[omp_get_thread_num()] : nullptr;
#pragma omp for schedule(dynamic, 16)
            for (int idx = 0; idx < nc; idx++) {
                rtk::TravC T;
                uint32_t target;
                bool has;
                if (idx < nrc) {
                    target = rtk::travc_resume(&W.park_c[par][idx], T, stk);
                    has = true;
                } else {
                    const rtk::RayRec r = W.fb_c[par][idx - nrc];
                    target = (rt_asuint(r.o.w) << 3) | rt_asuint(r.d.w);
                    if (ps) ps->c[RT_STAT_FALLBACK]++;
                    has = rtk::travc_begin(W.S, T, rtk::v3of(r.o), rtk::v3of(r.d), ps);
                    if (!has) {
                        rtk::finish_closest(W, target, T.o, T.d, T.best_t, T.best_k);
                        __atomic_fetch_sub(&W.r_park[target >> 3], 1, __ATOMIC_RELAXED);
                    }
                }
                while (has) {
                    if (!rtk::travc_step(W.S, T, stk, ps)) {
                        rtk::finish_closest(W, target, T.o, T.d, T.best_t, T.best_k);
                        __atomic_fetch_sub(&W.r_park[target >> 3], 1, __ATOMIC_RELAXED);
                        break;
                    }
                    if (T.steps >= W.budget && rtk::travc_parkable(T)) {
                        const int slot = __atomic_fetch_add(&parkc[par ^ 1], 1, __ATOMIC_RELAXED);
                        if (slot < W.park_cap) {
                            rtk::travc_park(T, stk, target, &W.park_c[par ^ 1][slot]);
                            break;
                        }
                        T.steps = 0;
                    }
                }
            }
#pragma omp for schedule(dynamic, 16)
            for (int idx = 0; idx < na; idx++) {
                rtk::TravA T;
                uint32_t target;
                bool has;
                if (idx < nra) {
                    target = rtk::trava_resume(&W.park_a[par][idx], T, stk);
                    has = true;
                } else {
                    const rtk::RayRec r = W.fb_a[par][idx - nra];
                    target = (rt_asuint(r.o.w) << 3) | rt_asuint(r.d.w);
                    if (ps) ps->c[RT_STAT_FALLBACK]++;
                    has = rtk::trava_begin(W.S, T, rtk::v3of(r.o), rtk::v3of(r.d), ps);
                    if (!has) {
                        rtk::finish_any(W, target, T.hit);  // (false, or the brute-force answer)
                        __atomic_fetch_sub(&W.r_park[target >> 3], 1, __ATOMIC_RELAXED);
                    }
                }
                while (has) {
                    if (!rtk::trava_step(W.S, T, stk, ps)) {
                        rtk::finish_any(W, target, T.hit);
                        __atomic_fetch_sub(&W.r_park[target >> 3], 1, __ATOMIC_RELAXED);
                        break;
                    }
                    if (T.steps >= W.budget && rtk::trava_parkable(T)) {
                        const int slot = __atomic_fetch_add(&parka[par ^ 1], 1, __ATOMIC_RELAXED);
                        if (slot < W.park_cap) {
                            rtk::trava_park(T, stk, target, &W.park_a[par ^ 1][slot]);
                            break;
                        }
                        T.steps = 0;
                    }
                }
            }
        }
        // k_trace, fast roles: this iteration's queries through the search
        // BVH; failures go to the fallback lists of the next iteration
        int nq = 0;
        for (int k = rtk::RK_CONT; k <= last_kind; k++) nq += counters[k];
        const int nqa = W.any_rays ? counters[rtk::RK_ESH] + counters[rtk::RK_BENV] : 0;
        int32_t* fbc_out = &fbc[par ^ 1];
        int32_t* fba_out = &fba[par ^ 1];
#pragma omp parallel
        {
            rtk::IdxStack<RT_HOSTSIM_FAST_CAP> fst;
            rtk::Stats* ps = c->stats_enabled ? &st[omp_get_thread_num()] : nullptr;
#pragma omp for schedule(dynamic, 64)
            for (int idx = 0; idx < nq; idx++) {
                uint32_t target;
                rtk::RayRec r = rtk::queue_item(W, counters, rtk::RK_CONT, last_kind, idx, target);
                float t;
                int k;
                if (!rtk::forced_fallback(W.force_fb, r.o, r.d) &&
                    rtk::fast_query_closest(W.S, rtk::v3of(r.o), rtk::v3of(r.d), fst, t, k, ps)) {
                    rtk::finish_closest(W, target, rtk::v3of(r.o), rtk::v3of(r.d), t, k);
                } else {
                    r.d.w = rt_asfloat(target & 7u);
                    W.fb_c[par ^ 1][__atomic_fetch_add(fbc_out, 1, __ATOMIC_RELAXED)] = r;
                    __atomic_fetch_add(&W.r_park[target >> 3], 1, __ATOMIC_RELAXED);
                }
            }
#pragma omp for schedule(dynamic, 64)
            for (int idx = 0; idx < nqa; idx++) {
                uint32_t target;
                rtk::RayRec r = rtk::queue_item(W, counters, rtk::RK_ESH, rtk::RK_BENV, idx, target);
                const int a = rtk::forced_fallback(W.force_fb, r.o, r.d) ? -1
                              : rtk::fast_query_any(W.S, rtk::v3of(r.o), rtk::v3of(r.d), fst, ps);
                if (a >= 0) {
                    rtk::finish_any(W, target, a == 1);
                } else {
                    r.d.w = rt_asfloat(target & 7u);
                    W.fb_a[par ^ 1][__atomic_fetch_add(fba_out, 1, __ATOMIC_RELAXED)] = r;
                    __atomic_fetch_add(&W.r_park[target >> 3], 1, __ATOMIC_RELAXED);
                }
            }
        }
        // k_step
        for (int k = 0; k < rtk::RK_COUNT; k++) counters[k] = 0;
        parkc[par] = parka[par] = 0;
        fbc[par] = fba[par] = 0;
        act[par ^ 1] = 0;
        W.act_in = lists[par];
        W.act_out = lists[par ^ 1];
        const int n_in = act[par];
        if (n_in == 0) break;
#pragma omp parallel
        {
            rtk::Stats* ps = c->stats_enabled ? &st[omp_get_thread_num()] : nullptr;
#pragma omp for schedule(dynamic, 64)
            for (int idx = 0; idx < n_in; idx++) {
                const int p = W.act_in[idx];
                // (the step's rays in a column, as k_step keeps them in LDS: rt_wave.h EmitLds)
                float col[6 * rtk::RK_COUNT];
                rtk::EmitLds<1> e;
                e.s = col;
                rtk::path_step<true>(W, p, e, ps);
                host_append(W, &act[par ^ 1], p, e);
            }
        }
    }
    if (!prog && !linear) {
#pragma omp parallel for schedule(static)
        for (int p = 0; p < n; p++) rtk::tonemap_pixel(W, p);
    }
    merge_stats(stats_out, st);
    return RT_OK;
}

// A compacted shard (row j = image row off + j*stride). A multi-device context
// (rt_create_multi) splits it the way the gfx950 backend's render_multi does: row j to
// "device" j mod N, each device's rows packed into a block, rendered as the rows
// off + d*stride + k*N*stride, and un-permuted (here with host copies instead of
// ncclScatter / ncclGather).
static int render_shard(rt_context* c, int w, int h, int spp, int bounces, int off, int stride, int rows,
                        float4_* shard, bool linear)
{
    const int N = c->devices.empty() ? 1 : (int)c->devices.size();
    if (N == 1) {
        rtk::PixSrc src{w, off, stride, nullptr};
        std::fill(c->stats, c->stats + RT_STAT_COUNT, 0ull);
        return run_wave_host(c, w, h, spp, bounces, src, rows * w, shard, c->stats, nullptr, nullptr, 0, 0, linear);
    }
    // one host thread per "device", as render_multi (rt_for_devices: per-device error slots),
    // each with its share of the OpenMP threads (not a full team per device)
    std::vector<std::vector<unsigned long long>> dst(N, std::vector<unsigned long long>(RT_STAT_COUNT, 0));
    const OmpShare share(N);
    const int r = rt_for_devices(c, N, [&](int d) {
        share.enter();
        const int rows_d = rows > d ? (rows - d + N - 1) / N : 0;
        std::vector<float4_> blk((size_t)rows_d * w);
        for (int k = 0; k < rows_d; k++) std::memcpy(&blk[(size_t)k * w], shard + (size_t)(d + k * N) * w, 16 * (size_t)w);
        rtk::PixSrc src{w, off + d * stride, N * stride, nullptr};
        if (int e = run_wave_host(c, w, h, spp, bounces, src, rows_d * w, blk.data(), dst[d].data(), nullptr, nullptr, 0, 0,
                                  linear))
            return e;
        for (int k = 0; k < rows_d; k++) std::memcpy(shard + (size_t)(d + k * N) * w, &blk[(size_t)k * w], 16 * (size_t)w);
        return 0;
    });
    if (r) return r;
    for (int i = 0; i < RT_STAT_COUNT; i++) {
        c->stats[i] = 0;
        for (int d = 0; d < N; d++) c->stats[i] += dst[d][i];
    }
    return RT_OK;
}

int rt_backend_render(rt_context* c, int w, int h, int spp, int bounces, float* host_fb, void* dev_fb, int row_offset,
                      int row_stride, void*, bool linear)
{
    // host_fb: the full frame (rt_render). dev_fb: in this build a host
    // pointer to a compacted row shard, row j = image row row_offset +
    // j*row_stride (rt_render_device semantics, used by the gloo tests).
    const int rows_local = (h - row_offset + row_stride - 1) / row_stride;
    const double t0 = omp_get_wtime();
    int r;
    if (host_fb) {
        // the full frame holds all rows; the wavefront works on the shard's rows
        std::vector<float4_> shard((size_t)rows_local * w);
        for (int j = 0; j < rows_local; j++)
            std::memcpy(&shard[(size_t)j * w], host_fb + 4 * (size_t)(row_offset + j * row_stride) * w, 16 * (size_t)w);
        r = render_shard(c, w, h, spp, bounces, row_offset, row_stride, rows_local, shard.data(), linear);
        for (int j = 0; j < rows_local; j++)
            std::memcpy(host_fb + 4 * (size_t)(row_offset + j * row_stride) * w, &shard[(size_t)j * w], 16 * (size_t)w);
    } else {
        r = render_shard(c, w, h, spp, bounces, row_offset, row_stride, rows_local, (float4_*)dev_fb, linear);
    }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return r;
}

// The material sweep as replicas: variant v on "device" v mod N (one host thread each,
// rt_for_devices), every device walking its variants in order (rt_backend.hip's driver).
int rt_backend_render_variants(rt_context* c, int w, int h, int spp, int bounces, int n_var,
                               const std::vector<RtMat>& tabs, int n_mats, int off, int stride, float* host_fb,
                               void* const* d_fbs)
{
    const int N = c->devices.empty() ? 1 : (int)c->devices.size();
    const int rows = (h - off + stride - 1) / stride;
    const size_t npx = (size_t)rows * w;
    const double t0 = omp_get_wtime();
    std::vector<std::vector<unsigned long long>> dst(N, std::vector<unsigned long long>(RT_STAT_COUNT, 0));
    const OmpShare share(N);
    const int r = rt_for_devices(c, N, [&](int d) {
        share.enter();
        for (int v = d; v < n_var; v += N) {
            // (hostsim: the per-variant mats pointer must cover the context's material indices)
            std::vector<RtMat> tab(tabs.begin() + (size_t)v * n_mats, tabs.begin() + (size_t)(v + 1) * n_mats);
            float4_* fb = host_fb ? (float4_*)(host_fb + 4 * npx * v) : (float4_*)d_fbs[v];  // (host pointers here)
            rtk::PixSrc src{w, off, stride, nullptr};
            if (int e = run_wave_host(c, w, h, spp, bounces, src, (int)npx, fb, dst[d].data(), tab.data())) return e;
        }
        return 0;
    });
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    if (r) return r;
    for (int i = 0; i < RT_STAT_COUNT; i++) {
        c->stats[i] = 0;
        for (int d = 0; d < N; d++) c->stats[i] += dst[d][i];
    }
    return RT_OK;
}

int rt_backend_render_pixels(rt_context* c, int w, int h, int spp, int bounces, const int* xy, int n, float* rgba)
{
    rtk::PixSrc src{w, 0, 1, xy};
    std::fill(c->stats, c->stats + RT_STAT_COUNT, 0ull);
    return run_wave_host(c, w, h, spp, bounces, src, n, (float4_*)rgba, c->stats);
}

// ---- progressions (rt_progress_*): base and state are the context's own vectors here
int rt_backend_progress_begin(rt_context* c, const float* base, const float* state)
{
    RtProgress& P = c->prog;
    const size_t n = P.npx();
    P.base.assign(n, float4_{0.0f, 0.0f, 0.0f, 1.0f});
    P.state.assign(n, float4_{0.0f, 0.0f, 0.0f, 0.0f});
    if (base) std::memcpy(P.base.data(), base, n * sizeof(float4_));
    if (state) std::memcpy(P.state.data(), state, n * sizeof(float4_));
    return RT_OK;
}

int rt_backend_progress_advance(rt_context* c, int first, int stop, void*)
{
    RtProgress& P = c->prog;
    const rtk::PixSrc src{P.w, P.off, P.stride, nullptr};
    std::fill(c->stats, c->stats + RT_STAT_COUNT, 0ull);
    const double t0 = omp_get_wtime();
    const bool fold = P.next_is_a();  // (a tracked progression's A pass: rt_noise.h)
    const long n = (long)P.npx();
    if (fold)
        for (long i = 0; i < n; i++) P.half[i] = rtk::fold_pixel(P.half[i], P.state[i], false);
    const int r = run_wave_host(c, P.w, P.h, stop, P.bounces, src, (int)P.npx(), P.state.data(), c->stats, nullptr,
                                P.state.data(), first, P.total);
    if (fold && !r)
        for (long i = 0; i < n; i++) P.half[i] = rtk::fold_pixel(P.half[i], P.state[i], true);
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return r;
}

int rt_backend_progress_track(rt_context* c, const float* half)
{
    RtProgress& P = c->prog;
    P.half.assign(P.npx(), float4_{0.0f, 0.0f, 0.0f, 0.0f});
    if (half) std::memcpy(P.half.data(), half, P.npx() * sizeof(float4_));
    return RT_OK;
}

int rt_backend_progress_read_half(rt_context* c, float* half)
{
    std::memcpy(half, c->prog.half.data(), c->prog.npx() * sizeof(float4_));
    return RT_OK;
}

// The noise estimate on the host: the loops around rt_noise.h's per-pixel function that
// k_noise_tiles (rt_noise.hip) runs one wave per tile. "Device" pointers are host pointers here; a
// caller's buffers need not be aligned, so words move by memcpy.
static int noise_host(rt_context* c, const rtk::NoiseArgs& F, bool per_tile, int32_t* stats, float* pixel_err, float* tile_err);

int rt_backend_progress_noise(rt_context* c, const rtk::NoiseArgs& A, int32_t* stats, float* pixel_err, float* tile_err,
                              bool, void*)
{
    return noise_host(c, A, false, stats, pixel_err, tile_err);
}

// (an adaptive progression: every tile with its own counts, k_adapt_tiles of rt_adapt.hip)
int rt_backend_progress_adapt_noise(rt_context* c, const rtk::NoiseArgs& A, int32_t* stats, float* pixel_err, float* tile_err,
                                    bool, void*)
{
    return noise_host(c, A, true, stats, pixel_err, tile_err);
}

// F: the frame's arguments; per_tile: n_all, n_a and k from the tile's counts instead. stats may be null.
static int noise_host(rt_context* c, const rtk::NoiseArgs& F, bool per_tile, int32_t* stats, float* pixel_err, float* tile_err)
{
    const RtProgress& P = c->prog;
    const double t0 = omp_get_wtime();
    const int tw = P.tiles_w(), th = P.tiles_h();
    int32_t tiles_over = 0, nonfinite = 0;
    float max_tile = 0.0f;
    for (int ty = 0; ty < th; ty++)
        for (int tx = 0; tx < tw; tx++) {
            const int t = ty * tw + tx;
            const rtk::NoiseArgs A = per_tile ? rtk::adapt_tile_args(P.tile_n[t], P.tile_nA[t], F) : F;
            float v[64];
            for (int l = 0; l < 64; l++) {
                const int x = rtk::NOISE_TILE * tx + (l & 7), y = rtk::NOISE_TILE * ty + (l >> 3);
                v[l] = 0.0f;
                if (x >= P.w || y >= P.rows) continue;
                const size_t i = (size_t)y * P.w + x;
                const float e = rtk::noise_pixel(P.state[i], P.half[i], A);
                if (pixel_err) std::memcpy((char*)pixel_err + 4 * i, &e, 4);
                if (rtk::noise_finite(e)) v[l] = e;
                else nonfinite++;
            }
            const float tile = rtk::noise_tree64(v) / (float)rtk::noise_tile_count(tx, ty, P.w, P.rows);
            if (tile_err) std::memcpy((char*)tile_err + 4 * ((size_t)ty * tw + tx), &tile, 4);
            if (tile > F.threshold) tiles_over++;
            if (rt_asuint(tile) > rt_asuint(max_tile)) max_tile = tile;
        }
    const int32_t st[8] = {tw * th, tiles_over, nonfinite, (int32_t)rt_asuint(max_tile), F.samples_a, F.samples_b, F.passes, 0};
    if (stats) std::memcpy(stats, st, sizeof st);
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// ---- adaptive progressions: the stages of rt_adapt.hip as loops over rt_adapt.h's functions
int rt_backend_progress_adapt_begin(rt_context* c, const int32_t* tile_n, const int32_t* tile_nA)
{
    RtProgress& P = c->prog;
    const size_t n_tiles = (size_t)P.tiles_w() * P.tiles_h();
    P.tile_n.assign(n_tiles, P.done);
    P.tile_nA.assign(n_tiles, P.n_a);
    if (tile_n) std::memcpy(P.tile_n.data(), tile_n, 4 * n_tiles);
    if (tile_nA) std::memcpy(P.tile_nA.data(), tile_nA, 4 * n_tiles);
    return RT_OK;
}

int rt_backend_progress_adapt_bump(rt_context* c, int samples, bool a_pass, void*)
{
    RtProgress& P = c->prog;
    for (size_t t = 0; t < P.tile_n.size(); t++) {
        P.tile_n[t] += samples;
        if (a_pass) P.tile_nA[t] += samples;
    }
    return RT_OK;
}

int rt_backend_progress_adapt_counts(rt_context* c, int32_t* tile_n, int32_t* tile_nA)
{
    const RtProgress& P = c->prog;
    if (tile_n) std::memcpy(tile_n, P.tile_n.data(), 4 * P.tile_n.size());
    if (tile_nA) std::memcpy(tile_nA, P.tile_nA.data(), 4 * P.tile_nA.size());
    return RT_OK;
}

int rt_backend_progress_adapt_advance(rt_context* c, int samples, float threshold, void*, int32_t* hdr)
{
    RtProgress& P = c->prog;
    const double t0 = omp_get_wtime();
    const int tw = P.tiles_w(), th = P.tiles_h(), n_tiles = tw * th;
    const bool estimate = P.passes >= 2, a_pass = P.next_is_a();
    // k_adapt_tiles, then k_adapt_select: flags, the ascending list, the offsets, the counts, the header
    std::vector<float> err(n_tiles, 0.0f);
    if (estimate) {
        rtk::NoiseArgs F{};
        F.threshold = threshold;
        if (int r = noise_host(c, F, true, nullptr, nullptr, err.data())) return r;
    }
    std::vector<int32_t> list, off;
    int n = 0, capped = 0, n_min = 0x7fffffff, n_max = (int)0x80000000;
    for (int t = 0; t < n_tiles; t++) {
        const int flags = rtk::adapt_flags(P.tile_n[t], samples, P.total, estimate, err[t], threshold);
        if (flags & rtk::ADAPT_ACTIVE) {
            list.push_back(t);
            off.push_back(n);
            n += rtk::noise_tile_count(t % tw, t / tw, P.w, P.rows);
            P.tile_n[t] += samples;
            if (a_pass) P.tile_nA[t] += samples;
        }
        if (flags & rtk::ADAPT_CAPPED) capped++;
        n_min = std::min(n_min, P.tile_n[t]);
        n_max = std::max(n_max, P.tile_n[t]);
    }
    const int32_t h[rtk::AD_WORDS] = {(int32_t)list.size(), n, capped, n_min, n_max, n_tiles, 0, 0};
    std::memcpy(hdr, h, sizeof h);
    std::fill(c->stats, c->stats + RT_STAT_COUNT, 0ull);
    if (list.empty()) return RT_OK;
    // k_adapt_gather: lane l of a tile is pixel (8tx + l % 8, 8ty + l / 8); in-frame lanes in lane order
    std::vector<int32_t> xy(2 * (size_t)n), idx(n);
    std::vector<float4_> cstate(n);
    for (size_t a = 0; a < list.size(); a++) {
        const int t = list[a], ty = t / tw, tx = t - ty * tw;
        int slot = off[a];
        for (int l = 0; l < 64; l++) {
            const int x = rtk::NOISE_TILE * tx + (l & 7), y = rtk::NOISE_TILE * ty + (l >> 3);
            if (x >= P.w || y >= P.rows) continue;
            const int p = y * P.w + x;
            xy[2 * (size_t)slot] = x;
            xy[2 * (size_t)slot + 1] = P.off + y * P.stride;
            idx[slot] = p;
            cstate[slot] = P.state[p];
            if (a_pass) P.half[p] = rtk::fold_pixel(P.half[p], P.state[p], false);
            slot++;
        }
    }
    // the pass: samples 1 .. samples of every listed pixel's own chain, paused into cstate (the index is a
    // counter only; before any sample, when every count is 0, from 0: path_init seeds the chains)
    const int first = P.tile_max == 0 ? 0 : 1;
    const rtk::PixSrc src{P.w, 0, 1, xy.data()};
    if (int r = run_wave_host(c, P.w, P.h, first + samples, P.bounces, src, n, cstate.data(), c->stats, nullptr, cstate.data(),
                              first, P.total))
        return r;
    // k_adapt_scatter
    for (int i = 0; i < n; i++) {
        const int p = idx[i];
        P.state[p] = cstate[i];
        if (a_pass) P.half[p] = rtk::fold_pixel(P.half[p], cstate[i], true);
    }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

int rt_backend_progress_resolve(rt_context* c, float* host_fb, void* dev_fb, void*, bool linear)
{
    const RtProgress& P = c->prog;
    float4_* out = host_fb ? (float4_*)host_fb : (float4_*)dev_fb;  // ("device" pointers are host pointers here)
    const long n = (long)P.npx();
    const int tw = P.tiles_w();
    // (an adaptive progression: the pixel's tile count, k_adapt_resolve of rt_adapt.hip)
    auto done_of = [&](long i) { return P.adaptive ? P.tile_n[rtk::adapt_tile_of((int)i, P.w, tw)] : P.done; };
    if (linear) {
#pragma omp parallel for schedule(static)
        for (long i = 0; i < n; i++) out[i] = rtk::resolve_linear_pixel(P.base[i], P.state[i], done_of(i));
        return RT_OK;
    }
#pragma omp parallel for schedule(static)
    for (long i = 0; i < n; i++) out[i] = rtk::resolve_pixel(P.base[i], P.state[i], done_of(i));
    return RT_OK;
}

// The display stage on the host: the loop around rt_display.h's per-pixel functions that
// k_display (rt_display.hip) runs one thread per pixel. "Device" pointers are host pointers in
// this build; a caller's float buffer need not be aligned for float4_, so pixels move by memcpy.
int rt_backend_display(rt_context* c, int w, int h, const void* in, float exposure, float inv_gamma, bool flip,
                       void* out, void* out8, bool, void*)
{
    const double t0 = omp_get_wtime();
#pragma omp parallel for schedule(static)
    for (long i = 0; i < (long)w * h; i++) {
        float4_ px;
        std::memcpy(&px, (const char*)in + 16 * i, 16);
        px = rtk::display_pixel(px, exposure, inv_gamma);
        if (out) std::memcpy((char*)out + 16 * i, &px, 16);
        if (out8) {
            const long y = i / w, x = i - y * w;
            const uint32_t word = rtk::pack_rgba8(px);
            std::memcpy((char*)out8 + 4 * ((flip ? h - 1 - y : y) * w + x), &word, 4);
        }
    }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

int rt_backend_progress_read(rt_context* c, float* base, float* state)
{
    const RtProgress& P = c->prog;
    std::memcpy(base, P.base.data(), P.npx() * sizeof(float4_));
    std::memcpy(state, P.state.data(), P.npx() * sizeof(float4_));
    return RT_OK;
}

void rt_backend_progress_end(rt_context*) {}  // (the vectors go with c->prog)

int rt_backend_intersect(rt_context* c, const float* rays, int n, void* out)
{
    const RtSceneView S = rt_host_view(c);
    std::vector<rtk::Stats> st(omp_get_max_threads());
    for (auto& s : st) std::memset(&s, 0, sizeof s);
#pragma omp parallel
    {
        std::vector<rtk::StackEnt> stack(RT_STACK_CAP);
        rtk::Stats* ps = c->stats_enabled ? &st[omp_get_thread_num()] : nullptr;
#pragma omp for schedule(dynamic, 64)
        for (int i = 0; i < n; i++) {
            const float* r = rays + 6 * (size_t)i;
            const rtk::V3 ro = rtk::v3(r[0], r[1], r[2]), rd = rtk::v3(r[3], r[4], r[5]);
            float t;
            int k;
            rtk::query_closest(S, ro, rd, stack.data(), t, k, ps);
            rtk::Hit h;
            bool f = rtk::hit_from(S, ro, rd, t, k, h);
            int32_t* o = (int32_t*)out + 11 * (size_t)i;
            const float neg1 = -1.0f;
            o[0] = f ? 1 : 0;
            o[1] = h.prim;
            std::memcpy(o + 2, &h.t, 4);
            float pn[6] = {0, 0, 0, 0, 0, 0};
            if (h.t != -1.0f) {
                pn[0] = h.p.x, pn[1] = h.p.y, pn[2] = h.p.z;
                pn[3] = h.n.x, pn[4] = h.n.y, pn[5] = h.n.z;
            }
            std::memcpy(o + 3, pn, 24);
            std::memcpy(o + 9, &neg1, 4);
            std::memcpy(o + 10, &neg1, 4);
        }
    }
    std::fill(c->stats, c->stats + RT_STAT_COUNT, 0ull);
    merge_stats(c->stats, st);
    return RT_OK;
}

// The post stage on the host: the loops around rt_denoise.h's per-pixel functions that the
// gfx950 kernels (rt_denoise.hip) run one thread per pixel. "Device" pointers are host
// pointers in this build.
int rt_backend_features(rt_context* c, int w, int h, void* albedo, void* normal_depth, bool, void*)
{
    const RtSceneView S = rt_host_view(c);
    const rtk::CamView V = rtk::cam_view(c->cam, w, h);
    float4_* alb = (float4_*)albedo;
    float4_* nd = (float4_*)normal_depth;
    const double t0 = omp_get_wtime();
#pragma omp parallel
    {
        std::vector<rtk::StackEnt> stack(RT_STACK_CAP);
#pragma omp for schedule(dynamic, 64)
        for (long i = 0; i < (long)w * h; i++) {
            const int y = (int)(i / w), x = (int)(i - (long)y * w);
            rtk::feature_pixel(S, V, x, y, stack.data(), nd[i], alb[i]);
        }
    }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// One pass of the à-trous filter in mode M: the loop the filter kernels (rt_atrous_hip.h) run one thread per pixel.
template <class M>
static int host_filter_pass(const rtk::DnPass& P, float4_* dst, const float4_* orig, float blend, float* sigma_out)
{
    const rtk::DnDirect F{P};
#pragma omp parallel for schedule(static)
    for (int y = 0; y < P.h; y++)
        for (int x = 0; x < P.w; x++)
            rtk::dn_store(rtk::dn_filter_pixel<M>(P, x, y, F), (size_t)y * P.w + x, dst, orig, blend, sigma_out);
    return RT_OK;
}

int rt_backend_denoise(rt_context* c, int w, int h, const void* in, const void* alb, const void* nd,
                       const rt_denoise_params& p, float blend, void* out, bool, void*)
{
    const size_t n = (size_t)w * h;
    std::vector<float4_> ping(p.passes > 1 ? n : 0), pong(p.passes > 2 ? n : 0);
    const float4_* orig = (const float4_*)in;
    const double t0 = omp_get_wtime();
    rtk::dn_run_passes(w, h, p, orig, {ping.data(), pong.data()}, 0, (float4_*)out, (const float4_*)nd, (const float4_*)alb,
                       [&](const rtk::DnPass& P, float4_* dst, bool last) {
                           return host_filter_pass<rtk::DnFixed>(P, dst, last ? orig : nullptr, blend, nullptr);
                       });
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// The variance-guided filter on the host: k_dnv_prep's loop (rt_dnv.hip), then the passes over its records.
int rt_backend_denoise_var(rt_context* c, int w, int h, const void* in, const void* sigma, const void* alb, const void* nd,
                           const rt_denoise_var_params& p, float blend, void* out, void* sigma_out, bool, void*)
{
    const size_t n = (size_t)w * h;
    std::vector<float4_> rec0(n), rec1(p.passes > 1 ? n : 0);
    const float4_* orig = (const float4_*)in;
    const double t0 = omp_get_wtime();
#pragma omp parallel for schedule(static)
    for (long i = 0; i < (long)n; i++) rec0[i] = rtk::dnv_prep(orig[i], ((const float*)sigma)[i]);
    rtk::dn_run_passes(w, h, p, rec0.data(), {rec0.data(), rec1.data()}, 1, (float4_*)out, (const float4_*)nd,
                       (const float4_*)alb, [&](const rtk::DnPass& P, float4_* dst, bool last) {
                           return host_filter_pass<rtk::DnVar>(P, dst, last ? orig : nullptr, blend,
                                                               last ? (float*)sigma_out : nullptr);
                       });
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// The estimate's numerator per pixel (k_dnv_sigma of rt_dnv.hip): the tile's counts when adaptive.
int rt_backend_progress_noise_sigma(rt_context* c, const rtk::NoiseArgs& F, float* sigma, bool, void*)
{
    const RtProgress& P = c->prog;
    const double t0 = omp_get_wtime();
    const int tw = P.tiles_w();
    for (long i = 0; i < (long)P.npx(); i++) {
        rtk::NoiseArgs A = F;
        if (P.adaptive) {
            const int t = rtk::adapt_tile_of((int)i, P.w, tw);
            A = rtk::adapt_tile_args(P.tile_n[t], P.tile_nA[t], F);
        }
        const float s = rtk::dnv_noise_sigma(P.state[i], P.half[i], A);
        std::memcpy((char*)sigma + 4 * i, &s, 4);
    }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// Temporal accumulation on the host: the loop around rt_temporal.h's temporal_pixel that k_temporal
// (rt_temporal.hip) runs one thread per pixel.
int rt_backend_temporal(rt_context* c, rtk::TemporalFrame T, void* rgba_out, void* sigma_out, void* len_out, bool, void*)
{
    const int w = T.cur.W, h = T.cur.H;
    const double t0 = omp_get_wtime();
#pragma omp parallel for schedule(static)
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            const rtk::TemporalOut r = rtk::temporal_pixel(T, x, y);
            ((float4_*)rgba_out)[p] = r.rgba;
            ((float*)sigma_out)[p] = r.sigma;
            ((float*)len_out)[p] = r.len;
        }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// Firefly rejection on the host: the loop around rt_firefly.h's firefly_pixel that the kernels of
// rt_firefly.hip run one thread per pixel, the neighbours read straight from the frame (FfDirect).
template <int R>
static void firefly_rows(const rtk::FireflyArgs& A, float4_* rgba_out, float* sigma_out, float* scale_out)
{
    const rtk::FfDirect F{A};
#pragma omp parallel for schedule(static)
    for (int y = 0; y < A.h; y++)
        for (int x = 0; x < A.w; x++) {
            const size_t p = (size_t)y * A.w + x;
            const rtk::FireflyOut r = rtk::firefly_pixel<R>(A, x, y, A.in[p], A.sigma ? A.sigma[p] : 0.0f, F);
            rgba_out[p] = r.rgba;
            if (sigma_out) sigma_out[p] = r.sigma;
            if (scale_out) scale_out[p] = r.scale;
        }
}

int rt_backend_firefly(rt_context* c, rtk::FireflyArgs A, void* rgba_out, void* sigma_out, void* scale_out, bool, void*)
{
    const double t0 = omp_get_wtime();
    if (A.radius == 1) firefly_rows<1>(A, (float4_*)rgba_out, (float*)sigma_out, (float*)scale_out);
    else firefly_rows<2>(A, (float4_*)rgba_out, (float*)sigma_out, (float*)scale_out);
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// Bloom on the host: the loops around rt_bloom.h's texel functions that the kernels of rt_bloom.hip run one
// thread per texel, every tap read straight from the level before (bl_reduce_texel over BlFrame / BlLevel).
int rt_backend_bloom(rt_context* c, rtk::BloomArgs A, void* rgba_out, void* layer_out, bool, void*)
{
    const double t0 = omp_get_wtime();
    std::vector<float4_> pyr(rtk::bl_pyramid_texels(A.w, A.h, A.levels));
    struct Lv {
        float4_* g;
        int w, h;
    } L[rtk::BL_MAX_LEVELS + 1];
    L[0] = Lv{nullptr, A.w, A.h};
    float4_* next = pyr.data();
    for (int k = 1; k <= A.levels; k++) {
        L[k] = Lv{next, rtk::bl_half(L[k - 1].w), rtk::bl_half(L[k - 1].h)};
        next += (size_t)L[k].w * L[k].h;
    }
    for (int k = 1; k <= A.levels; k++) {
        const Lv d = L[k];
        const rtk::BlFrame F0{A};
        const rtk::BlLevel Fk{L[k - 1].g, L[k - 1].w, L[k - 1].h};
#pragma omp parallel for schedule(static)
        for (int y = 0; y < d.h; y++)
            for (int x = 0; x < d.w; x++)
                d.g[(size_t)y * d.w + x] = k == 1 ? rtk::bl_reduce_texel(F0, x, y) : rtk::bl_reduce_texel(Fk, x, y);
    }
    for (int k = A.levels - 1; k >= 1; k--) {
        const Lv d = L[k];
        const rtk::BlLevel U{L[k + 1].g, L[k + 1].w, L[k + 1].h};
#pragma omp parallel for schedule(static)
        for (int y = 0; y < d.h; y++)
            for (int x = 0; x < d.w; x++) {
                const size_t p = (size_t)y * d.w + x;
                d.g[p] = rtk::bl_accumulate(d.g[p], U, x, y);
            }
    }
    const rtk::BlLevel U1{L[1].g, L[1].w, L[1].h};
    float4_* out = (float4_*)rgba_out;
    float4_* layer_o = (float4_*)layer_out;
#pragma omp parallel for schedule(static)
    for (int y = 0; y < A.h; y++)
        for (int x = 0; x < A.w; x++) {
            const size_t p = (size_t)y * A.w + x;
            float4_ layer;
            out[p] = rtk::bl_composite(A, A.in[p], U1, x, y, layer);
            if (layer_o) layer_o[p] = layer;
        }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// Depth of field on the host: the loop around rt_dof.h's dof_pixel that k_dof_direct runs one thread per
// pixel, every tap read straight from the frame and its guide record (DofDirect), over the rule's whole window.
int rt_backend_dof(rt_context* c, rtk::DofArgs A, void* rgba_out, void* coc_out, bool, void*)
{
    const double t0 = omp_get_wtime();
    const rtk::DofDirect F{A};
    float4_* out = (float4_*)rgba_out;
    float* coc = (float*)coc_out;
#pragma omp parallel for schedule(static)
    for (int y = 0; y < A.h; y++)
        for (int x = 0; x < A.w; x++) {
            const size_t p = (size_t)y * A.w + x;
            float r;
            out[p] = rtk::dof_pixel(A, x, y, A.in[p], A.nd[p].w, F, &r);
            if (coc) coc[p] = r;
        }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// The motion vectors on the host: the loop around rt_motion.h's mv_pixel that k_motion_vectors runs one thread per pixel.
int rt_backend_motion_vectors(rt_context* c, rtk::MotionVecArgs A, void* motion_out, bool, void*)
{
    const double t0 = omp_get_wtime();
    rtk::MbVec* out = (rtk::MbVec*)motion_out;
    const int w = A.cur.W, h = A.cur.H;
#pragma omp parallel for schedule(static)
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) out[(size_t)y * w + x] = rtk::mv_pixel(A, x, y, A.nd[(size_t)y * w + x]);
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// Motion blur on the host: rule 2 as a raster scan of each tile (a strictly larger l replaces the record, which is the
// key's maximum that k_motion_tilemax reduces), then the loop around mb_neighbour_max and mb_pixel that k_mblur_direct
// runs one thread per pixel, every tap read straight from the frame (MbDirect).
int rt_backend_motion_blur(rt_context* c, rtk::MotionArgs A, void* rgba_out, void* reach_out, bool, void*)
{
    const double t0 = omp_get_wtime();
    const int ntx = rtk::mb_tiles_x(A.w), nty = rtk::mb_tiles_y(A.h);
    std::vector<float4_> tiles((size_t)ntx * nty);
#pragma omp parallel for schedule(static)
    for (int t = 0; t < ntx * nty; t++) {
        const int X0 = (t % ntx) * rtk::MB_TILE, Y0 = (t / ntx) * rtk::MB_TILE;
        float4_ best{0.0f, 0.0f, -1.0f, 0.0f};
        for (int y = Y0; y < Y0 + rtk::MB_TILE && y < A.h; y++)
            for (int x = X0; x < X0 + rtk::MB_TILE && x < A.w; x++) {
                const float4_ r = rtk::mb_reach(A, A.motion[(size_t)y * A.w + x]);
                if (r.z > best.z) best = r;
            }
        tiles[t] = best;
    }
    const rtk::MbDirect F{A};
    float4_* out = (float4_*)rgba_out;
    float* reach = (float*)reach_out;
#pragma omp parallel for schedule(static)
    for (int y = 0; y < A.h; y++)
        for (int x = 0; x < A.w; x++) {
            const size_t p = (size_t)y * A.w + x;
            const float4_ N = rtk::mb_neighbour_max(tiles.data(), ntx, nty, x / rtk::MB_TILE, y / rtk::MB_TILE);
            const float l = rtk::mb_reach(A, A.motion[p]).z;
            out[p] = rtk::mb_pixel(A, x, y, A.in[p], A.nd[p].w, l, N, F);
            if (reach) reach[p] = l;
        }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// The guided upscale on the host: the loop around rt_upscale.h's up_pixel that the kernels of
// rt_upscale.hip run one thread per output pixel, the taps read straight from the low frame (UpDirect).
int rt_backend_upscale(rt_context* c, rtk::UpArgs A, void* rgba_out, void* sigma_out, bool, void*)
{
    const double t0 = omp_get_wtime();
    const rtk::UpDirect F{A};
    float4_* out = (float4_*)rgba_out;
    float* sout = (float*)sigma_out;
#pragma omp parallel for schedule(static)
    for (int y = 0; y < A.h; y++)
        for (int x = 0; x < A.w; x++) {
            const size_t p = (size_t)y * A.w + x;
            const rtk::UpOut r = rtk::up_pixel(A, x, y, A.nd_hi[p], A.alb_hi[p], F);
            out[p] = r.rgba;
            if (sout) sout[p] = r.sigma;
        }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// Exposure metering on the host: the loop around rt_meter.h's meter_pixel that the kernels of
// rt_meter.hip walk grid-stride. Each thread counts its rows into a histogram of its own; the
// histograms are integers, so the merge gives the same words in any order.
int rt_backend_meter(rt_context* c, int w, int h, const void* in, void* hist, bool, void*)
{
    const double t0 = omp_get_wtime();
    uint32_t total[rtk::MT_WORDS] = {};
    total[rtk::MT_MIN_BITS] = 0xffffffffu;
#pragma omp parallel
    {
        uint32_t own[rtk::MT_WORDS] = {};
        own[rtk::MT_MIN_BITS] = 0xffffffffu;
#pragma omp for schedule(static) nowait
        for (long i = 0; i < (long)w * h; i++) {
            float4_ px;
            std::memcpy(&px, (const char*)in + 16 * i, 16);
            rtk::meter_count(own, px);
        }
#pragma omp critical(rt_meter_merge)
        {
            for (int k = 0; k < rtk::MT_WORDS; k++)
                if (k == rtk::MT_MAX_BITS) total[k] = std::max(total[k], own[k]);
                else if (k == rtk::MT_MIN_BITS) total[k] = std::min(total[k], own[k]);
                else total[k] += own[k];
        }
    }
    std::memcpy(hist, total, sizeof(total));
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    return RT_OK;
}

// The ray queries on the host (rt_query.h): the routing of the gfx950 kernels (rt_query.hip)
// with the one-lane search-BVH walks of rt_fast.h in the quads' place; fast_query_closest /
// fast_query_any test far_origin themselves and say when the exact walk must answer.
int rt_backend_query(rt_context* c, bool any, bool all_exact, const void* rays_v, long n, void* out_v, bool, void*)
{
    const RtSceneView S = rt_host_view(c);
    const float* rays = (const float*)rays_v;
    int32_t* out = (int32_t*)out_v;
    long exact = 0;
    const double t0 = omp_get_wtime();
#pragma omp parallel reduction(+ : exact)
    {
        std::vector<rtk::StackEnt> stack(RT_STACK_CAP);
        rtk::IdxStack<RT_HOSTSIM_FAST_CAP> fst;
#pragma omp for schedule(dynamic, 64)
        for (long i = 0; i < n; i++) {
            const float* r = rays + 6 * (size_t)i;
            const rtk::V3 o = rtk::v3(r[0], r[1], r[2]), d = rtk::v3(r[3], r[4], r[5]);
            bool settled = false;
            if (!all_exact) {
                if (any) {
                    const int a = rtk::fast_query_any(S, o, d, fst, nullptr);
                    settled = a >= 0;
                    if (settled) out[i] = a;
                } else {
                    float t;
                    int k;
                    settled = rtk::fast_query_closest(S, o, d, fst, t, k, nullptr);
                    if (settled) rtk::rq_closest_record(S, o, d, t, k, out + RQ_WORDS * (size_t)i);
                }
            }
            if (!settled) {
                rtk::rq_exact(S, rays, (size_t)i, any, stack.data(), out);
                exact++;
            }
        }
    }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    c->query_exact = exact;
    c->query_on_device = false;
    return RT_OK;
}

long rt_backend_query_last_exact(rt_context* c) { return c->query_exact; }

// The first-hit G-buffer on the host (rt_gbuffer.h): gb_pixel per pixel, the routing above with the
// gb_force_every stressor in front of it.
int rt_backend_gbuffer(rt_context* c, int w, int h, bool all_exact, void* albedo, void* normal_depth, void* ids_v, bool,
                       void*)
{
    const RtSceneView S = rt_host_view(c);
    const rtk::CamView V = rtk::cam_view(c->cam, w, h);
    float4_* alb = (float4_*)albedo;
    float4_* nd = (float4_*)normal_depth;
    int32_t* ids = (int32_t*)ids_v;
    const int force = c->sched.gb_force_every;
    long exact = 0;
    const double t0 = omp_get_wtime();
#pragma omp parallel reduction(+ : exact)
    {
        std::vector<rtk::StackEnt> stack(RT_STACK_CAP);
        rtk::IdxStack<RT_HOSTSIM_FAST_CAP> fst;
#pragma omp for schedule(dynamic, 64)
        for (long i = 0; i < (long)w * h; i++) {
            bool ex;
            const rtk::GbRecord r = rtk::gb_pixel(S, V, (int)i, all_exact, force, stack.data(), fst, &ex);
            nd[i] = r.nd;
            alb[i] = r.alb;
            if (ids) ids[2 * i] = r.prim, ids[2 * i + 1] = r.mat;
            exact += ex ? 1 : 0;
        }
    }
    c->last_kernel_ms = (omp_get_wtime() - t0) * 1e3;
    c->gbuffer_exact = exact;
    c->gbuffer_on_device = false;
    return RT_OK;
}

long rt_backend_gbuffer_last_exact(rt_context* c) { return c->gbuffer_exact; }

// The search-BVH closest-hit query the render's k_trace stage runs (rt_fast.h
// fast_query_closest, with its verification), for tests/test_hostsim.py: out_t = the
// answer's t (-1 no hit) or -2 when the exact octree walk must answer; out_k its
// triangle's original index (-1 none). rays[n][6] = origin, direction.
extern "C" int rt_hostsim_fast_queries(rt_context* c, const float* rays, int n, float* out_t, int* out_k)
{
    if (!c || n < 0 || (n > 0 && (!rays || !out_t || !out_k))) return RT_ERR_ARG;
    if (!c->have_bvh) return RT_ERR_STATE;
    const RtSceneView S = rt_host_view(c);
#pragma omp parallel
    {
        rtk::IdxStack<RT_HOSTSIM_FAST_CAP> fst;
#pragma omp for schedule(dynamic, 64)
        for (int i = 0; i < n; i++) {
            const float* r = rays + 6 * (size_t)i;
            float t;
            int k;
            if (rtk::fast_query_closest(S, rtk::v3(r[0], r[1], r[2]), rtk::v3(r[3], r[4], r[5]), fst, t, k, nullptr)) {
                out_t[i] = t;
                out_k[i] = k < 0 ? -1 : (int)rt_asuint(S.tri4[3 * (size_t)k].w);
            } else {
                out_t[i] = -2.0f;
                out_k[i] = -2;
            }
        }
    }
    return RT_OK;
}

// What the leaf visits of a ray's occlusion walk meet (tests/test_trace_fixed_cost.py selects its
// rays by these): the whole search BVH under the ray's boxes is walked, no early exit, and every
// leaf (a pack of up to four triangles, one per lane of a quad) is classified by the lanes whose
// Moller-Trumbore test hits and by their octree leaves. out[n][4]:
//   [0] the most hit lanes in one pack
//   [1] packs with two or more hit lanes in one octree leaf
//   [2] packs whose hit lanes lie in different octree leaves
//   [3] of those, packs where the first hit lane's leaf fails its chain check (a second check runs)
extern "C" int rt_hostsim_leaf_hits(rt_context* c, const float* rays, int n, int* out)
{
    if (!c || n < 0 || (n > 0 && (!rays || !out))) return RT_ERR_ARG;
    if (!c->have_bvh) return RT_ERR_STATE;
    const RtSceneView S = rt_host_view(c);
#pragma omp parallel
    {
        std::vector<int> stack;
#pragma omp for schedule(dynamic, 64)
        for (int i = 0; i < n; i++) {
            const float* r = rays + 6 * (size_t)i;
            const rtk::V3 o = rtk::v3(r[0], r[1], r[2]), d = rtk::v3(r[3], r[4], r[5]);
            int* w = out + 4 * (size_t)i;
            w[0] = w[1] = w[2] = w[3] = 0;
            if (rt_isnan(o.x) || rt_isnan(o.y) || rt_isnan(o.z) || rt_isnan(d.x) || rt_isnan(d.y) || rt_isnan(d.z)) continue;
            const rtk::RayB rb = rtk::rayb_setup(o, d);
            rtk::RayK K;
            rtk::ray_setup(o, d, K);
            stack.assign(1, 0);
            while (!stack.empty()) {
                const int cur = stack.back();
                stack.pop_back();
                rtk::ItemRecs R;
                rtk::load_item(S, cur, R);
                if (cur >= 0) {
                    const rtk::Bvh4R nd = rtk::node_of(R);
                    float tn[4];
                    bool hit[4];
                    rtk::box4(S, cur, nd, rb, o, d, __builtin_inff(), tn, hit);
                    for (int ch = 0; ch < 4; ch++)
                        if (hit[ch]) stack.push_back(nd.cnt[ch] > 0 ? rtk::leaf_item(nd.ref[ch], nd.cnt[ch]) : nd.ref[ch]);
                    continue;
                }
                const int cnt = ((~cur) & 3) + 1;
                int leaves[4], nh = 0;
                for (int j = 0; j < cnt; j++) {
                    float t;
                    if (rtk::tri_test_v(rtk::ld3(R.q[3 * j]), rtk::ld3(R.q[3 * j + 1]), rtk::ld3(R.q[3 * j + 2]), o, d, t))
                        leaves[nh++] = (int)rt_asuint(R.q[3 * j + 1].w);
                }
                if (nh > w[0]) w[0] = nh;
                bool same = false, other = false;
                for (int a = 0; a < nh; a++)
                    for (int b = a + 1; b < nh; b++) (leaves[a] == leaves[b] ? same : other) = true;
                if (same) w[1]++;
                if (other) {
                    w[2]++;
                    if (!rtk::chain_ok(S, K, leaves[0], false, 0.0f, nullptr)) w[3]++;
                }
            }
        }
    }
    return RT_OK;
}

// TEST ONLY (include/rt_hip.h): the env-CDF search alone, as the host build runs it (there is no
// LDS copy here: forms 0 and 1 read the same tables through cdf_search and cdf_search_global).
extern "C" int rt_device_env_search(rt_context* c, int form, const float* values, int n, int* xy_out)
{
    if (!c || n <= 0 || !values || !xy_out || form < 0 || form > 1) return RT_ERR_ARG;
    if (!c->have_env) return RT_ERR_STATE;
    const RtSceneView S = rt_host_view(c);
    for (int i = 0; i < n; i++) {
        if (form == 0)
            rtk::cdf_search(S, values[i], xy_out[2 * i], xy_out[2 * i + 1], nullptr);
        else
            rtk::cdf_search_global(S, values[i], xy_out[2 * i], xy_out[2 * i + 1]);
    }
    return RT_OK;
}

// Heap-order emulation self-check against std::priority_queue (exported for
// tests/test_hostsim.py): keys[m] in push order -> order[m] of pushed indices.
#include <queue>
extern "C" int rt_hostsim_heap_order(const float* keys, int m, int* order_emul, int* order_std)
{
    if (m < 1 || m > 8) return -1;
    float k[8], ok[8];
    int id[8], oi[8];
    for (int i = 0; i < m; i++) k[i] = keys[i], id[i] = i;
    rtk::heap_order(k, id, m, ok, oi);
    for (int i = 0; i < m; i++) order_emul[i] = oi[i];
    struct QE {
        int id;
        float t;
        bool operator>(const QE& o) const { return t > o.t; }
    };
    std::priority_queue<QE, std::vector<QE>, std::greater<QE>> q;
    for (int i = 0; i < m; i++) q.emplace(QE{i, keys[i]});
    for (int i = 0; i < m; i++) {
        order_std[i] = q.top().id;
        q.pop();
    }
    return 0;
}

#ifndef RT_BUILD_SRC
#define RT_BUILD_SRC "unknown"
#endif
#ifndef RT_BUILD_DEFS
#define RT_BUILD_DEFS ""
#endif
extern "C" const char* rt_build_id(void) { return "src=" RT_BUILD_SRC " defs=" RT_BUILD_DEFS " (hostsim)"; }

// What a ray's closest-hit search-BVH walk meets, trip by trip (tests/test_trip_code.py checks with it that
// its inputs produce the cases they are for): rt_fast.h fast_closest_u with counters, over a stack of
// RT_HOSTSIM_FAST_CAP entries (32: the quads' RT_HOSTSIM_FAST_CAP). One trip = one item, as a quad takes them. out[n][10]:
//   [0..4] inner trips with 0, 1, 2, 3, 4 children hit (4 hit: 3 pushed)
//   [5]    inner trips where two hit children have equal keys (the tie rule decides the push order)
//   [6]    the deepest stack (entries) the walk reached; with [8] set, the depth at the overflow
//   [7]    pops that found the stack empty (the walk's end included)
//   [8]    1 when the bounded stack overflowed (the walk stops: the exact walk answers)
//   [9]    leaf visits
extern "C" int rt_hostsim_trip_cases(rt_context* c, const float* rays, int n, int* out)
{
    if (!c || n < 0 || (n > 0 && (!rays || !out))) return RT_ERR_ARG;
    if (!c->have_bvh) return RT_ERR_STATE;
    const RtSceneView S = rt_host_view(c);
#pragma omp parallel
    {
        rtk::IdxStack<RT_HOSTSIM_FAST_CAP> stk;
#pragma omp for schedule(dynamic, 64)
        for (int i = 0; i < n; i++) {
            const float* r = rays + 6 * (size_t)i;
            const rtk::V3 o = rtk::v3(r[0], r[1], r[2]), d = rtk::v3(r[3], r[4], r[5]);
            int* w = out + 10 * (size_t)i;
            for (int j = 0; j < 10; j++) w[j] = 0;
            if (rt_isnan(o.x) || rt_isnan(o.y) || rt_isnan(o.z) || rt_isnan(d.x) || rt_isnan(d.y) || rt_isnan(d.z)) continue;
            rtk::FastHit h;
            h.t = h.t2 = __builtin_inff();
            h.k = -1, h.leaf = -1, h.prim = 0x7fffffff, h.tie = false, h.ovf = false;
            const rtk::RayB rb = rtk::rayb_setup(o, d);
            int sp = 0, cur = 0;
            for (;;) {
                rtk::ItemRecs R;
                rtk::load_item(S, cur, R);
                if (cur >= 0) {
                    const rtk::Bvh4R nd = rtk::node_of(R);
                    float tn[4], kk[4];
                    bool hit[4];
                    int v[4], ix[4] = {0, 1, 2, 3}, nv = 0;
                    const float tmax = h.t + h.t * RT_T2_WINDOW;
                    rtk::box4(S, cur, nd, rb, o, d, tmax, tn, hit);
                    for (int ch = 0; ch < 4; ch++) {
                        const bool ok = hit[ch] && tn[ch] <= tmax;
                        kk[ch] = ok ? tn[ch] : __builtin_inff();
                        v[ch] = nd.cnt[ch] > 0 ? rtk::leaf_item(nd.ref[ch], nd.cnt[ch]) : nd.ref[ch];
                        nv += ok ? 1 : 0;
                    }
                    rtk::sort4(kk, ix);
                    w[nv]++;
                    for (int j = 1; j < nv; j++)
                        if (kk[j] == kk[j - 1]) {
                            w[5]++;
                            break;
                        }
                    if (sp + nv - 1 > RT_HOSTSIM_FAST_CAP) {
                        w[6] = sp + nv - 1;
                        w[8] = 1;
                        break;
                    }
                    for (int j = nv - 1; j >= 1; j--) stk.set(sp++, (uint32_t)v[ix[j]], kk[j]);
                    if (sp > w[6]) w[6] = sp;
                    if (nv > 0) {
                        cur = v[ix[0]];
                        continue;
                    }
                } else {
                    const int cnt = ((~cur) & 3) + 1;
                    w[9]++;
                    for (int j = 0; j < cnt; j++) {
                        float t;
                        if (rtk::tri_test_v(rtk::ld3(R.q[3 * j]), rtk::ld3(R.q[3 * j + 1]), rtk::ld3(R.q[3 * j + 2]), o, d, t))
                            rtk::fast_take(h, t, (int)rt_asuint(R.q[3 * j].w), (int)rt_asuint(R.q[3 * j + 1].w),
                                           (int)rt_asuint(R.q[3 * j + 2].w), S.brute != 0);
                    }
                }
                const float tmax = h.t + h.t * RT_T2_WINDOW;
                cur = 0x7fffffff;
                while (sp > 0) {
                    --sp;
                    if (stk.key(sp) <= tmax) {
                        cur = (int)stk.rec(sp);
                        break;
                    }
                }
                if (cur == 0x7fffffff) {
                    w[7]++;
                    break;
                }
            }
        }
    }
    return RT_OK;
}
