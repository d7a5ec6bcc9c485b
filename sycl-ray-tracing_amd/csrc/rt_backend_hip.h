// rt_backend_hip.h — what the translation units of the gfx950 backend share: the HIP error
// check, the owners of device resources (freed by their destructors), the recorded-event
// Marker, the per-device Backend (every unit reaches the root's through rt_backend_dev0), the
// StagedCall that runs a stage in its host or its device form, and the hooks between the units:
//   rt_backend.hip  contexts, uploads, the multi-device / variant / pixel-list drivers
//   rt_render.hip   the render kernels and their launch helpers (rt_wave_kernels.h)
//   rt_wave_run.hip the wavefront loop (run_wave) over them; rt_wave_layout.h: the counters both index
//   rt_probe.hip    rt_intersect's kernel and the test / measurement kernels no render launches
//   rt_denoise.hip  the post stage          rt_query.hip  the ray queries
//   rt_display.hip  the display stage and the linear resolve
//   rt_noise.hip    a tracked progression's fold and noise estimate
//   rt_dnv.hip      the variance-guided post stage and the absolute noise figure it takes
//   rt_temporal.hip temporal accumulation: the previous frame reprojected and blended in
//   rt_firefly.hip  firefly rejection: a pixel's luminance limited by a rank of its neighbours'
//   rt_upscale.hip  guided upscale: a low-resolution frame taken to the output size along the full-size guides
//   rt_meter.hip    exposure metering: the luminance histogram of a linear frame
//   rt_gbuffer.hip  the first-hit G-buffer on the render's walks (quads in front, octets behind)
//   rt_bloom.hip    bloom: the energy above a threshold spread by a Gaussian pyramid and added back
//   rt_dof.hip      depth of field: a gather over each pixel's circle of confusion, from the first-hit distance
//   rt_motion.hip   motion vectors from the guides and the previous camera; motion blur: a gather along each tile's line
#pragma once

#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "rt_context.h"
#include "rt_plan.h"

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return rt_fail(ctx, RT_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_));     \
    } while (0)

#define RT_MAX_TIMED_ITERS 16384

// A HIP handle released by its destructor (the owner's device is current: destroy_one).
template <class T, class A, hipError_t (*FREE)(A)>
struct Owned {
    T h{};
    Owned() = default;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = T{}; }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned()
    {
        if (h) (void)FREE(h);
    }
    operator T() const { return h; }
};
using Event = Owned<hipEvent_t, hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStream_t, hipStreamDestroy>;
template <class T>
using Pinned = Owned<T*, void*, hipHostFree>;

// A device allocation, grown on demand (ensure) and freed with its owner.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
};

inline int ensure(rt_context* c, DevBuf& b, size_t bytes)
{
    if (b.bytes >= bytes && b.p) return RT_OK;
    if (b.p) HIPCHK(c, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    if (bytes == 0) return RT_OK;
    HIPCHK(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return RT_OK;
}

template <class T>
int upload(rt_context* c, DevBuf& b, const std::vector<T>& v)
{
    const size_t bytes = v.size() * sizeof(T);
    if (int r = ensure(c, b, bytes > 0 ? bytes : 16)) return r;
    if (bytes) HIPCHK(c, hipMemcpy(b.p, v.data(), bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

// A device made current for the call; the caller's device restored afterwards.
struct DeviceScope {
    int prev = -1;
    int enter(rt_context* c, int device)
    {
        int cur = -1;
        HIPCHK(c, hipGetDevice(&cur));
        if (cur != device) {
            HIPCHK(c, hipSetDevice(device));
            if (prev < 0) prev = cur;
        }
        return RT_OK;
    }
    ~DeviceScope()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// An event and whether it has been recorded: waiting for one never recorded is a no-op.
struct Marker {
    Event ev;
    bool recorded = false;
    int record(rt_context* c, hipStream_t s)
    {
        HIPCHK(c, hipEventRecord(ev, s));
        recorded = true;
        return RT_OK;
    }
    int wait(rt_context* c, hipStream_t s) const  // s waits for it
    {
        if (recorded) HIPCHK(c, hipStreamWaitEvent(s, ev, 0));
        return RT_OK;
    }
    int sync(rt_context* c) const  // the host waits for it
    {
        if (recorded) HIPCHK(c, hipEventSynchronize(ev));
        return RT_OK;
    }
};

// The ray queries' workspace (rt_query.hip), created on first use and deleted with its Backend
// (its device current).
struct Query;
struct QueryDelete {
    void operator()(Query* q) const;
};

// The G-buffer stage's workspace (rt_gbuffer.hip), owned the same way.
struct Gbuf;
struct GbufDelete {
    void operator()(Gbuf* g) const;
};

namespace rtk {
struct WaveView;
struct PixSrc;
}

// The buffers of an à-trous stage on the root device (rt_atrous_hip.h: rt_denoise's and rt_denoise_var's,
// one each), created on first use and cached across calls like the render's.
struct Post {
    DevBuf io;  // host-pointer calls: the stage's inputs and outputs
    DevBuf pp;  // the two buffers the passes alternate between
    // optional timing (dn_pass_ms): an event before each launch (rt_denoise_var's prep, each pass) and after the last
    bool timing = false;
    Event pev[12];
    int timed_passes = 0;
};

// An adaptive progression's buffers (rt_adapt.hip), created by its first adaptive pass or a
// version-3 load and dropped with the progression.
struct Adapt {
    DevBuf tile_n, tile_nA;  // int32 per tile: samples done, and those of them in A passes
    DevBuf err;              // float per tile: the selection's tile errors
    DevBuf list, off;        // per active tile, ascending: its index; its first slot in the pixel list
    DevBuf hdr;              // the selection's header (rtk::AD_WORDS int32)
    DevBuf xy, idx, cstate;  // per slot: (x, image y); pixel index in the shard; the compact paused state
    Pinned<int32_t> h_hdr;   // the header's readback
};

// One device's resources. Created and destroyed with its device current (rt_backend.hip).
struct Backend {
    int device = 0;
    int index = 0;    // position in the context's device list (0: the root)
    Stream own;       // device-side work not on a caller's stream (multi-device shards, pixel lists)
    DevBuf tables[RT_SCENE_TABLES];  // the uploads of rt_scene_tables' vectors, in its order
    DevBuf tri4, mats, matk;         // the patched triangle records, the material table, leaf-order k -> material
    DevBuf stats;     // 2 x RT_STAT_COUNT u64: all kernels, then the tail kernel's share
    DevBuf handovers; // u64: queries k_trace handed to the exact walk, every render since the last reset
    DevBuf iterq;     // stats renders: per-iteration {queries, live slots} (RT_ITER_LOG)
    DevBuf wlog;      // stats renders with a walk log: count (256 B), then 3 float4 per record
    DevBuf wave[RT_MAX_LANES];      // per lane: path state, pending records, results, queues, lists
    DevBuf counters[RT_MAX_LANES];  // per lane: the wavefront counters (rt_wave_counter_bytes)
    // fast lane (rt_test_schedule fast_k): per lane its handed-over list + ticket, counters,
    // samples-done histogram and spill area; the lanes' views for the one tail kernel over them
    DevBuf fast[RT_MAX_LANES], fcnt[RT_MAX_LANES], fhist[RT_MAX_LANES], fspill[RT_MAX_LANES], fviews;
    Pinned<int32_t> h_hist[RT_MAX_LANES];
    Pinned<rtk::WaveView> h_fviews;
    Event fev[RT_MAX_LANES];
    Marker fev_done;          // end of the last fast-lane kernel: it read the views the next one overwrites
    Event hev[RT_MAX_LANES];  // fast lane: each lane's samples-done histogram readback
    Event ftev[2];  // (timed renders: around the fast lane's kernel)
    Stream fs;      // the fast lane's stream with 4 lanes (fewer: the first idle lane stream)
    DevBuf xy;        // pixel list (rt_render_pixels)
    DevBuf fb;        // host-fb staging
    DevBuf pg_base, pg_state, pg_out;  // a progression (rt_progress_*): base values, paused state, host-resolve staging
    DevBuf pg_half, pg_noise;          // a tracked one: the A passes' sum; the host noise query's stat words and maps
    DevBuf disp;      // rt_display with host pointers: the frame (in, float out in place), then the 8-bit output
    // the other stages' host-pointer calls, each its own staging buffer, grown on first use and kept across calls:
    DevBuf temporal_io;  // rt_temporal_accumulate: the three inputs of this frame, the four of the history, the three outputs
    DevBuf firefly_io;   // rt_firefly: the frame and its sigma, then the three outputs
    DevBuf meter_io;     // rt_meter: the frame, then the histogram
    DevBuf upscale_io;   // rt_upscale: the low frame, its sigma and guides, the full-size guides, then the two outputs
    DevBuf bloom;        // rt_bloom: the pyramid (levels 1.. back to back); host form: the frame and the two outputs, then the pyramid
    DevBuf dof_io;       // rt_dof: the frame and its guide record, then the two outputs
    DevBuf motion_io;    // rt_motion_vectors: the guides, then the vectors; rt_motion_blur: the frame, its guide record and motion, then the two outputs
    DevBuf motion_tiles; // rt_motion_blur: one record {hx, hy, l, 0} per 16 x 16 motion tile, host and device form
    int cus = 0;         // the device's compute units, asked by the first rt_meter (rt_meter.hip; 0: not yet)
    DevBuf shard;     // multi-device renders: the root's N blocks of rows_max rows (scatter source /
                      // gather target); device d >= 1: its block
    Pinned<int32_t> h_act[RT_MAX_LANES];  // per lane: live-slot counters (sharded) + 8 fallback counters
    Event ev0, ev1;
    Marker ev_pg;    // end of the last device resolve or noise query: the next pass writes the state it reads
    Marker ev_done;  // end of the last run_wave (all lanes joined): the next render waits for it
    Stream ls[RT_MAX_LANES];                // lanes 1.. streams (lane 0 runs on the caller's)
    Event ev_fork, ev_join[RT_MAX_LANES], ev_lane[RT_MAX_LANES];
    int lanes = 0;                          // RT_LANES; 0: auto, 4 lanes for launches of at most RT_LANES4_MAX
                                            // slots, else 3 (cfg2 1-4 lanes: 452 / 499 / 519 / 509 Msamples/s, r01;
                                            // r03: 3 / 4 lanes cfg2 147.5 / 148.6 ms, cfg4 8-way shard 398 / 386 ms,
                                            // 6 / 8 lanes 230-710 ms: more streams than the 4 hardware queues)
    RtSceneView view{};
    int bl_rays = 1, any_rays = 1;
    int last_iters = 0;
    int tail_iter = -1;     // iteration whose step launch was the tail kernel (-1: none)
    int budget = 1024;  // steps per query per launch before it parks (RT_STEP_BUDGET)
    // optional per-kernel timing: events around each launch of each class
    bool timing = false;
    Event tev[RT_MAX_LANES][3][RT_MAX_TIMED_ITERS];
    double kms[3] = {0, 0, 0};      // k_trace, k_step, k_tail
    long klaunch[3] = {0, 0, 0};
    std::unique_ptr<Post> post, post_var;       // (rt_denoise.hip, rt_dnv.hip)
    std::unique_ptr<Query, QueryDelete> query;  // (rt_query.hip)
    std::unique_ptr<Adapt> adapt;               // (rt_adapt.hip)
    std::unique_ptr<Gbuf, GbufDelete> gbuf;     // (rt_gbuffer.hip)
};

Backend* rt_backend_dev0(rt_context* c);  // rt_backend.hip: the root device's Backend

// One call of a stage, in its device form (the caller's device buffers on the caller's stream,
// no wait; rt_last_kernel_ms is -1 until rt_device_last_kernel_ms reads ev0 / ev1 once the caller
// has synchronized) or its host form (host buffers through regions of the stage's staging
// DevBuf, each at a 16-byte boundary; waits; rt_last_kernel_ms is the time between ev0 and ev1):
//   enter, [staging], in / out / inout per buffer, begin, the stage's launches, end
// b's device is current until the StagedCall leaves scope, then the caller's again.
// The host forms' streams are inherited from the stages as they were written, not chosen here:
//   null stream   features, denoise and denoise_var (a Post::io each), temporal_accumulate
//                 (temporal_io), firefly (firefly_io), meter (meter_io), upscale (upscale_io), bloom (bloom), dof (dof_io),
//                 motion_vectors and motion_blur (motion_io),
//                 display (disp), queries (Query::io), rt_render (fb)
//   Backend::own  noise and noise_sigma (pg_noise), progressive resolves (pg_out), pixel lists (fb)
struct StagedCall {
    rt_context* c = nullptr;
    Backend* b = nullptr;
    bool device = false;
    hipStream_t s = nullptr;
    DeviceScope sc;
    char* base = nullptr;  // host form: the staging buffer, what it holds and what is taken
    size_t cap = 0, used = 0;
    struct Out {
        void* host;
        const void* dev;
        size_t bytes;
    } outs[4];
    int n_out = 0;
    int err = RT_OK;  // the first failure of a region; begin returns it

    static size_t pad(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
    int enter(rt_context* ctx, Backend* be, bool device_form, void* caller_stream, hipStream_t host_stream)
    {
        c = ctx, b = be, device = device_form;
        s = device ? (hipStream_t)caller_stream : host_stream;
        return sc.enter(c, b->device);
    }
    // host form: the regions come from d, grown to `bytes` (the padded sizes of all of them)
    int staging(DevBuf& d, size_t bytes)
    {
        if (device) return RT_OK;
        if (int r = ensure(c, d, bytes)) return r;
        base = (char*)d.p, cap = d.bytes, used = 0;
        return RT_OK;
    }
    // A buffer of the call. Device form: the caller's pointer (src, or dst for an output). Host
    // form: the next region, filled from src now and copied to dst by end; neither: no region.
    void* inout(const void* src, void* dst, size_t bytes)
    {
        if (device) return src ? (void*)src : dst;
        if ((!src && !dst) || err) return nullptr;
        if (used + bytes > cap || (dst && n_out == 4)) {
            err = rt_fail(c, RT_ERR_ARG, "StagedCall: a region beyond the staging buffer");
            return nullptr;
        }
        void* p = base + used;
        used += pad(bytes);
        if (src) {
            const hipError_t e = hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) err = rt_fail(c, RT_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
        }
        if (dst) outs[n_out++] = Out{dst, p, bytes};
        return p;
    }
    void* in(const void* src, size_t bytes) { return inout(src, nullptr, bytes); }
    void* out(void* dst, size_t bytes) { return inout(nullptr, dst, bytes); }
    int begin()
    {
        if (err) return err;
        HIPCHK(c, hipEventRecord(b->ev0, s));
        return RT_OK;
    }
    int stop()
    {
        HIPCHK(c, hipEventRecord(b->ev1, s));
        return RT_OK;
    }
    // mark: recorded in the device form (the call's end, for whoever overwrites what it read).
    // ms_out: the host form's time goes there instead of the context (one device's thread of many).
    int finish(Marker* mark = nullptr, float* ms_out = nullptr)
    {
        if (device) {
            if (mark)
                if (int r = mark->record(c, s)) return r;
            c->last_kernel_ms = -1.0;
            return RT_OK;
        }
        for (int i = 0; i < n_out; i++)
            HIPCHK(c, hipMemcpyAsync(outs[i].host, outs[i].dev, outs[i].bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, b->ev0, b->ev1));
        if (ms_out) *ms_out = ms;
        else c->last_kernel_ms = ms;
        return RT_OK;
    }
    int end(Marker* mark = nullptr, float* ms_out = nullptr)
    {
        if (int r = stop()) return r;
        return finish(mark, ms_out);
    }
};

// The measurement hooks' loop body (TimedRounds below): one
// launch alone on the default stream between e0 and e1, waited for; its GPU time into *ms.
template <class F>
int rt_time_alone(rt_context* c, hipEvent_t e0, hipEvent_t e1, F launch, double* ms)
{
    HIPCHK(c, hipEventRecord(e0, nullptr));
    const int rc = launch();
    HIPCHK(c, hipEventRecord(e1, nullptr));
    if (rc) return rc;
    HIPCHK(c, hipEventSynchronize(e1));
    float f = 0;
    HIPCHK(c, hipEventElapsedTime(&f, e0, e1));
    *ms = f;
    return RT_OK;
}

// The rounds of a measurement hook (rt_device_*_kernel_ms): reps rounds in which each kernel of a list runs alone
// (rt_time_alone), its time stored at out_ms[slot * reps + r].
//   enter  the reps / out_ms check, the root device made current, the two events
//   run    the default stream synchronised (the hook's validating product call has ended), then the rounds
// The kernels run in the list's order, but for the rotated ones: round r starts them at the (r + first)-th of them, so
// that none always runs behind another; the others keep their place around them.
struct TimedKernel {
    int slot;
    std::function<int()> launch;  // none: the kernel is absent and its slots hold 0
    bool rotated;
    std::function<int()> before;  // optional: runs in front of the first event (not timed)
    static TimedKernel fixed(int slot, std::function<int()> launch, std::function<int()> before = nullptr)
    {
        return {slot, std::move(launch), false, std::move(before)};
    }
    static TimedKernel turns(int slot, std::function<int()> launch) { return {slot, std::move(launch), true, nullptr}; }
    static TimedKernel absent(int slot) { return {slot, nullptr, false, nullptr}; }
};
struct TimedRounds {
    rt_context* c = nullptr;
    int reps = 0;
    double* out_ms = nullptr;
    DeviceScope sc;
    Event e0, e1;
    int enter(rt_context* ctx, const char* hook, int n_reps, double* out)
    {
        if (!ctx || !ctx->backend || n_reps <= 0 || !out) return rt_fail(ctx, RT_ERR_ARG, std::string(hook) + ": bad arguments");
        c = ctx, reps = n_reps, out_ms = out;
        if (int r = sc.enter(c, rt_backend_dev0(c)->device)) return r;
        HIPCHK(c, hipEventCreate(&e0.h));
        HIPCHK(c, hipEventCreate(&e1.h));
        return RT_OK;
    }
    int run(int first, const std::vector<TimedKernel>& kernels)
    {
        HIPCHK(c, hipStreamSynchronize(nullptr));
        std::vector<int> rot;  // the rotated kernels' places in the list
        for (size_t i = 0; i < kernels.size(); i++)
            if (kernels[i].rotated) rot.push_back((int)i);
        const int n_rot = (int)rot.size();
        for (int r = 0; r < reps; r++) {
            int turn = n_rot ? ((r + first) % n_rot + n_rot) % n_rot : 0;
            for (const TimedKernel& at : kernels) {
                const TimedKernel& k = at.rotated ? kernels[rot[turn++ % n_rot]] : at;
                double& ms = out_ms[(size_t)k.slot * reps + r];
                ms = 0.0;
                if (!k.launch) continue;
                if (k.before)
                    if (int e = k.before()) return e;
                if (int e = rt_time_alone(c, e0, e1, k.launch, &ms)) return e;
            }
        }
        return RT_OK;
    }
};

// rt_wave_run.hip: the wavefront loop for n slots of `src` into fb (device, n float4) on b's
// device (current), and the sizes of a lane's counters and of its pinned readback block.
// A progressive pass (rt_progress_advance): samples first .. spp - 1 of every pixel of a frame
// of seed_spp samples, each pixel paused into state (n float4, indexed like fb; fb unused).
struct WavePass {
    float4_* state;
    int first, seed_spp;
};
// linear: an ordinary render whose k_tonemap launch is skipped (rt_render_linear): fb keeps
// entry + final_color / spp.
int run_wave(rt_context* c, Backend* b, int w, int h, int spp, int bounces, const rtk::PixSrc& src, int n, float4_* fb,
             hipStream_t s, const WavePass* pass = nullptr, bool linear = false);
// rt_wave_run.hip (rt_render.hip k_resolve): out[i] = the tone-mapped pixel of base[i] and state[i] after `done` samples
int rt_wave_resolve(rt_context* c, const float4_* base, const float4_* state, float4_* out, int n, int done, hipStream_t s);
// rt_display.hip k_resolve_linear: out[i] = base[i] + state[i].rgb / done, the base's alpha (not tone-mapped)
int rt_display_resolve_linear(rt_context* c, const float4_* base, const float4_* state, float4_* out, int n, int done,
                              hipStream_t s);
// rt_noise.hip k_noise_fold: half[i].rgb -= state[i].rgb (add: +=), half[i].w = 0
int rt_noise_fold(rt_context* c, float4_* half, const float4_* state, int n, bool add, hipStream_t s);
// rt_adapt.hip: the stages of an adaptive pass on s (P = c->prog; b->adapt holds the buffers).
//   select   tile errors with per-tile counts (estimate), flags, the ascending list and offsets, the counts'
//            update and the header, which it reads back: waits for s. hdr: rtk::AD_WORDS words.
//   gather   the active tiles' pixels into xy / idx / cstate; on an A pass half -= state for them
//   scatter  cstate back into the state; on an A pass half += state for them
//   bump     a uniform pass keeps the counts in step: tile_n += samples, on an A pass tile_nA too
//   resolve  k_resolve / k_resolve_linear with the pixel's tile count for `done`
int rt_adapt_select(rt_context* c, Backend* b, int samples, float threshold, bool estimate, bool a_pass, int32_t* hdr,
                    hipStream_t s);
int rt_adapt_gather(rt_context* c, Backend* b, int n_tiles_active, bool a_pass, hipStream_t s);
int rt_adapt_scatter(rt_context* c, Backend* b, int n_pixels, bool a_pass, hipStream_t s);
int rt_adapt_bump(rt_context* c, Backend* b, int samples, bool a_pass, hipStream_t s);
int rt_adapt_resolve(rt_context* c, Backend* b, const float4_* base, const float4_* state, float4_* out, bool linear,
                     hipStream_t s);
size_t rt_wave_counter_bytes();
size_t rt_wave_readback_bytes();
