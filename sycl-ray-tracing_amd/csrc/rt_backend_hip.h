// rt_backend_hip.h — what the translation units of the gfx950 backend share: the HIP error
// check, the owners of device resources (freed by their destructors), the per-device
// Backend, and the hooks between the units:
//   rt_backend.hip  contexts, uploads, the multi-device / variant / pixel-list drivers
//   rt_render.hip   the render kernels and their launch helpers (rt_wave_kernels.h)
//   rt_wave_run.hip the wavefront loop (run_wave) over them; rt_wave_layout.h: the counters both index
//   rt_probe.hip    rt_intersect's kernel and the test / measurement kernels no render launches
//   rt_denoise.hip  the post stage          rt_query.hip  the ray queries
//   rt_display.hip  the display stage and the linear resolve
//   rt_noise.hip    a tracked progression's fold and noise estimate
#pragma once

#include <hip/hip_runtime.h>

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

void rt_post_free(void* post);    // rt_denoise.hip (the device is current)
void rt_query_free(void* query);  // rt_query.hip (the device is current)

namespace rtk {
struct WaveView;
struct PixSrc;
}

// One device's resources. Created and destroyed with its device current (rt_backend.hip).
struct Backend {
    int device = 0;
    int index = 0;    // position in the context's device list (0: the root)
    Stream own;       // device-side work not on a caller's stream (multi-device shards, pixel lists)
    DevBuf nodes, tri4, prim2k, mat_idx, mats, emissive, spheres, env, env_lum, cdf;
    DevBuf bvh4, bvh16, bvh4s, bvh16s, bvh_tri4, parent, leaf_of, cdf_row, cdf_coarse, cdf_fence, matk;
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
    Event fev[RT_MAX_LANES], fev_done;
    Event hev[RT_MAX_LANES];  // fast lane: each lane's samples-done histogram readback
    bool fev_done_recorded = false;
    Event ftev[2];  // (timed renders: around the fast lane's kernel)
    Stream fs;      // the fast lane's stream with 4 lanes (fewer: the first idle lane stream)
    DevBuf xy;        // pixel list (rt_render_pixels)
    DevBuf fb;        // host-fb staging
    DevBuf pg_base, pg_state, pg_out;  // a progression (rt_progress_*): base values, paused state, host-resolve staging
    DevBuf pg_half, pg_noise;          // a tracked one: the A passes' sum; the host noise query's stat words and maps
    DevBuf disp;      // rt_display with host pointers: the frame (in, float out in place), then the 8-bit output
    DevBuf shard;     // multi-device renders: the root's N blocks of rows_max rows (scatter source /
                      // gather target); device d >= 1: its block
    Pinned<int32_t> h_act[RT_MAX_LANES];  // per lane: live-slot counters (sharded) + 8 fallback counters
    Event ev0, ev1;
    Event ev_pg;    // end of the last rt_progress_resolve_device: the next pass writes the state it reads
    bool pg_recorded = false;
    Event ev_done;  // end of the last run_wave (all lanes joined): the next render waits for it
    bool done_recorded = false;
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
    void* post = nullptr;           // the post stage's buffers (rt_denoise.hip owns them: rt_post_free)
    void* query = nullptr;          // the ray-query workspace (rt_query.hip owns it: rt_query_free)
    ~Backend()
    {
        if (post) rt_post_free(post);
        if (query) rt_query_free(query);
    }
};

struct RtRootDev {
    int device;               // HIP ordinal of the context's root device
    const RtSceneView* view;  // its scene view (valid after rt_backend_upload)
    hipEvent_t ev0, ev1;      // the events rt_last_kernel_ms / rt_device_last_kernel_ms read
    void** post;              // the post stage's state, created on first use; rt_post_free releases it
    void** query;             // the ray queries' workspace, likewise; rt_query_free releases it
    DevBuf* disp;             // the display stage's staging buffer (freed with the Backend)
};

int rt_backend_root(rt_context* c, RtRootDev* out);  // rt_backend.hip
Backend* rt_backend_dev0(rt_context* c);             // rt_backend.hip: the root device's Backend

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
size_t rt_wave_counter_bytes();
size_t rt_wave_readback_bytes();
