// rt_context.h — the state behind an rt_context* (include/rt_hip.h).
//
// Host-side scene state is shared; the compute backend (rt_render.hip for
// gfx950, rt_hostsim.cpp for the CPU debugging build used by the CPU test
// suite) implements the rt_backend_* hooks.
#pragma once

#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_device.h"
#include "rt_scene.h"

// The stages that have two kernels for one result, and the rt_test_schedule key that forces one: a value is
// clamped to 0..2 and 0 is the product's choice, the faster kernel as measured on the MI355X.
//   the first seven (a kernel of direct global loads and one that stages its footprint in LDS; for rt_denoise
//   and rt_denoise_var the à-trous filter of each step, for rt_bloom the reduce, for rt_motion_blur the gather):
//   RT_KERNEL_DIRECT or RT_KERNEL_LDS, resolved by rt_use_lds
//   rq, gb (the search-BVH kernel of rt_query and of rt_render_gbuffer): 1 plain rounds, 2 per-quad refill
enum RtVariant { RT_VAR_DN, RT_VAR_FF, RT_VAR_MT, RT_VAR_UP, RT_VAR_BLOOM, RT_VAR_DOF, RT_VAR_MOTION, RT_VAR_RQ, RT_VAR_GB, RT_VAR_COUNT };
constexpr struct {
    const char* key;
    RtVariant slot;
} rt_variant_keys[] = {{"dn_variant", RT_VAR_DN},       {"ff_variant", RT_VAR_FF},   {"mt_variant", RT_VAR_MT},
                       {"up_variant", RT_VAR_UP},       {"bloom_variant", RT_VAR_BLOOM}, {"dof_variant", RT_VAR_DOF},
                       {"motion_variant", RT_VAR_MOTION}, {"rq_variant", RT_VAR_RQ},   {"gb_variant", RT_VAR_GB}};
enum { RT_KERNEL_MEASURED = 0, RT_KERNEL_DIRECT = 1, RT_KERNEL_LDS = 2 };
// measured_choice: whether the LDS kernel is the faster one for this call (the caller quotes the figures)
inline bool rt_use_lds(int variant, bool measured_choice)
{
    return variant == RT_KERNEL_MEASURED ? measured_choice : variant == RT_KERNEL_LDS;
}

// Schedule of the wavefront loop (rt_wave_run.hip run_wave). The product runs the defaults
// (-1: the backend's own choice); rt_test_schedule (tests and measurement tools only,
// include/rt_hip.h) overrides them per context. No parameter changes a pixel: the GPU
// schedule tests render with each and compare the bits. Nothing here is read from the
// environment.
struct RtSchedule {
    int lanes = 0;             // wavefront lanes per render (0: auto, rt_device_set_lanes)
    int tail_paths = -1;       // k_tail paths per wave (0: no tail kernel)
    double tail_enter = -1.0;  // k_tail entry: live paths per lane, in grid-fills' pools
    int tail_rows = -1;        // k_tail walks by rows (1) or quads (0)
    int drain_rows = -1;       // k_trace: a drain's last walks continue as rows (0: off)
    int heavy_calls = -1;      // k_trace heavy class threshold in quad_visit calls (0: off)
    int spec_cam = -1;         // camera ray traced ahead: 0 never, 1 always, 2 where the last sample ended
    int tail_spec_cam = -1;    // the same in k_tail
    int force_fallback = 0;    // stressor: every k-th query (by a ray hash) skips to the exact walk
    int step_budget = -1;      // exact-walk steps per query per launch before it parks
    int fast_k = -1;           // fast lane: this many of the slowest paths to a tail kernel early (0: off)
    double fast_spp = -1.0;    // ... at the lanes' first readback from iteration fast_spp x spp on
    double near_scale = -1.0;  // near box: the scene's box widened by this x its largest extent (rt_view_near;
                               // study probes only: answers never depend on it, only which walk gives them)
    int variant[RT_VAR_COUNT] = {};  // the forced kernel of each stage that has two (RtVariant), 0: as measured
    int mt_blocks = 0;         // rt_meter's grid: 0 the product's cap, n > 0 that many blocks (many grid-stride rounds)
    int gb_force_every = 0;    // stressor: G-buffer pixels with i % N == 0 skip to the exact walk's list (0: off)
    bool chain_full = false;   // the scene view reports chain_monotone = 0: chain_ok / quad_chain_ok run their full
                               // ancestor-chain loop (rt_fast.h), which no tree the host builds reaches otherwise
};

// Diagnostics, read from the environment once when the context is created (rt_create*):
// RT_TIMELINE (per-launch timeline file), RT_ITER_LOG (per-iteration log prefix),
// RT_VERBOSE. They change no result and no schedule.
struct RtDiag {
    std::string timeline, iter_log;
    bool verbose = false;
    // walk log (rt_test_walk_log): stats renders record every search-BVH walk of at least
    // min_calls quad_visit calls (row trips count 2), up to cap records of RT_WLOG_FLOATS
    int wlog_min = 0, wlog_cap = 0, wlog_every = 1;
    std::vector<float> wlog;  // the last stats render's records
    long wlog_total = 0;      // walks that qualified (may exceed cap)
};

// A progression (rt_progress_*, include/rt_hip.h): a frame of `total` samples rendered in
// passes. `done` is uniform over the pixels. The buffers (base values and paused state, one
// float4 per pixel of the row shard each) belong to the backend: on the device for gfx950,
// the two vectors here for the hostsim build.
// Tracked (rt_progress_noise_track): the backend keeps one more buffer, `half`, the rgb sum of the
// samples of the A passes (rt_noise.h). `passes` counts the advances that rendered a sample, from
// 0; the even ones are A passes and n_a is their samples, so the B passes' are done - n_a.
struct RtProgress {
    bool active = false;
    int w = 0, h = 0, total = 0, done = 0, bounces = 0, off = 0, stride = 1, rows = 0;
    bool tracked = false;
    int passes = 0, n_a = 0;
    // Adaptive (rt_progress_advance_adaptive, rt_adapt.h): the backend keeps tile_n and tile_nA per 8x8
    // tile. `done` is then the smallest tile_n and tile_max the largest (the host's copy of the last
    // selection's header); n_a and n_b are what a tile active in every pass has.
    bool adaptive = false;
    int n_b = 0, tile_max = 0;
    std::vector<float4_> base, state, half;  // (hostsim only)
    std::vector<int32_t> tile_n, tile_nA;    // (hostsim only)
    size_t npx() const { return (size_t)rows * w; }
    int tiles_w() const { return (w + 7) / 8; }
    int tiles_h() const { return (rows + 7) / 8; }
    bool next_is_a() const { return tracked && (passes & 1) == 0; }
};

struct rt_context {
    int device = 0;
    RtSchedule sched;
    RtProgress prog;
    RtDiag diag;
    // rt_create_multi: the devices a render shards over (rows y -> device y mod N, RCCL
    // scatter / gather through devices[0]); empty for a single-device context (rt_create).
    // One entry: a single-device context on that ordinal (nothing to shard, no RCCL)
    std::vector<int> devices;
    bool loopback = false;        // devices may repeat: shards exchanged by device copies, not RCCL
    bool force_multi = false;     // (rt_test_create_multi_rccl) the multi-device driver and RCCL even for one device
    int fail_device = -1;         // rt_test_fail_device (tests only): that device fails its share
    std::string err;

    // RenderKernel constructor inputs (render_kernel.h:27-34)
    std::vector<float> tris;      // [N][9]
    std::vector<int32_t> mat_idx; // >= N entries (spheres append theirs)
    std::vector<RtMat> mats;
    std::vector<int32_t> emissive;
    std::vector<float4_> spheres; // 2 records per sphere
    bool have_scene = false;

    rt::Octree octree;
    rt::FlatBvh flat;
    bool have_bvh = false;

    std::vector<float4_> env;     // RGBA, alpha 0
    std::vector<float> env_lum, cdf;
    std::vector<float> cdf_row, cdf_coarse;  // exact copies of CDF entries (rt_trace.h cdf_search)
    std::vector<float> cdf_fence;            // fence tables of the counting search (empty: not eligible)
    int cdf_cw = 0;
    int ew = 0, eh = 0;
    bool have_env = false;

    RtCamera cam{};
    bool have_cam = false;

    bool brute = false;           // USE_BVH 0 (rt_set_intersect_mode)
    bool stats_enabled = false;
    bool stats_seq = false;       // rt_set_stats(ctx, 2): occlusion walks unpaired (gfx950), see rt_hip.h
    unsigned long long stats[2 * RT_STAT_COUNT] = {};  // all kernels, then the gfx950 tail kernel's share
    double last_kernel_ms = 0.0;
    long query_exact = 0;         // rt_query_last_exact: the last call's exact-walk count where the host knows it,
    bool query_on_device = false; // ... else (gfx950, a routed call) it is read from the device's fallback counter
    long gbuffer_exact = 0;         // rt_gbuffer_last_exact: the same pair for the last rt_render_gbuffer call
    bool gbuffer_on_device = false;

    bool dirty = true;            // host state changed since the last upload
    bool mats_dirty_only = false; // only the material table changed (rt_set_materials)
    void* backend = nullptr;
};

// ---- backend hooks
int rt_backend_create(rt_context* ctx);
void rt_backend_destroy(rt_context* ctx);
int rt_backend_upload(rt_context* ctx);
// linear: the render stops before its tone-map pass (rt_render_linear: the framebuffer keeps
// entry + final_color / samples); the flag travels with every shard of a multi-device render
int rt_backend_render(rt_context* ctx, int w, int h, int spp, int bounces, float* host_fb, void* dev_fb, int row_offset,
                      int row_stride, void* stream, bool linear = false);
// n_variants material tables (RtMat, n_mats each, back to back); variant v on device v mod N
int rt_backend_render_variants(rt_context* ctx, int w, int h, int spp, int bounces, int n_variants,
                               const std::vector<RtMat>& tables, int n_mats, int row_offset, int row_stride,
                               float* host_fb, void* const* d_fbs);
// rt_scene_has_emissive_prim for another material table over the context's material indices
bool rt_table_has_emissive_prim(const rt_context* ctx, const RtMat* table);
int rt_backend_render_pixels(rt_context* ctx, int w, int h, int spp, int bounces, const int* xy, int n, float* rgba);
int rt_backend_intersect(rt_context* ctx, const float* rays, int n, void* out);
// The post stage (rt_denoise.h), on the context's root device. device = false: host buffers,
// synchronous; true: device buffers on `stream`, no wait (hostsim: host pointers, stream unused).
int rt_backend_features(rt_context* ctx, int w, int h, void* albedo, void* normal_depth, bool device, void* stream);
// alb and nd both null: colour only. p is validated (rt_capi_stages.cpp).
int rt_backend_denoise(rt_context* ctx, int w, int h, const void* in, const void* alb, const void* nd,
                       const rt_denoise_params& p, float blend, void* out, bool device, void* stream);
// The variance-guided filter (rt_dnv.h): rt_backend_denoise plus sigma (w*h floats) and the optional
// sigma_out (w*h floats, or null). p is validated (rt_capi_stages.cpp).
int rt_backend_denoise_var(rt_context* ctx, int w, int h, const void* in, const void* sigma, const void* alb, const void* nd,
                           const rt_denoise_var_params& p, float blend, void* out, void* sigma_out, bool device,
                           void* stream);
// Temporal accumulation (rt_temporal.h), on the root device like the post stage: T holds the cameras, the
// validated parameters and the caller's seven input buffers (the four of the history all null: the first
// frame); rgba_out (w*h float4), sigma_out and len_out (w*h floats each) are required.
namespace rtk {
struct TemporalFrame;
}
int rt_backend_temporal(rt_context* ctx, rtk::TemporalFrame T, void* rgba_out, void* sigma_out, void* len_out, bool device,
                        void* stream);
// Firefly rejection (rt_firefly.h), on the root device like the post stage: A holds the validated parameters,
// the frame (w*h float4) and its sigma (w*h floats, or null); rgba_out (w*h float4) is required, sigma_out
// (null when A.sigma is) and scale_out (w*h floats each) may be null.
namespace rtk {
struct FireflyArgs;
}
int rt_backend_firefly(rt_context* ctx, rtk::FireflyArgs A, void* rgba_out, void* sigma_out, void* scale_out, bool device,
                       void* stream);
// Exposure metering (rt_meter.h), on the root device like the post stage: in (w*h float4) -> hist
// (rtk::MT_WORDS uint32 words, cleared by the call). The arguments are validated (rt_capi_stages.cpp).
int rt_backend_meter(rt_context* ctx, int w, int h, const void* in, void* hist, bool device, void* stream);
// The guided upscale (rt_upscale.h), on the root device like the post stage: A holds the validated sizes and
// parameters, the low frame (w_lo*h_lo float4), its sigma (floats, or null) and guides, and the full-size guides
// (w*h float4); rgba_out (w*h float4) is required, sigma_out (w*h floats) is null exactly when A.sigma_lo is.
namespace rtk {
struct UpArgs;
}
int rt_backend_upscale(rt_context* ctx, rtk::UpArgs A, void* rgba_out, void* sigma_out, bool device, void* stream);
// Bloom (rt_bloom.h), on the root device like the post stage: A holds the validated parameters (scale =
// intensity / levels) and the frame (w*h float4); rgba_out (w*h float4) is required, layer_out (w*h float4) may be null.
namespace rtk {
struct BloomArgs;
}
int rt_backend_bloom(rt_context* ctx, rtk::BloomArgs A, void* rgba_out, void* layer_out, bool device, void* stream);
// Depth of field (rt_dof.h), on the root device like the post stage: A holds the validated parameters, the table of
// tap distances, the frame and its guide record (w*h float4 each); rgba_out (w*h float4) is required, coc_out (w*h
// floats) may be null.
namespace rtk {
struct DofArgs;
}
int rt_backend_dof(rt_context* ctx, rtk::DofArgs A, void* rgba_out, void* coc_out, bool device, void* stream);
// The motion stages (rt_motion.h), on the root device like the post stage. Vectors: A holds the current camera's view, the
// previous camera's inverse and origin and the guides (w*h float4); motion_out is w*h float2. Blur: A holds the validated
// parameters, the frame, its guide record (w*h float4 each) and the motion (w*h float2); rgba_out (w*h float4) is
// required, reach_out (w*h floats) may be null. rt_motion_vec_args (rt_capi_stages.cpp) fills a MotionVecArgs from an
// already validated call (the measurement hook of rt_motion.hip).
namespace rtk {
struct MotionVecArgs;
struct MotionArgs;
}
int rt_backend_motion_vectors(rt_context* ctx, rtk::MotionVecArgs A, void* motion_out, bool device, void* stream);
int rt_backend_motion_blur(rt_context* ctx, rtk::MotionArgs A, void* rgba_out, void* reach_out, bool device, void* stream);
int rt_motion_vec_args(rt_context* ctx, int w, int h, const void* nd, const float* prev_view, float prev_fov_dist, rtk::MotionVecArgs& A);
// The display stage (rt_display.h), on the root device like the post stage: in (w*h float4) ->
// out (w*h float4, may be `in`, or null) and out8 (w*h RGBA bytes, rows reversed when flip, or
// null). The arguments are validated and inv_gamma = 1.0f / gamma (rt_capi_stages.cpp).
int rt_backend_display(rt_context* ctx, int w, int h, const void* in, float exposure, float inv_gamma, bool flip,
                       void* out, void* out8, bool device, void* stream);

// The ray queries (rt_query.h): n > 0 rays[n][6] -> out (closest: int32[n][11], any: int32[n]);
// all_exact: every query takes the exact walk. device = false: host buffers, synchronous;
// true: device buffers on `stream`, no wait (hostsim: host pointers, stream unused).
int rt_backend_query(rt_context* ctx, bool any, bool all_exact, const void* rays, long n, void* out, bool device,
                     void* stream);
// Queries of the last rt_backend_query that took the exact walk (waits for them); < 0: an error.
long rt_backend_query_last_exact(rt_context* ctx);

// The first-hit G-buffer (rt_gbuffer.h), on the root device like the post stage: albedo and normal_depth
// (w*h float4 each) and the optional ids (w*h int32 pairs, or null); all_exact: every pixel takes the
// exact walk. The arguments are validated (rt_capi_stages.cpp). Both forms as rt_backend_query.
int rt_backend_gbuffer(rt_context* ctx, int w, int h, bool all_exact, void* albedo, void* normal_depth, void* ids,
                       bool device, void* stream);
// Pixels of the last rt_backend_gbuffer that took the exact walk (waits for them); < 0: an error.
long rt_backend_gbuffer_last_exact(rt_context* ctx);

// Progressions (ctx->prog describes the frame; single-device contexts only, arguments validated).
// begin: the backend's buffers for prog.npx() pixels; base / state: host float4 per pixel, or
// null for (0, 0, 0, 1) / zeroes. advance: samples first .. stop - 1 of every pixel (device:
// on `stream`, no wait). resolve: the image after prog.done samples into host_fb (waits) or
// dev_fb (on `stream`); linear: base + state / done, not tone-mapped. read: base and state back
// to the host (waits). end: frees the buffers.
int rt_backend_progress_begin(rt_context* ctx, const float* base, const float* state);
int rt_backend_progress_advance(rt_context* ctx, int first, int stop, void* stream);
int rt_backend_progress_resolve(rt_context* ctx, float* host_fb, void* dev_fb, void* stream, bool linear = false);
int rt_backend_progress_read(rt_context* ctx, float* base, float* state);
void rt_backend_progress_end(rt_context* ctx);
// A tracked progression (ctx->prog.tracked is set by the caller once track succeeds). track: the
// half buffer, prog.npx() float4 from `half` (host) or zeroes for null. advance folds the state into
// it around a pass for which prog.next_is_a() holds, on the pass's stream. read_half: back to the
// host (waits). noise: the estimate of rt_noise.h from the state and half; stats: 8 int32 words;
// pixel_err (rows * w floats) and tile_err (tiles_h * tiles_w floats) may be null. device = false:
// host buffers, waits; true: device buffers on `stream`, no wait (hostsim: host pointers).
namespace rtk {
struct NoiseArgs;
}
int rt_backend_progress_track(rt_context* ctx, const float* half);
int rt_backend_progress_read_half(rt_context* ctx, float* half);
int rt_backend_progress_noise(rt_context* ctx, const rtk::NoiseArgs& args, int32_t* stats, float* pixel_err,
                              float* tile_err, bool device, void* stream);
// noise_sigma: the estimate's numerator k * d per pixel (rt_dnv.h; rows * w floats), with the tile's counts
// when prog.adaptive; args: the frame's counts as for noise. Both forms as noise.
int rt_backend_progress_noise_sigma(rt_context* ctx, const rtk::NoiseArgs& args, float* sigma, bool device, void* stream);
// An adaptive progression (rt_adapt.h; ctx->prog.adaptive is set by the caller once adapt_begin succeeds).
// adapt_begin: the two count arrays, tiles_h * tiles_w int32 each, from the host arrays or, for null,
//   prog.done and prog.n_a in every tile. With prog.adaptive set, resolve divides by the pixel's tile count.
// adapt_bump: a uniform pass of `samples` keeps the counts in step (on `stream`, behind the pass).
// adapt_advance: one adaptive pass. Waits for the progression's queued work, selects (one small readback),
//   then enqueues gather, the pass over the compact pixel list and scatter on `stream`; hdr: rtk::AD_WORDS
//   words {active tiles, active pixels, capped, min and max count after, tiles, 0, 0}. No active tile: no pass.
// adapt_counts: the arrays back to the host (waits); either may be null.
// adapt_noise: rt_backend_progress_noise with the tile's counts in k and both divisions (args: the
//   threshold and the stat words 4..6).
int rt_backend_progress_adapt_begin(rt_context* ctx, const int32_t* tile_n, const int32_t* tile_nA);
int rt_backend_progress_adapt_bump(rt_context* ctx, int samples, bool a_pass, void* stream);
int rt_backend_progress_adapt_advance(rt_context* ctx, int samples, float threshold, void* stream, int32_t* hdr);
int rt_backend_progress_adapt_counts(rt_context* ctx, int32_t* tile_n, int32_t* tile_nA);
int rt_backend_progress_adapt_noise(rt_context* ctx, const rtk::NoiseArgs& args, int32_t* stats, float* pixel_err,
                                    float* tile_err, bool device, void* stream);

int rt_fail(rt_context* ctx, int code, const std::string& msg);
// The device tables made current before a call that reads them (rt_capi_host.cpp; rt_capi_stages.cpp for the
// feature buffers). mats_too: a changed material table alone is a reason too; env_stub: bind the placeholder
// env first (the calls that need no env).
int rt_tables_current(rt_context* ctx, bool mats_too, bool env_stub);
// RtDiag from the environment (rt_create*)
void rt_read_diag(rt_context* ctx);
// While set (per host thread), rt_fail writes its message to *sink instead of the
// context: the per-device threads of a multi-device render report into their own
// slots, and the caller raises the error once, after the join (rt_for_devices).
void rt_err_sink(std::string* sink);

// fn(d) for every device d of a multi-device render: d >= 1 on threads of their own,
// d = 0 on the caller's. Each device's errors go to its own slot; after the join the
// lowest failing device's code and message are raised on the context (one writer).
// c->fail_device (rt_test_fail_device, tests only) fails that device before its work starts.
template <class F>
int rt_for_devices(rt_context* c, int n, F fn)
{
    std::vector<int> rc(n, 0);
    std::vector<std::string> msg(n);
    const int inject = c->fail_device;
    auto one = [&](int d) {
        rt_err_sink(&msg[d]);
        rc[d] = d == inject ? rt_fail(c, RT_ERR_STATE, "injected failure (rt_test_fail_device)") : fn(d);
        rt_err_sink(nullptr);
    };
    {
        std::vector<std::thread> th;
        for (int d = 1; d < n; d++) th.emplace_back(one, d);
        one(0);
        for (auto& t : th) t.join();
    }
    for (int d = 0; d < n; d++)
        if (rc[d]) return rt_fail(c, rc[d], "device " + std::to_string(d) + ": " + msg[d]);
    return 0;
}
RtSceneView rt_host_view(const rt_context* ctx);  // host-memory view (hostsim)
// The view's fields that do not depend on where the tables live: the counts, the env's size and
// CDF scalars, chain_monotone, brute and the near box. Both builds start their view with it.
void rt_view_scalars(const rt_context* ctx, RtSceneView& v);
// The context's host tables, each with the view's pointer to it: f(vector, field) for every one.
// The host view points at the vectors, the device view at its upload of each. Not listed, because
// the builds differ there: tri4 and mats (the device patches the one and re-sends the other alone),
// matk (device only), tri_mat, and cdf_fence's null when the table is empty.
#define RT_SCENE_TABLES 18
template <class F>
void rt_scene_tables(const rt_context* c, RtSceneView& v, F f)
{
    f(c->flat.nodes, v.nodes), f(c->flat.prim2k, v.prim2k), f(c->mat_idx, v.mat_idx), f(c->emissive, v.emissive);
    f(c->spheres, v.spheres), f(c->env, v.env), f(c->env_lum, v.env_lum), f(c->cdf, v.cdf);
    f(c->cdf_row, v.cdf_row), f(c->cdf_coarse, v.cdf_coarse), f(c->cdf_fence, v.cdf_fence);
    f(c->flat.bvh4, v.bvh4), f(c->flat.bvh16, v.bvh16), f(c->flat.bvh4s, v.bvh4s), f(c->flat.bvh16s, v.bvh16s);
    f(c->flat.bvh_tri4, v.bvh_tri4), f(c->flat.parent, v.parent), f(c->flat.leaf_of, v.leaf_of);
}
// The view's near box (rt_fast.h far_origin): the octree root's axis planes (the scene's box)
// widened on every side by RT_NEAR_SCALE (or sched.near_scale) x the box's largest extent;
// unbounded for an empty scene.
#ifndef RT_NEAR_SCALE
#define RT_NEAR_SCALE 0.5
#endif
void rt_view_near(const rt_context* ctx, RtSceneView& v);
// The view's chain_monotone: the built tree's (rt_scene.h FlatBvh), 0 under sched.chain_full.
int rt_view_chain_monotone(const rt_context* ctx);
// Does any primitive (triangle or sphere) use a material with a positive
// emission component (the test at render_kernel.cpp:696)? If not, the
// BRDF->light query of sample_light_sources can never contribute.
bool rt_scene_has_emissive_prim(const rt_context* ctx);
