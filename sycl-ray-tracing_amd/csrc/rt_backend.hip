// rt_backend.hip — the kernel-free half of the gfx950 backend: contexts and their devices
// (create / destroy / upload, RCCL loading), the multi-device, variant and pixel-list
// drivers over rt_wave_run.hip's run_wave, and the rt_device_* accessors.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <dlfcn.h>

#include <rccl/rccl.h>

#include "rt_adapt.h"
#include "rt_backend_hip.h"
#include "rt_wave.h"

namespace {
// A context drives one Backend per device. rt_create: one device, renders on the
// caller's stream. rt_create_multi: devices[0] is the root that holds the caller's
// framebuffer; a render shards its rows over the devices (render_multi).
struct Group {
    std::vector<Backend*> dev;     // dev[0]: the root
    bool multi = false;            // rt_create_multi over two or more devices
    bool loopback = false;         // (RT_MULTI_LOOPBACK test contexts) shards exchanged by device copies
    std::vector<ncclComm_t> comms; // ncclCommInitAll over the devices, in order (RCCL exchange)
};

Group* grp(rt_context* c) { return (Group*)c->backend; }
Backend* be(rt_context* c) { return grp(c)->dev[0]; }

// RCCL, loaded on the first multi-device context: the library need not be present
// (or be the same build as a framework's own copy) for single-device use.
struct Rccl {
    void* h = nullptr;
    decltype(&ncclCommInitAll) init = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclScatter) scatter = nullptr;
    decltype(&ncclGather) gather = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) errstr = nullptr;
};
std::mutex g_rccl_mu;
Rccl g_rccl;

const Rccl* rccl_load(std::string& err)
{
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.h) return &g_rccl;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        err = std::string("librt_hip: RCCL not found (librccl.so.1): ") + dlerror();
        return nullptr;
    }
    Rccl r;
    r.h = h;
    r.init = (decltype(r.init))dlsym(h, "ncclCommInitAll");
    r.destroy = (decltype(r.destroy))dlsym(h, "ncclCommDestroy");
    r.scatter = (decltype(r.scatter))dlsym(h, "ncclScatter");
    r.gather = (decltype(r.gather))dlsym(h, "ncclGather");
    r.group_start = (decltype(r.group_start))dlsym(h, "ncclGroupStart");
    r.group_end = (decltype(r.group_end))dlsym(h, "ncclGroupEnd");
    r.errstr = (decltype(r.errstr))dlsym(h, "ncclGetErrorString");
    if (!r.init || !r.destroy || !r.scatter || !r.gather || !r.group_start || !r.group_end || !r.errstr) {
        err = "librt_hip: librccl.so.1 lacks ncclCommInitAll / ncclScatter / ncclGather";
        return nullptr;
    }
    g_rccl = r;
    return &g_rccl;
}

#define NCCLCHK(ctx, R, expr)                                                                    \
    do {                                                                                         \
        ncclResult_t e_ = (expr);                                                                \
        if (e_ != ncclSuccess) return rt_fail(ctx, RT_ERR_HIP, std::string(#expr ": ") + (R)->errstr(e_)); \
    } while (0)

int create_one(rt_context* c, int device, Backend** out)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return rt_fail(c, RT_ERR_NODEV, "librt_hip: no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= n) return rt_fail(c, RT_ERR_NODEV, "librt_hip: device index out of range");
    HIPCHK(c, hipSetDevice(device));
    Backend* b = new Backend();
    *out = b;
    b->device = device;
    HIPCHK(c, hipEventCreate(&b->ev0.h));
    HIPCHK(c, hipEventCreate(&b->ev1.h));
    for (int l = 0; l < RT_MAX_LANES; l++) {
        HIPCHK(c, hipHostMalloc((void**)&b->h_act[l].h, rt_wave_readback_bytes(), hipHostMallocDefault));
        HIPCHK(c, hipEventCreateWithFlags(&b->ev_lane[l].h, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&b->ev_join[l].h, hipEventDisableTiming));
        if (l > 0) HIPCHK(c, hipStreamCreateWithFlags(&b->ls[l].h, hipStreamNonBlocking));
    }
    HIPCHK(c, hipStreamCreateWithFlags(&b->own.h, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&b->ev_fork.h, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&b->ev_done.ev.h, hipEventDisableTiming));
    return RT_OK;
}

void destroy_one(Backend* b)
{
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    delete b;
}

// Scene, BVH and env of the context into one device's memory (replicated per device).
int upload_one(rt_context* c, Backend* b, const std::vector<int32_t>& matk, bool mats_only)
{
    HIPCHK(c, hipSetDevice(b->device));
    // the previous render may still run (rt_render_device returns at once, its kernels on
    // non-blocking streams that a null-stream copy does not wait for): it reads these tables
    if (int r = b->ev_done.sync(c)) return r;
    int r = 0;
    if (mats_only) {  // rt_set_materials: the material table (and what depends on it) alone
        if ((r = upload(c, b->mats, c->mats))) return r;
        b->view.mats = (const RtMat*)b->mats.p;
        b->view.n_mats = (int)c->mats.size();
        b->bl_rays = rt_scene_has_emissive_prim(c) ? 1 : 0;
        return RT_OK;
    }
    // device triangle records carry the material index in e1.w (rt_wave.h hit_from)
    std::vector<float4_> tri4 = c->flat.tri4;
    for (size_t k = 0; k < matk.size(); k++) std::memcpy(&tri4[3 * k + 1].w, &matk[k], 4);
    if ((r = upload(c, b->tri4, tri4)) || (r = upload(c, b->mats, c->mats)) || (r = upload(c, b->matk, matk)) ||
        (r = ensure(c, b->stats, 2 * RT_STAT_COUNT * sizeof(unsigned long long))))
        return r;
    for (int l = 0; l < RT_MAX_LANES; l++)
        if ((r = ensure(c, b->counters[l], rt_wave_counter_bytes()))) return r;
    RtSceneView v{};
    rt_view_scalars(c, v);
    int i = 0;
    rt_scene_tables(c, v, [&](const auto& table, auto& field) {
        DevBuf& d = b->tables[i++ % RT_SCENE_TABLES];
        if (!r) r = upload(c, d, table);
        field = (std::remove_reference_t<decltype(field)>)d.p;
    });
    if (r) return r;
    v.tri4 = (const float4_*)b->tri4.p;
    v.mats = (const RtMat*)b->mats.p;
    v.matk = (const int32_t*)b->matk.p;
    if (c->cdf_fence.empty()) v.cdf_fence = nullptr;
    v.tri_mat = 1;
    b->view = v;
    b->bl_rays = rt_scene_has_emissive_prim(c) ? 1 : 0;
    b->any_rays = v.n_spheres == 0 ? 1 : 0;
    return RT_OK;
}
}  // namespace

int rt_backend_create(rt_context* c)
{
    Group* g = new Group();
    c->backend = g;
    // (one listed device: a single-device context on it, unless a test asks for the driver
    // and a one-rank RCCL clique: rt_test_create_multi_rccl)
    g->multi = c->devices.size() > 1 || (c->force_multi && !c->devices.empty());
    g->loopback = g->multi && c->loopback;
    const std::vector<int> ids = g->multi ? c->devices : std::vector<int>{c->device};
    for (int d : ids) {
        Backend* b = nullptr;
        const int r = create_one(c, d, &b);
        if (b) {
            b->index = (int)g->dev.size();
            g->dev.push_back(b);
        }
        if (r) return r;
    }
    if (g->multi && !g->loopback) {
        std::string err;
        const Rccl* R = rccl_load(err);
        if (!R) return rt_fail(c, RT_ERR_NODEV, err);
        g->comms.resize(ids.size());
        NCCLCHK(c, R, R->init(g->comms.data(), (int)ids.size(), ids.data()));
    }
    return RT_OK;
}

void rt_backend_destroy(rt_context* c)
{
    Group* g = grp(c);
    if (!g) return;
    for (Backend* b : g->dev) destroy_one(b);
    if (!g->comms.empty()) {
        std::string err;
        if (const Rccl* R = rccl_load(err))
            for (ncclComm_t cm : g->comms)
                if (cm) (void)R->destroy(cm);
    }
    delete g;
    c->backend = nullptr;
}

int rt_backend_upload(rt_context* c)
{
    Group* g = grp(c);
    const bool mats_only = c->mats_dirty_only && !c->dirty;
    // material index of each leaf-order triangle k: mat_idx[prim(k)] (rt_trace.h load_mat_hit)
    std::vector<int32_t> matk;
    if (!mats_only) {
        matk.resize(c->flat.tri4.size() / 3);
        for (size_t k = 0; k < matk.size(); k++) {
            int32_t prim;
            std::memcpy(&prim, &c->flat.tri4[3 * k].w, 4);
            matk[k] = c->mat_idx[prim];
        }
    }
    for (Backend* b : g->dev)
        if (int r = upload_one(c, b, matk, mats_only)) return r;
    return RT_OK;
}


namespace {
int finish_stats(rt_context* c, Backend* b, hipStream_t s)
{
    if (!c->stats_enabled) return RT_OK;
    HIPCHK(c, hipMemcpyAsync(c->stats, b->stats.p, sizeof(c->stats), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return RT_OK;
}

// Rows of a multi-device render: request row j (image row off + j*stride) belongs to
// device j mod N. Device d's rows go to block d of the root's staging buffer (rows_max
// rows each; the tail of a short block is padding), ncclScatter sends block d to
// device d, every device renders its block with its own wavefront loop (one host
// thread per device: run_wave polls its lanes), and ncclGather brings the blocks back
// for the un-permute. Pack and un-permute are strided 2-D copies on the root.
int render_multi(rt_context* c, Group* g, int w, int h, int spp, int bounces, float4_* fb, int off, int stride,
                 hipStream_t s, bool linear)
{
    const int N = (int)g->dev.size();
    std::string err;
    const Rccl* R = nullptr;
    if (!g->loopback && !(R = rccl_load(err))) return rt_fail(c, RT_ERR_NODEV, err);
    const int rows = (h - off + stride - 1) / stride;
    const int rows_max = (rows + N - 1) / N;
    const size_t blk = (size_t)rows_max * w;  // float4 per block
    auto rows_of = [&](int d) { return rows > d ? (rows - d + N - 1) / N : 0; };
    Backend* root = g->dev[0];
    for (int d = 1; d < N; d++) {
        HIPCHK(c, hipSetDevice(g->dev[d]->device));
        if (int r = ensure(c, g->dev[d]->shard, std::max<size_t>(blk, 1) * sizeof(float4_))) return r;
    }
    HIPCHK(c, hipSetDevice(root->device));
    if (int r = ensure(c, root->shard, std::max<size_t>(blk, 1) * N * sizeof(float4_))) return r;
    float4_* stage = (float4_*)root->shard.p;
    HIPCHK(c, hipEventRecord(root->ev0, s));
    const size_t pitch = (size_t)w * sizeof(float4_);
    for (int d = 0; d < N; d++)
        if (rows_of(d))
            HIPCHK(c, hipMemcpy2DAsync(stage + d * blk, pitch, fb + (size_t)d * w, N * pitch, pitch, rows_of(d),
                                       hipMemcpyDeviceToDevice, s));
    std::vector<hipStream_t> st(N);
    for (int d = 0; d < N; d++) st[d] = d == 0 ? s : g->dev[d]->own;
    const size_t cnt = blk * 4;  // floats per block
    if (g->loopback) {  // block d -> device d by a device copy on the root stream; the shard streams wait for it
        for (int d = 1; d < N; d++)
            HIPCHK(c, hipMemcpyAsync(g->dev[d]->shard.p, stage + d * blk, blk * sizeof(float4_), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipEventRecord(root->ev_fork, s));
        for (int d = 1; d < N; d++) {
            HIPCHK(c, hipSetDevice(g->dev[d]->device));
            HIPCHK(c, hipStreamWaitEvent(st[d], root->ev_fork, 0));
        }
        HIPCHK(c, hipSetDevice(root->device));
    } else {
        NCCLCHK(c, R, R->group_start());
        for (int d = 0; d < N; d++)
            NCCLCHK(c, R, R->scatter(stage, d == 0 ? (void*)stage : g->dev[d]->shard.p, cnt, ncclFloat, 0, g->comms[d], st[d]));
        NCCLCHK(c, R, R->group_end());
    }
    // the wavefront loops, one host thread per device; errors are collected per device
    // and raised once after the join (rt_for_devices). run_wave resets the stats itself.
    if (int r = rt_for_devices(c, N, [&](int d) -> int {
            Backend* b = g->dev[d];
            HIPCHK(c, hipSetDevice(b->device));
            const rtk::PixSrc src{w, off + d * stride, N * stride, nullptr};
            float4_* dst = d == 0 ? stage : (float4_*)g->dev[d]->shard.p;
            return run_wave(c, b, w, h, spp, bounces, src, rows_of(d) * w, dst, st[d], nullptr, linear);
        }))
        return r;
    HIPCHK(c, hipSetDevice(root->device));
    if (g->loopback) {  // each block back to the root after its device's loop; the root stream waits for all
        for (int d = 1; d < N; d++) {
            Backend* b = g->dev[d];
            HIPCHK(c, hipSetDevice(b->device));
            HIPCHK(c, hipMemcpyAsync(stage + d * blk, g->dev[d]->shard.p, blk * sizeof(float4_), hipMemcpyDeviceToDevice, st[d]));
            HIPCHK(c, hipEventRecord(b->ev_join[0], st[d]));
            HIPCHK(c, hipSetDevice(root->device));
            HIPCHK(c, hipStreamWaitEvent(s, b->ev_join[0], 0));
        }
    } else {
        NCCLCHK(c, R, R->group_start());
        for (int d = 0; d < N; d++)
            NCCLCHK(c, R, R->gather(d == 0 ? (const void*)stage : g->dev[d]->shard.p, stage, cnt, ncclFloat, 0, g->comms[d], st[d]));
        NCCLCHK(c, R, R->group_end());
    }
    for (int d = 0; d < N; d++)
        if (rows_of(d))
            HIPCHK(c, hipMemcpy2DAsync(fb + (size_t)d * w, N * pitch, stage + d * blk, pitch, pitch, rows_of(d),
                                       hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipEventRecord(root->ev1, s));
    if (c->stats_enabled) {  // counters summed over the devices
        unsigned long long sum[2 * RT_STAT_COUNT] = {};
        for (int d = 0; d < N; d++) {
            HIPCHK(c, hipSetDevice(g->dev[d]->device));
            HIPCHK(c, hipMemcpyAsync(c->stats, g->dev[d]->stats.p, sizeof(c->stats), hipMemcpyDeviceToHost, st[d]));
            HIPCHK(c, hipStreamSynchronize(st[d]));
            for (int i = 0; i < 2 * RT_STAT_COUNT; i++) sum[i] += c->stats[i];
        }
        std::memcpy(c->stats, sum, sizeof sum);
        HIPCHK(c, hipSetDevice(root->device));
    }
    root->last_iters = 0;
    for (Backend* b : g->dev) root->last_iters = std::max(root->last_iters, b->last_iters);
    return RT_OK;
}
}  // namespace

int rt_backend_render(rt_context* c, int w, int h, int spp, int bounces, float* host_fb, void* dev_fb, int row_offset,
                      int row_stride, void* stream, bool linear)
{
    Group* g = grp(c);
    Backend* b = be(c);
    StagedCall st;  // (the host form runs on `stream` too: rt_render passes the null stream)
    if (int r = st.enter(c, b, host_fb == nullptr, stream, (hipStream_t)stream)) return r;
    hipStream_t s = st.s;
    const int rows_local = (h - row_offset + row_stride - 1) / row_stride;
    const size_t npx = (size_t)rows_local * w;
    if (npx > 0x7fffffff / 8) return rt_fail(c, RT_ERR_ARG, "render: too many pixels for one launch");
    if (int r = st.staging(b->fb, npx * sizeof(float4_))) return r;
    float4_* fb = (float4_*)st.inout(host_fb ? (void*)host_fb : dev_fb, host_fb, npx * sizeof(float4_));
    if (g->multi) {  // (render_multi records the root's ev0 and ev1 itself, around its pack and un-permute)
        if (st.err) return st.err;
        if (int r = render_multi(c, g, w, h, spp, bounces, fb, row_offset, row_stride, s, linear)) return r;
        return st.finish();
    }
    rtk::PixSrc src{w, row_offset, row_stride, nullptr};
    if (int r = st.begin()) return r;
    if (int r = run_wave(c, b, w, h, spp, bounces, src, (int)npx, fb, s, nullptr, linear)) return r;
    if (int r = st.end()) return r;
    return finish_stats(c, b, s);
}

// The material sweep as replicas (rt_render_variants): variant v on device v mod N, one
// host thread per device (rt_for_devices), each device walking its variants in order on
// its own stream: the variant's table goes into the device's material buffer with a copy
// ordered after the previous variant's frame (same stream), then the wavefront loop.
// No exchange between devices.
int rt_backend_render_variants(rt_context* c, int w, int h, int spp, int bounces, int n_var,
                               const std::vector<RtMat>& tabs, int n_mats, int off, int stride, float* host_fb,
                               void* const* d_fbs)
{
    Group* g = grp(c);
    const int N = (int)g->dev.size();
    const int rows = (h - off + stride - 1) / stride;
    const size_t npx = (size_t)rows * w;
    if (npx > 0x7fffffff / 8) return rt_fail(c, RT_ERR_ARG, "render: too many pixels for one launch");
    std::vector<float> ms(N, 0.0f);
    // counters summed over every variant of every device (run_wave zeroes a device's per render)
    std::vector<std::vector<unsigned long long>> vsum(N, std::vector<unsigned long long>(2 * RT_STAT_COUNT, 0));
    const int r = rt_for_devices(c, N, [&](int d) -> int {
        Backend* b = g->dev[d];
        HIPCHK(c, hipSetDevice(b->device));
        hipStream_t s = b->own;
        if (int e = b->ev_done.sync(c)) return e;  // (the table and buffers are reused)
        if (int e = ensure(c, b->mats, (size_t)n_mats * sizeof(RtMat))) return e;
        b->view.mats = (const RtMat*)b->mats.p;
        b->view.n_mats = n_mats;
        if (host_fb)
            if (int e = ensure(c, b->fb, npx * sizeof(float4_))) return e;
        HIPCHK(c, hipEventRecord(b->ev0, s));
        for (int v = d; v < n_var; v += N) {
            const RtMat* tab = tabs.data() + (size_t)v * n_mats;
            b->bl_rays = rt_table_has_emissive_prim(c, tab) ? 1 : 0;
            // (pageable source: the copy is staged before the call returns, and ordered on s
            // after the previous variant's frame, whose lanes joined back into s)
            HIPCHK(c, hipMemcpyAsync(b->mats.p, tab, (size_t)n_mats * sizeof(RtMat), hipMemcpyHostToDevice, s));
            float4_* fb = host_fb ? (float4_*)b->fb.p : (float4_*)d_fbs[v];
            if (host_fb)
                HIPCHK(c, hipMemcpyAsync(fb, host_fb + 4 * npx * v, npx * sizeof(float4_), hipMemcpyHostToDevice, s));
            const rtk::PixSrc src{w, off, stride, nullptr};
            if (int e = run_wave(c, b, w, h, spp, bounces, src, (int)npx, fb, s)) return e;
            if (host_fb)
                HIPCHK(c, hipMemcpyAsync(host_fb + 4 * npx * v, fb, npx * sizeof(float4_), hipMemcpyDeviceToHost, s));
            if (c->stats_enabled) {  // (diagnostic renders: this variant's counters, before the next zeroes them)
                unsigned long long one[2 * RT_STAT_COUNT];
                HIPCHK(c, hipMemcpyAsync(one, b->stats.p, sizeof one, hipMemcpyDeviceToHost, s));
                HIPCHK(c, hipStreamSynchronize(s));
                for (int i = 0; i < 2 * RT_STAT_COUNT; i++) vsum[d][i] += one[i];
            }
        }
        HIPCHK(c, hipEventRecord(b->ev1, s));
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipEventElapsedTime(&ms[d], b->ev0, b->ev1));
        return 0;
    });
    // the bound table comes back with the next render's upload (rt_render_variants marks it)
    for (Backend* b : g->dev) b->bl_rays = rt_scene_has_emissive_prim(c) ? 1 : 0;
    HIPCHK(c, hipSetDevice(be(c)->device));
    if (r) return r;
    c->last_kernel_ms = *std::max_element(ms.begin(), ms.end());
    if (c->stats_enabled)  // every variant of every device, summed
        for (int i = 0; i < 2 * RT_STAT_COUNT; i++) {
            c->stats[i] = 0;
            for (int d = 0; d < N; d++) c->stats[i] += vsum[d][i];
        }
    return RT_OK;
}

// One device's share of a pixel list (host buffers in and out).
static int render_pixels_one(rt_context* c, Backend* b, int w, int h, int spp, int bounces, const int* xy, int n,
                             float* rgba, float* ms_out)
{
    StagedCall st;
    if (int r = st.enter(c, b, false, nullptr, b->own)) return r;
    if (n == 0) return RT_OK;
    const size_t bxy = (size_t)n * 8, brgba = (size_t)n * 16;
    hipStream_t s = st.s;
    if (int r = ensure(c, b->xy, bxy)) return r;  // (the list: a buffer of its own beside the staged pixels)
    if (int r = st.staging(b->fb, brgba)) return r;
    HIPCHK(c, hipMemcpyAsync(b->xy.p, xy, bxy, hipMemcpyHostToDevice, s));
    float4_* fb = (float4_*)st.inout(rgba, rgba, brgba);
    if (c->stats_enabled) HIPCHK(c, hipMemsetAsync(b->stats.p, 0, b->stats.bytes, s));
    rtk::PixSrc src{w, 0, 1, (const int32_t*)b->xy.p};
    if (int r = st.begin()) return r;
    if (int r = run_wave(c, b, w, h, spp, bounces, src, n, fb, s)) return r;
    return st.end(nullptr, ms_out);
}

int rt_backend_render_pixels(rt_context* c, int w, int h, int spp, int bounces, const int* xy, int n, float* rgba)
{
    Group* g = grp(c);
    const int N = (int)g->dev.size();
    if (N == 1) {
        float ms = 0;
        if (int r = render_pixels_one(c, g->dev[0], w, h, spp, bounces, xy, n, rgba, &ms)) return r;
        c->last_kernel_ms = ms;
        return finish_stats(c, g->dev[0], g->dev[0]->own);
    }
    // pixel i -> device i mod N (pixels are independent); host-side split and merge
    std::vector<std::vector<int>> pxy(N);
    std::vector<std::vector<float>> prgba(N);
    for (int i = 0; i < n; i++) {
        pxy[i % N].push_back(xy[2 * i]);
        pxy[i % N].push_back(xy[2 * i + 1]);
        prgba[i % N].insert(prgba[i % N].end(), rgba + 4 * (size_t)i, rgba + 4 * (size_t)i + 4);
    }
    std::vector<int> rc(N, RT_OK);
    std::vector<float> ms(N, 0.0f);
    {
        std::vector<std::thread> th;
        for (int d = 0; d < N; d++)
            th.emplace_back([&, d] {
                rc[d] = render_pixels_one(c, g->dev[d], w, h, spp, bounces, pxy[d].data(), (int)pxy[d].size() / 2,
                                          prgba[d].data(), &ms[d]);
            });
        for (auto& t : th) t.join();
    }
    for (int d = 0; d < N; d++)
        if (rc[d]) return rc[d];
    for (int i = 0; i < n; i++) std::memcpy(rgba + 4 * (size_t)i, &prgba[i % N][4 * (size_t)(i / N)], 16);
    c->last_kernel_ms = *std::max_element(ms.begin(), ms.end());
    if (c->stats_enabled) {
        unsigned long long sum[2 * RT_STAT_COUNT] = {};
        for (int d = 0; d < N; d++) {
            if (int r = finish_stats(c, g->dev[d], g->dev[d]->own)) return r;
            for (int i = 0; i < 2 * RT_STAT_COUNT; i++) sum[i] += c->stats[i];
        }
        std::memcpy(c->stats, sum, sizeof sum);
    }
    return RT_OK;
}

// ---- progressions (rt_progress_*): the base values and the paused state live in buffers of
// their own on the context's device; a pass is run_wave with a WavePass (no k_tonemap), a
// resolve is k_resolve (linear: rt_display.hip's k_resolve_linear) over base and state.
// Single-device contexts (rt_capi_host.cpp).
namespace {
// the passes (ev_done) and device resolves (ev_pg) still in flight have finished with the buffers
int progress_quiesce(rt_context* c, Backend* b)
{
    if (int r = b->ev_done.sync(c)) return r;
    return b->ev_pg.sync(c);
}
void release(DevBuf& d)
{
    if (d.p) (void)hipFree(d.p);
    d.p = nullptr;
    d.bytes = 0;
}
}  // namespace

int rt_backend_progress_begin(rt_context* c, const float* base, const float* state)
{
    Backend* b = be(c);
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    if (int r = progress_quiesce(c, b)) return r;
    const size_t n = c->prog.npx(), bytes = n * sizeof(float4_);
    if (int r = ensure(c, b->pg_base, bytes)) return r;
    if (int r = ensure(c, b->pg_state, bytes)) return r;
    if (!b->ev_pg.ev) HIPCHK(c, hipEventCreateWithFlags(&b->ev_pg.ev.h, hipEventDisableTiming));
    if (base) {
        HIPCHK(c, hipMemcpy(b->pg_base.p, base, bytes, hipMemcpyHostToDevice));
    } else {
        const std::vector<float4_> one(n, float4_{0.0f, 0.0f, 0.0f, 1.0f});
        HIPCHK(c, hipMemcpy(b->pg_base.p, one.data(), bytes, hipMemcpyHostToDevice));
    }
    if (state) HIPCHK(c, hipMemcpy(b->pg_state.p, state, bytes, hipMemcpyHostToDevice));
    else HIPCHK(c, hipMemset(b->pg_state.p, 0, bytes));
    HIPCHK(c, hipDeviceSynchronize());  // (a pass may start on any stream)
    return RT_OK;
}

int rt_backend_progress_advance(rt_context* c, int first, int stop, void* stream)
{
    Backend* b = be(c);
    const RtProgress& P = c->prog;
    HIPCHK(c, hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    if (int r = b->ev_pg.wait(c, s)) return r;  // (a device resolve still reads the state)
    const rtk::PixSrc src{P.w, P.off, P.stride, nullptr};
    // (the framebuffer pointer of the pass is never used: it names the state, valid memory of the same size)
    const WavePass pass{(float4_*)b->pg_state.p, first, P.total};
    // a tracked progression's A pass: half -= state ahead of it and half += state behind it, on its stream
    const bool fold = P.next_is_a();
    HIPCHK(c, hipEventRecord(b->ev0, s));
    if (fold) {
        if (int r = b->ev_done.wait(c, s)) return r;  // (the last pass wrote the state)
        if (int r = rt_noise_fold(c, (float4_*)b->pg_half.p, pass.state, (int)P.npx(), false, s)) return r;
    }
    if (int r = run_wave(c, b, P.w, P.h, stop, P.bounces, src, (int)P.npx(), pass.state, s, &pass)) return r;
    if (fold) {
        if (int r = rt_noise_fold(c, (float4_*)b->pg_half.p, pass.state, (int)P.npx(), true, s)) return r;
        if (int r = b->ev_done.record(c, s)) return r;  // (resolves, queries and the next pass wait for the fold too)
    }
    HIPCHK(c, hipEventRecord(b->ev1, s));
    c->last_kernel_ms = -1.0;  // (a device call: StagedCall's convention)
    return finish_stats(c, b, s);
}

int rt_backend_progress_resolve(rt_context* c, float* host_fb, void* dev_fb, void* stream, bool linear)
{
    Backend* b = be(c);
    const RtProgress& P = c->prog;
    StagedCall st;
    if (int r = st.enter(c, b, host_fb == nullptr, stream, b->own)) return r;
    const int n = (int)P.npx();
    hipStream_t s = st.s;
    if (int r = st.staging(b->pg_out, (size_t)n * sizeof(float4_))) return r;
    float4_* out = (float4_*)st.out(host_fb ? (void*)host_fb : dev_fb, (size_t)n * sizeof(float4_));
    if (int r = b->ev_done.wait(c, s)) return r;  // (the last pass, on its own streams)
    const float4_ *base = (const float4_*)b->pg_base.p, *state = (const float4_*)b->pg_state.p;
    if (int r = st.begin()) return r;
    if (P.adaptive) {  // (the pixel's tile count for `done`: rt_adapt.hip)
        if (int r = rt_adapt_resolve(c, b, base, state, out, linear, s)) return r;
    } else if (int r = linear ? rt_display_resolve_linear(c, base, state, out, n, P.done, s)
                              : rt_wave_resolve(c, base, state, out, n, P.done, s))
        return r;
    return st.end(&b->ev_pg);  // (device form: the next pass writes the state this reads)
}

int rt_backend_progress_read(rt_context* c, float* base, float* state)
{
    Backend* b = be(c);
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    if (int r = progress_quiesce(c, b)) return r;
    const size_t bytes = c->prog.npx() * sizeof(float4_);
    HIPCHK(c, hipMemcpy(base, b->pg_base.p, bytes, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(state, b->pg_state.p, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

void rt_backend_progress_end(rt_context* c)
{
    if (!c->backend) return;
    Backend* b = be(c);
    DeviceScope sc;
    if (sc.enter(c, b->device)) return;
    (void)progress_quiesce(c, b);
    release(b->pg_base);
    release(b->pg_state);
    release(b->pg_out);
    release(b->pg_half);
    release(b->pg_noise);
    b->adapt.reset();
}

int rt_backend_progress_track(rt_context* c, const float* half)
{
    Backend* b = be(c);
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    if (int r = progress_quiesce(c, b)) return r;
    const size_t bytes = c->prog.npx() * sizeof(float4_);
    if (int r = ensure(c, b->pg_half, bytes)) return r;
    if (half) HIPCHK(c, hipMemcpy(b->pg_half.p, half, bytes, hipMemcpyHostToDevice));
    else HIPCHK(c, hipMemset(b->pg_half.p, 0, bytes));
    HIPCHK(c, hipDeviceSynchronize());  // (a pass may start on any stream)
    return RT_OK;
}

int rt_backend_progress_read_half(rt_context* c, float* half)
{
    Backend* b = be(c);
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    if (int r = progress_quiesce(c, b)) return r;
    HIPCHK(c, hipMemcpy(half, b->pg_half.p, c->prog.npx() * sizeof(float4_), hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- adaptive progressions (rt_adapt.h): the stages are rt_adapt.hip's, the pass is run_wave over
// the compact pixel list with the compact state as its WavePass.
int rt_backend_progress_adapt_begin(rt_context* c, const int32_t* tile_n, const int32_t* tile_nA)
{
    Backend* b = be(c);
    const RtProgress& P = c->prog;
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    if (int r = progress_quiesce(c, b)) return r;
    if (!b->adapt) b->adapt.reset(new Adapt);
    const size_t n_tiles = (size_t)P.tiles_w() * P.tiles_h();
    if (int r = ensure(c, b->adapt->tile_n, 4 * n_tiles)) return r;
    if (int r = ensure(c, b->adapt->tile_nA, 4 * n_tiles)) return r;
    const std::vector<int32_t> n(n_tiles, P.done), na(n_tiles, P.n_a);
    HIPCHK(c, hipMemcpy(b->adapt->tile_n.p, tile_n ? tile_n : n.data(), 4 * n_tiles, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(b->adapt->tile_nA.p, tile_nA ? tile_nA : na.data(), 4 * n_tiles, hipMemcpyHostToDevice));
    HIPCHK(c, hipDeviceSynchronize());  // (a pass may start on any stream)
    return RT_OK;
}

int rt_backend_progress_adapt_bump(rt_context* c, int samples, bool a_pass, void* stream)
{
    Backend* b = be(c);
    HIPCHK(c, hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    // Behind the uniform pass on its stream (which waited for ev_pg and ev_done); ev_done is recorded again
    // behind the bump, so resolves, queries and the next pass wait for the counts too.
    if (int r = rt_adapt_bump(c, b, samples, a_pass, s)) return r;
    return b->ev_done.record(c, s);
}

int rt_backend_progress_adapt_advance(rt_context* c, int samples, float threshold, void* stream, int32_t* hdr)
{
    Backend* b = be(c);
    const RtProgress& P = c->prog;
    HIPCHK(c, hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    if (int r = progress_quiesce(c, b)) return r;  // (the host sizes the launch: nothing of the progression in flight)
    Adapt& ad = *b->adapt;
    const bool a_pass = P.next_is_a();
    if (int r = rt_adapt_select(c, b, samples, threshold, P.passes >= 2, a_pass, hdr, s)) return r;
    const int n_act = hdr[rtk::AD_TILES_ACTIVE], n = hdr[rtk::AD_PIXELS];
    c->last_kernel_ms = -1.0;
    if (n_act == 0) return RT_OK;
    if (int r = ensure(c, ad.xy, 8 * (size_t)n)) return r;
    if (int r = ensure(c, ad.idx, 4 * (size_t)n)) return r;
    if (int r = ensure(c, ad.cstate, 16 * (size_t)n)) return r;
    HIPCHK(c, hipEventRecord(b->ev0, s));
    if (int r = rt_adapt_gather(c, b, n_act, a_pass, s)) return r;
    // Slot i of the list is its own pixel: fb_at is the identity for a list, and run_wave offsets the
    // list, the framebuffer and the pass's state by a lane's first slot alike. The sample index is a
    // counter only (the seed takes seed_spp), so pixels at different counts run as samples 1 .. samples.
    // Only a pixel without a sample has no state to go on from: it starts at 0 (k_init seeds its chain), and
    // the counts are then all 0 (rt_progress_load refuses a mix of zero and positive counts).
    const int first = P.tile_max == 0 ? 0 : 1;
    const rtk::PixSrc src{P.w, 0, 1, (const int32_t*)ad.xy.p};
    const WavePass pass{(float4_*)ad.cstate.p, first, P.total};
    if (int r = run_wave(c, b, P.w, P.h, first + samples, P.bounces, src, n, pass.state, s, &pass)) return r;
    if (int r = rt_adapt_scatter(c, b, n, a_pass, s)) return r;
    if (int r = b->ev_done.record(c, s)) return r;  // (resolves, queries and the next pass wait for the scatter too)
    HIPCHK(c, hipEventRecord(b->ev1, s));
    return finish_stats(c, b, s);
}

int rt_backend_progress_adapt_counts(rt_context* c, int32_t* tile_n, int32_t* tile_nA)
{
    Backend* b = be(c);
    DeviceScope sc;
    if (int r = sc.enter(c, b->device)) return r;
    if (int r = progress_quiesce(c, b)) return r;
    const size_t bytes = 4 * (size_t)c->prog.tiles_w() * c->prog.tiles_h();
    if (tile_n) HIPCHK(c, hipMemcpy(tile_n, b->adapt->tile_n.p, bytes, hipMemcpyDeviceToHost));
    if (tile_nA) HIPCHK(c, hipMemcpy(tile_nA, b->adapt->tile_nA.p, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

Backend* rt_backend_dev0(rt_context* c) { return be(c); }

// Time between the events around the last rt_render_device launch sequence
// (recorded on its stream); call after synchronizing that stream.
extern "C" double rt_device_last_kernel_ms(rt_context* c)
{
    if (!c || !c->backend) return -1.0;
    Backend* b = be(c);
    float ms = 0;
    if (hipEventSynchronize(b->ev1) != hipSuccess) return -1.0;
    if (hipEventElapsedTime(&ms, b->ev0, b->ev1) != hipSuccess) return -1.0;
    c->last_kernel_ms = ms;
    return ms;
}

// Iterations the last wavefront render took.
extern "C" int rt_device_last_iterations(rt_context* c) { return c && c->backend ? be(c)->last_iters : -1; }

// Queries k_trace handed to the exact octree walk (ties, failed verifications, stack
// overflows, far origins, the force_fallback stressor) in every render on every device of
// the context since the last reset: the walks' health figure (~2e-6 per sample on cfg2).
// Waits for the devices.
extern "C" int rt_device_exact_handovers(rt_context* c, unsigned long long* out, int reset)
{
    if (!c || !c->backend || !out) return rt_fail(c, RT_ERR_ARG, "rt_device_exact_handovers: no context or no output");
    unsigned long long sum = 0;
    DeviceScope sc;  // (the caller's device is current again on every return)
    for (Backend* b : grp(c)->dev) {
        if (int r = sc.enter(c, b->device)) return r;
        HIPCHK(c, hipDeviceSynchronize());
        if (!b->handovers.p) continue;
        unsigned long long v = 0;
        HIPCHK(c, hipMemcpy(&v, b->handovers.p, 8, hipMemcpyDeviceToHost));
        sum += v;
        if (reset) HIPCHK(c, hipMemset(b->handovers.p, 0, 8));
    }
    *out = sum;
    return RT_OK;
}

// Per-kernel-class timing (k_trace, k_step, k_tail) over the renders since it
// was enabled, summed over the context's devices: out_ms[3] total ms (HIP events
// around every launch on its lane's stream), out_launches[3].
extern "C" int rt_device_kernel_timing(rt_context* c, int enable, double* out_ms, long* out_launches)
{
    if (!c || !c->backend) return RT_ERR_ARG;
    Group* g = grp(c);
    for (int k = 0; k < 3; k++) {
        double ms = 0;
        long n = 0;
        for (Backend* b : g->dev) ms += b->kms[k], n += b->klaunch[k];
        if (out_ms) out_ms[k] = ms;
        if (out_launches) out_launches[k] = n;
    }
    if (enable >= 0)
        for (Backend* b : g->dev) {
            b->timing = enable != 0;
            for (int k = 0; k < 3; k++) b->kms[k] = 0, b->klaunch[k] = 0;
        }
    return RT_OK;
}

// Wavefront lanes (streams) per render on every device of the context (RT_LANES at
// creation; 1 serializes a render's launches, for per-launch kernel timing; 0: auto).
extern "C" int rt_device_set_lanes(rt_context* c, int lanes)
{
    if (!c || !c->backend || lanes < 0) return RT_ERR_ARG;
    for (Backend* b : grp(c)->dev) b->lanes = std::min(RT_MAX_LANES, lanes);
    return RT_OK;
}

#ifndef RT_BUILD_SRC
#define RT_BUILD_SRC "unknown"
#endif
#ifndef RT_BUILD_DEFS
#define RT_BUILD_DEFS ""
#endif
extern "C" const char* rt_build_id(void) { return "src=" RT_BUILD_SRC " defs=" RT_BUILD_DEFS " (gfx950)"; }
