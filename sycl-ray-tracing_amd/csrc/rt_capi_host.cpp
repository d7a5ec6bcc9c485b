// rt_capi_host.cpp — the backend-independent half of the C ABI
// (include/rt_hip.h): argument checking, host scene preparation, host
// helpers: contexts, scene / BVH / env / camera, renders, queries, progressions,
// stats, mesh and image helpers. The frame stages are rt_capi_stages.cpp. The
// compute half lives in rt_render.hip (gfx950).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "rt_adapt.h"
#include "rt_context.h"
#include "rt_noise.h"

namespace {
std::mutex g_err_mu;
std::string g_err;
thread_local std::string* tl_sink = nullptr;  // rt_err_sink
void set_global_err(const std::string& m)
{
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_err = m;
}
}  // namespace

void rt_err_sink(std::string* sink) { tl_sink = sink; }

// A rebind ends the context's progression (rt_progress_*): its state was computed under the old binding.
static void progress_drop(rt_context* c)
{
    if (!c || !c->prog.active) return;
    rt_backend_progress_end(c);
    c->prog = RtProgress{};
}

void rt_read_diag(rt_context* c)
{
    if (const char* e = std::getenv("RT_TIMELINE")) c->diag.timeline = e;
    if (const char* e = std::getenv("RT_ITER_LOG")) c->diag.iter_log = e;
    c->diag.verbose = std::getenv("RT_VERBOSE") != nullptr;
}

int rt_fail(rt_context* ctx, int code, const std::string& msg)
{
    if (tl_sink) {  // a device thread of a multi-device render: its own slot (rt_for_devices)
        *tl_sink = msg;
        return code;
    }
    if (ctx) {
        std::lock_guard<std::mutex> lk(g_err_mu);
        ctx->err = msg;
    }
    set_global_err(msg);
    return code;
}

// One material of the C ABI (10 floats: emission rgba, diffuse rgba, metalness, roughness) as the device's record.
static RtMat unpack_mat(const float* p) { return RtMat{p[0], p[1], p[2], p[8], p[4], p[5], p[6], p[9]}; }

// The tail of rt_create*: the backend for a filled-in context, which is destroyed if that fails.
static int create_finish(rt_context* c, rt_context** out)
{
    rt_read_diag(c);
    int r = rt_backend_create(c);
    if (r) {
        set_global_err(c->err);
        rt_backend_destroy(c);
        delete c;
        return r;
    }
    *out = c;
    return RT_OK;
}

// (rt_context.h) mats_too: rt_set_materials, rt_render_variants
static void placeholder_env(rt_context* c);
int rt_tables_current(rt_context* c, bool mats_too, bool env_stub)
{
    if (!c->dirty && !(mats_too && c->mats_dirty_only)) return RT_OK;
    if (env_stub) placeholder_env(c);
    if (int r = rt_backend_upload(c)) return r;
    c->dirty = false;
    c->mats_dirty_only = false;
    return RT_OK;
}

RtSceneView rt_host_view(const rt_context* c)
{
    RtSceneView v{};
    rt_view_scalars(c, v);
    rt_scene_tables(c, v, [](const auto& table, auto& field) { field = table.data(); });
    v.tri4 = c->flat.tri4.data();
    v.mats = c->mats.data();
    if (c->cdf_fence.empty()) v.cdf_fence = nullptr;
    v.tri_mat = 0;
    return v;
}

void rt_view_scalars(const rt_context* c, RtSceneView& v)
{
    v.n_mats = (int)c->mats.size();
    v.cdf_cw = c->cdf_cw;
    v.cdf_total = c->cdf.empty() ? 0.0f : c->cdf.back();
    v.n_emissive = (int)c->emissive.size();
    v.n_spheres = (int)(c->spheres.size() / 2);
    v.ew = c->ew;
    v.eh = c->eh;
    v.n_tris = (int)(c->tris.size() / 9);
    v.chain_monotone = rt_view_chain_monotone(c);
    v.brute = c->brute ? 1 : 0;
    rt_view_near(c, v);
}

int rt_view_chain_monotone(const rt_context* c) { return c->flat.chain_monotone && !c->sched.chain_full ? 1 : 0; }

void rt_view_near(const rt_context* c, RtSceneView& v)
{
    const double scale = c->sched.near_scale >= 0.0 ? c->sched.near_scale : RT_NEAR_SCALE;
    // the scene's box: the octree root's axis planes (PLANE_NORMALS 0-2 are the axes: the
    // vertices' min / max) and every analytic sphere's box
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, ext = 0.0;
    if (!c->flat.nodes.empty())
        for (int i = 0; i < 3; i++) lo[i] = c->flat.nodes[0].dn[i], hi[i] = c->flat.nodes[0].df[i];
    for (size_t k = 0; k + 1 < c->spheres.size(); k += 2) {
        const float4_& sp = c->spheres[k];
        const double cc[3] = {sp.x, sp.y, sp.z}, r = std::fabs((double)sp.w);
        for (int i = 0; i < 3; i++) lo[i] = std::min(lo[i], cc[i] - r), hi[i] = std::max(hi[i], cc[i] + r);
    }
    bool have = true;
    for (int i = 0; i < 3; i++) {
        if (!(lo[i] <= hi[i]) || !std::isfinite(lo[i]) || !std::isfinite(hi[i])) have = false;
        else ext = std::max(ext, hi[i] - lo[i]);
    }
    for (int i = 0; i < 3; i++) {
        const double w = have ? scale * ext : 0.0;
        // rounded outwards; beyond float range (or no scene): unbounded
        v.near_lo[i] = have ? std::nextafter((float)(lo[i] - w), -INFINITY) : -INFINITY;
        v.near_hi[i] = have ? std::nextafter((float)(hi[i] + w), INFINITY) : INFINITY;
    }
}

bool rt_table_has_emissive_prim(const rt_context* c, const RtMat* table)
{
    for (int32_t mi : c->mat_idx) {
        const RtMat& m = table[mi];
        if (m.er > 0 || m.eg > 0 || m.eb > 0) return true;
    }
    return false;
}

bool rt_scene_has_emissive_prim(const rt_context* c) { return rt_table_has_emissive_prim(c, c->mats.data()); }

extern "C" {

int rt_version(void) { return 10002; }

const char* rt_last_error(const rt_context* ctx)
{
    if (ctx) return ctx->err.c_str();
    std::lock_guard<std::mutex> lk(g_err_mu);
    static thread_local std::string copy;
    copy = g_err;
    return copy.c_str();
}

int rt_create(int device, rt_context** out)
{
    if (!out) return rt_fail(nullptr, RT_ERR_ARG, "rt_create: out is NULL");
    *out = nullptr;
    rt_context* c = new rt_context();
    c->device = device;
    return create_finish(c, out);
}

}  // extern "C"

namespace {
// ids: non-negative and distinct (one rank per GPU in the RCCL clique); the range is
// checked against the devices present when the backend opens them (RT_ERR_NODEV).
// loopback (rt_create_multi_loopback, tests only) admits a list that names a GPU more
// than once: the context then exchanges the shards with device copies instead of RCCL.
// rccl (rt_test_create_multi_rccl, tests only): the multi-device driver and its RCCL clique
// even for one listed device (a one-rank ncclCommInitAll), so a one-GPU box runs the pack,
// ncclScatter, render, ncclGather and un-permute sequence the 8-GPU node runs.
int create_multi(int n_devices, const int* devices, bool loopback, rt_context** out, bool rccl = false)
{
    if (!out) return rt_fail(nullptr, RT_ERR_ARG, "rt_create_multi: out is NULL");
    *out = nullptr;
    if (n_devices < 1 || n_devices > 64) return rt_fail(nullptr, RT_ERR_ARG, "rt_create_multi: n_devices must be 1..64");
    for (int d = 0; d < n_devices; d++) {
        const int id = devices ? devices[d] : d;
        if (id < 0) return rt_fail(nullptr, RT_ERR_ARG, "rt_create_multi: negative device id");
        for (int e = 0; e < d; e++)
            if ((devices ? devices[e] : e) == id && !loopback)
                return rt_fail(nullptr, RT_ERR_ARG, "rt_create_multi: device " + std::to_string(id) + " listed twice");
    }
    rt_context* c = new rt_context();
    for (int d = 0; d < n_devices; d++) c->devices.push_back(devices ? devices[d] : d);
    c->device = c->devices[0];
    c->loopback = loopback;
    c->force_multi = rccl;
    return create_finish(c, out);
}
}  // namespace

extern "C" {
int rt_create_multi(int n_devices, const int* devices, rt_context** out)
{
    return create_multi(n_devices, devices, false, out);
}

int rt_create_multi_loopback(int n_devices, const int* devices, rt_context** out)
{
    return create_multi(n_devices, devices, true, out);
}

int rt_test_create_multi_rccl(int n_devices, const int* devices, rt_context** out)
{
    return create_multi(n_devices, devices, false, out, true);
}

int rt_test_fail_device(rt_context* c, int device)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "rt_test_fail_device: ctx is NULL");
    c->fail_device = device;
    return RT_OK;
}

int rt_test_schedule(rt_context* c, const char* key, double value)
{
    if (!c || !key) return rt_fail(c, RT_ERR_ARG, "rt_test_schedule: ctx or key is NULL");
    RtSchedule& s = c->sched;
    const std::string k = key;
    // (finite for every key; in int range for the integer ones: the cast is otherwise undefined)
    const bool real_key = k == "tail_enter" || k == "fast_spp" || k == "near_scale";
    if (!std::isfinite(value) || (!real_key && (value < -2147483648.0 || value > 2147483647.0)))
        return rt_fail(c, RT_ERR_ARG, "rt_test_schedule: value of " + k + " is out of range");
    const int v = real_key ? 0 : (int)value;
    for (const auto& e : rt_variant_keys)
        if (k == e.key) {
            s.variant[e.slot] = std::max(0, std::min(2, v));
            return RT_OK;
        }
    if (k == "lanes") s.lanes = std::max(0, v);
    else if (k == "tail_paths") s.tail_paths = v;
    else if (k == "tail_enter") s.tail_enter = value;
    else if (k == "tail_rows") s.tail_rows = v;
    else if (k == "drain_rows") s.drain_rows = std::min(4, v);
    else if (k == "heavy_calls") s.heavy_calls = v;
    else if (k == "spec_cam") s.spec_cam = std::min(2, v);
    else if (k == "tail_spec_cam") s.tail_spec_cam = std::min(2, v);
    else if (k == "force_fallback") s.force_fallback = std::max(0, v);
    else if (k == "step_budget") s.step_budget = v;
    else if (k == "fast_k") s.fast_k = v;
    else if (k == "fast_spp") s.fast_spp = value;
    else if (k == "near_scale") s.near_scale = value;
    else if (k == "mt_blocks") s.mt_blocks = std::max(0, std::min(65536, v));
    else if (k == "gb_force_every") s.gb_force_every = std::max(0, v);
    else if (k == "chain_full") {
        // the devices' views carry the flag: the next call uploads them again
        if (s.chain_full != (v != 0)) c->dirty = true;
        s.chain_full = v != 0;
    } else if (k == "reset") {
        if (s.chain_full) c->dirty = true;
        s = RtSchedule{};
    }
    else return rt_fail(c, RT_ERR_ARG, "rt_test_schedule: unknown key " + k);
    return RT_OK;
}

int rt_test_obj_parallel_min(long bytes)
{
    rt::g_obj_parallel_min.store(bytes < 0 ? -1 : bytes);
    return RT_OK;
}

int rt_test_walk_log(rt_context* c, int min_calls, int sample_every, int capacity)
{
    if (!c || min_calls < 0 || capacity < 0) return rt_fail(c, RT_ERR_ARG, "rt_test_walk_log: bad arguments");
    c->diag.wlog_min = min_calls;
    c->diag.wlog_every = sample_every < 0 ? -1 : std::max(1, sample_every);
    c->diag.wlog_cap = min_calls > 0 ? capacity : 0;
    c->diag.wlog.clear();
    c->diag.wlog_total = 0;
    return RT_OK;
}

long rt_test_walk_log_read(const rt_context* c, float* out, long capacity)
{
    if (!c || capacity < 0 || (capacity > 0 && !out)) return rt_fail(nullptr, RT_ERR_ARG, "rt_test_walk_log_read: bad arguments");
    const long n = (long)(c->diag.wlog.size() / RT_WLOG_FLOATS);
    const long m = std::min(n, capacity);
    if (m > 0) std::memcpy(out, c->diag.wlog.data(), (size_t)m * RT_WLOG_FLOATS * sizeof(float));
    return c->diag.wlog_total;
}

int rt_device_count(const rt_context* ctx) { return ctx ? (ctx->devices.empty() ? 1 : (int)ctx->devices.size()) : RT_ERR_ARG; }

void rt_destroy(rt_context* ctx)
{
    if (!ctx) return;
    rt_backend_destroy(ctx);
    delete ctx;
}

int rt_set_scene(rt_context* c, const float* triangles, int n, const int* material_indices, int n_mi,
                 const float* materials, int n_mats, const int* emissive, int n_em, const float* spheres, int n_sph)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "rt_set_scene: ctx is NULL");
    progress_drop(c);
    if (n < 0 || (n > 0 && !triangles) || n_mats <= 0 || !materials || n_mi < n || (n_mi > 0 && !material_indices) ||
        n_em < 0 || (n_em > 0 && !emissive) || n_sph < 0 || (n_sph > 0 && !spheres))
        return rt_fail(c, RT_ERR_ARG, "rt_set_scene: bad buffer sizes");
    for (int i = 0; i < n_mi; i++)
        if (material_indices[i] < 0 || material_indices[i] >= n_mats)
            return rt_fail(c, RT_ERR_ARG, "rt_set_scene: material index out of range");
    for (int i = 0; i < n_em; i++)
        if (emissive[i] < 0 || emissive[i] >= n) return rt_fail(c, RT_ERR_ARG, "rt_set_scene: emissive id out of range");
    for (int i = 0; i < n_sph; i++) {
        const int prim = (int)spheres[5 * i + 4];
        if (prim < 0 || prim >= n_mi)
            return rt_fail(c, RT_ERR_ARG, "rt_set_scene: sphere primitive index has no material index");
    }
    c->tris.assign(triangles, triangles + 9 * (size_t)n);
    c->mat_idx.assign(material_indices, material_indices + n_mi);
    c->mats.resize(n_mats);
    for (int i = 0; i < n_mats; i++) c->mats[i] = unpack_mat(materials + 10 * (size_t)i);
    c->emissive.assign(emissive, emissive + n_em);
    c->spheres.clear();
    for (int i = 0; i < n_sph; i++) {
        const float* p = spheres + 5 * (size_t)i;
        float4_ a{p[0], p[1], p[2], p[3]}, b{0, 0, 0, 0};
        const int prim = (int)p[4];
        std::memcpy(&b.x, &prim, 4);
        c->spheres.push_back(a);
        c->spheres.push_back(b);
    }
    c->have_scene = true;
    c->have_bvh = false;
    c->dirty = true;
    return RT_OK;
}

int rt_set_materials(rt_context* c, const float* materials, int n_mats)
{
    progress_drop(c);
    if (!c || !c->have_scene) return rt_fail(c, RT_ERR_STATE, "rt_set_materials: no scene");
    if (n_mats <= 0 || !materials) return rt_fail(c, RT_ERR_ARG, "rt_set_materials: bad buffer");
    for (int32_t mi : c->mat_idx)
        if (mi >= n_mats) return rt_fail(c, RT_ERR_ARG, "rt_set_materials: a material index is out of range");
    c->mats.resize(n_mats);
    for (int i = 0; i < n_mats; i++) c->mats[i] = unpack_mat(materials + 10 * (size_t)i);
    c->mats_dirty_only = true;  // the octree, search BVH, triangles and env stay on the device
    return RT_OK;
}

int rt_build_bvh(rt_context* c, int max_depth, int leaf_max)
{
    progress_drop(c);
    if (!c || !c->have_scene) return rt_fail(c, RT_ERR_STATE, "rt_build_bvh: no scene");
    if (max_depth > 32 || max_depth < -1 || leaf_max < 1)
        return rt_fail(c, RT_ERR_ARG, "rt_build_bvh: max_depth must be -1..32 (device stack bound), leaf_max >= 1");
    const int n = (int)(c->tris.size() / 9);
    rt::build_octree(c->tris.data(), n, max_depth, leaf_max, c->octree);
    rt::flatten_octree(c->octree, c->tris.data(), n, c->flat);
    if (c->flat.max_depth > 32) return rt_fail(c, RT_ERR_ARG, "rt_build_bvh: octree deeper than 32");
    rt::build_search_bvh(c->flat);
    c->have_bvh = true;
    c->dirty = true;
    return RT_OK;
}

int rt_set_bvh_preorder(rt_context* c, const void* dump, long bytes)
{
    progress_drop(c);
    if (!c || !c->have_scene) return rt_fail(c, RT_ERR_STATE, "rt_set_bvh_preorder: no scene");
    if (!dump || bytes <= 0) return rt_fail(c, RT_ERR_ARG, "rt_set_bvh_preorder: empty dump");
    rt::Octree t;
    if (rt::octree_from_dump((const char*)dump, (size_t)bytes, t))
        return rt_fail(c, RT_ERR_ARG, "rt_set_bvh_preorder: malformed pre-order dump");
    const int n = (int)(c->tris.size() / 9);
    for (const auto& nd : t.pool)
        for (int id : nd.tris)
            if (id < 0 || id >= n) return rt_fail(c, RT_ERR_ARG, "rt_set_bvh_preorder: triangle id out of range");
    c->octree = std::move(t);
    rt::flatten_octree(c->octree, c->tris.data(), n, c->flat);
    if (c->flat.max_depth > 32) return rt_fail(c, RT_ERR_ARG, "rt_set_bvh_preorder: octree deeper than 32");
    rt::build_search_bvh(c->flat);
    c->have_bvh = true;
    c->dirty = true;
    return RT_OK;
}

long rt_bvh_dump(const rt_context* c, void* buf, long cap)
{
    if (!c || !c->have_bvh) return RT_ERR_STATE;
    std::vector<char> d = rt::dump_octree(c->octree);
    if (buf && cap >= (long)d.size()) std::memcpy(buf, d.data(), d.size());
    return (long)d.size();
}

int rt_bvh_info(const rt_context* c, long* info)
{
    if (!c || !c->have_bvh || !info) return RT_ERR_STATE;
    info[0] = (long)c->octree.pool.size();
    info[1] = (long)c->flat.nodes.size();
    info[2] = (long)(c->tris.size() / 9);
    info[3] = c->flat.max_depth;
    info[4] = (long)(c->flat.nodes.size() * sizeof(RtNode) + c->flat.tri4.size() * sizeof(float4_) +
                     c->flat.prim2k.size() * 4 + c->flat.parent.size() * 4 + c->flat.leaf_of.size() * 4 +
                     c->flat.bvh4.size() * sizeof(Bvh4Node) + c->flat.bvh_tri4.size() * sizeof(float4_));
    return RT_OK;
}

int rt_set_env(rt_context* c, const float* px, int w, int h, int ch, const float* cdf)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "rt_set_env: ctx is NULL");
    progress_drop(c);
    if (!px || w <= 0 || h <= 0 || (ch != 3 && ch != 4)) return rt_fail(c, RT_ERR_ARG, "rt_set_env: bad image");
    const size_t n = (size_t)w * h;
    c->ew = w;
    c->eh = h;
    c->env_lum.resize(n);
    c->cdf.resize(n);
    rt::env_luminance_cdf(px, w, h, ch, c->env_lum.data(), c->cdf.data());
    if (cdf) c->cdf.assign(cdf, cdf + n);
    // RGB + the texel's luminance in w: the env-map sample reads both with one 16-B load
    c->env.resize(n);
    for (size_t i = 0; i < n; i++) c->env[i] = float4_{px[ch * i], px[ch * i + 1], px[ch * i + 2], c->env_lum[i]};
    c->cdf_row.assign((size_t)((h + 15) & ~15), 0.0f);  // (padded: the fence search loads 16 at a time)
    for (int y = 0; y < h; y++) c->cdf_row[y] = c->cdf[(size_t)y * w + w - 1];
    rt::env_cdf_fences(c->cdf.data(), c->cdf_row.data(), w, h, c->cdf_fence);
    c->cdf_cw = w / 32;
    c->cdf_coarse.resize(std::max<size_t>(1, (size_t)h * c->cdf_cw));
    for (int y = 0; y < h; y++)
        for (int j = 0; j < c->cdf_cw; j++) c->cdf_coarse[(size_t)y * c->cdf_cw + j] = c->cdf[(size_t)y * w + 32 * j + 31];
    c->have_env = true;
    c->dirty = true;
    return RT_OK;
}

}  // extern "C"

// rt_intersect, rt_query and rt_render_features need no env, but the device view must be valid:
// a 1x1 black texel stands in. It is not the caller's env: have_env stays false, so a render
// still asks for one (check_ready), and a later rt_set_env replaces it.
static void placeholder_env(rt_context* c)
{
    if (c->have_env) return;
    const float z[3] = {0, 0, 0};
    rt_set_env(c, z, 1, 1, 3, nullptr);
    c->have_env = false;
}

extern "C" {

int rt_set_camera(rt_context* c, const float view[16], float fov_dist)
{
    progress_drop(c);
    if (!c || !view) return rt_fail(c, RT_ERR_ARG, "rt_set_camera: bad arguments");
    std::memcpy(c->cam.m, view, 64);
    c->cam.fov_dist = fov_dist;
    c->have_cam = true;
    return RT_OK;
}

static int check_ready(rt_context* c, int w, int h, int spp, int bounces)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "ctx is NULL");
    if (!c->have_scene || !c->have_bvh) return rt_fail(c, RT_ERR_STATE, "scene/BVH not set");
    if (!c->have_env) return rt_fail(c, RT_ERR_STATE, "environment map not set");
    if (!c->have_cam) return rt_fail(c, RT_ERR_STATE, "camera not set");
    if (w <= 0 || h <= 0 || spp <= 0 || bounces < 0) return rt_fail(c, RT_ERR_ARG, "bad render size");
    // the reference seeds with the int 31 + x*y*spp (render_kernel.cpp:77)
    if ((double)(w - 1) * (double)(h - 1) * (double)spp + 31.0 > 2147483647.0)
        return rt_fail(c, RT_ERR_ARG, "31 + x*y*spp overflows int (reference seed)");
    return rt_tables_current(c, true, false);
}

int rt_render(rt_context* c, int w, int h, int spp, int bounces, float* fb)
{
    if (int r = check_ready(c, w, h, spp, bounces)) return r;
    if (!fb) return rt_fail(c, RT_ERR_ARG, "rt_render: fb is NULL");
    return rt_backend_render(c, w, h, spp, bounces, fb, nullptr, 0, 1, nullptr);
}

int rt_render_device(rt_context* c, int w, int h, int spp, int bounces, void* d_fb, int row_offset, int row_stride,
                     void* stream)
{
    if (int r = check_ready(c, w, h, spp, bounces)) return r;
    if (!d_fb || row_stride <= 0 || row_offset < 0 || row_offset >= row_stride)
        return rt_fail(c, RT_ERR_ARG, "rt_render_device: bad shard");
    return rt_backend_render(c, w, h, spp, bounces, nullptr, d_fb, row_offset, row_stride, stream);
}

// rt_render / rt_render_device without the tone-map pass: the same checks, the same shards.
int rt_render_linear(rt_context* c, int w, int h, int spp, int bounces, float* fb)
{
    if (int r = check_ready(c, w, h, spp, bounces)) return r;
    if (!fb) return rt_fail(c, RT_ERR_ARG, "rt_render_linear: fb is NULL");
    return rt_backend_render(c, w, h, spp, bounces, fb, nullptr, 0, 1, nullptr, true);
}

int rt_render_linear_device(rt_context* c, int w, int h, int spp, int bounces, void* d_fb, int row_offset,
                            int row_stride, void* stream)
{
    if (int r = check_ready(c, w, h, spp, bounces)) return r;
    if (!d_fb || row_stride <= 0 || row_offset < 0 || row_offset >= row_stride)
        return rt_fail(c, RT_ERR_ARG, "rt_render_linear_device: bad shard");
    return rt_backend_render(c, w, h, spp, bounces, nullptr, d_fb, row_offset, row_stride, stream, true);
}

int rt_render_variants(rt_context* c, int w, int h, int spp, int bounces, int n_var, const float* materials,
                       int n_mats, int row_offset, int row_stride, float* fb, void* const* d_fbs)
{
    if (int r = check_ready(c, w, h, spp, bounces)) return r;
    if (n_var <= 0 || !materials || n_mats <= 0 || (fb == nullptr) == (d_fbs == nullptr))
        return rt_fail(c, RT_ERR_ARG, "rt_render_variants: bad buffers (exactly one of fb_rgba / d_fbs)");
    if (row_stride <= 0 || row_offset < 0 || row_offset >= row_stride)
        return rt_fail(c, RT_ERR_ARG, "rt_render_variants: bad row shard");
    for (int32_t mi : c->mat_idx)
        if (mi >= n_mats) return rt_fail(c, RT_ERR_ARG, "rt_render_variants: a material index is out of range");
    if (d_fbs)
        for (int v = 0; v < n_var; v++)
            if (!d_fbs[v]) return rt_fail(c, RT_ERR_ARG, "rt_render_variants: null device buffer");
    std::vector<RtMat> tabs((size_t)n_var * n_mats);
    for (size_t i = 0; i < tabs.size(); i++) tabs[i] = unpack_mat(materials + 10 * i);
    const int r = rt_backend_render_variants(c, w, h, spp, bounces, n_var, tabs, n_mats, row_offset, row_stride, fb, d_fbs);
    c->mats_dirty_only = true;  // the devices' tables hold the last variants: the next render re-sends the bound one
    return r;
}

int rt_render_pixels(rt_context* c, int w, int h, int spp, int bounces, const int* xy, int n, float* rgba)
{
    if (int r = check_ready(c, w, h, spp, bounces)) return r;
    if (n < 0 || (n > 0 && (!xy || !rgba))) return rt_fail(c, RT_ERR_ARG, "rt_render_pixels: bad buffers");
    for (int i = 0; i < n; i++)
        if (xy[2 * i] < 0 || xy[2 * i] >= w || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= h)
            return rt_fail(c, RT_ERR_ARG, "rt_render_pixels: pixel outside the image");
    if (n == 0) return RT_OK;
    return rt_backend_render_pixels(c, w, h, spp, bounces, xy, n, rgba);
}

int rt_intersect(rt_context* c, const float* rays, int n, void* out)
{
    if (!c || !c->have_scene || !c->have_bvh) return rt_fail(c, RT_ERR_STATE, "rt_intersect: scene/BVH not set");
    if (n < 0 || (n > 0 && (!rays || !out))) return rt_fail(c, RT_ERR_ARG, "rt_intersect: bad buffers");
    if (n == 0) return RT_OK;
    if (int r = rt_tables_current(c, false, true)) return r;
    return rt_backend_intersect(c, rays, n, out);
}

// ------------------------------------------------------------ ray queries
static int query_ready(rt_context* c, const char* fn, int mode, const void* rays, long n, const void* out)
{
    const std::string f = fn;
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, f + ": ctx is NULL");
    if (!c->have_scene || !c->have_bvh) return rt_fail(c, RT_ERR_STATE, f + ": scene/BVH not set");
    const int m = mode & ~RT_QUERY_EXACT;
    if (m != RT_QUERY_CLOSEST && m != RT_QUERY_ANY) return rt_fail(c, RT_ERR_ARG, f + ": unknown mode");
    if (n < 0) return rt_fail(c, RT_ERR_ARG, f + ": n is negative");
    if (n >= (1L << 27)) return rt_fail(c, RT_ERR_ARG, f + ": n must be below 2^27");
    if (n > 0 && (!rays || !out)) return rt_fail(c, RT_ERR_ARG, f + ": a buffer is NULL");
    if (n == 0) {
        c->query_exact = 0;
        c->query_on_device = false;
        return RT_OK;
    }
    return rt_tables_current(c, false, true);
}

// Spheres and the brute-force mode take k_intersect's path for every query (rt_query.h).
static bool query_all_exact(const rt_context* c, int mode)
{
    return (mode & RT_QUERY_EXACT) != 0 || !c->spheres.empty() || c->brute;
}

int rt_query(rt_context* c, int mode, const float* rays, long n, void* out)
{
    if (int r = query_ready(c, "rt_query", mode, rays, n, out)) return r;
    if (n == 0) return RT_OK;
    return rt_backend_query(c, (mode & ~RT_QUERY_EXACT) == RT_QUERY_ANY, query_all_exact(c, mode), rays, n, out, false,
                            nullptr);
}

int rt_query_device(rt_context* c, int mode, const void* d_rays, long n, void* d_out, void* stream)
{
    if (int r = query_ready(c, "rt_query_device", mode, d_rays, n, d_out)) return r;
    if (n == 0) return RT_OK;
    return rt_backend_query(c, (mode & ~RT_QUERY_EXACT) == RT_QUERY_ANY, query_all_exact(c, mode), d_rays, n, d_out,
                            true, stream);
}

long rt_query_last_exact(rt_context* c)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "rt_query_last_exact: ctx is NULL");
    return rt_backend_query_last_exact(c);
}

int rt_set_intersect_mode(rt_context* c, int use_bvh)
{
    if (!c) return RT_ERR_ARG;
    progress_drop(c);
    c->brute = use_bvh == 0;
    c->dirty = true;
    return RT_OK;
}

// ------------------------------------------------- progressive rendering
#define RT_PROGRESS_MAGIC 0x47505452  // "RTPG"
#define RT_PROGRESS_VERSION 1         // an untracked progression: header, base, state
#define RT_PROGRESS_VERSION_TRACKED 2 // a tracked one: header, {passes, nA}, base, state, half
#define RT_PROGRESS_VERSION_ADAPTIVE 3 // an adaptive one: version 2 (done = nA + nB), then tile_n, then tile_nA
#define RT_PROGRESS_HEADER 10         // int32 words: magic, version, the eight info words

static bool ctx_is_multi(const rt_context* c) { return c->devices.size() > 1 || (c->force_multi && !c->devices.empty()); }

// The frame of a progression: begin's arguments, or a checkpoint's header (fn names the caller).
static int progress_frame(rt_context* c, const char* fn, int w, int h, int total, int bounces, int off, int stride)
{
    const std::string f = fn;
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, f + ": ctx is NULL");
    if (ctx_is_multi(c))
        return rt_fail(c, RT_ERR_ARG, f + ": multi-device contexts are not supported (one process per GPU, each with its row shard)");
    if (int r = check_ready(c, w, h, total, bounces)) return r;
    if (stride <= 0 || off < 0 || off >= stride || off >= h) return rt_fail(c, RT_ERR_ARG, f + ": row shard outside the frame");
    const int rows = (h - off + stride - 1) / stride;
    if ((size_t)rows * w > 0x7fffffff / 8) return rt_fail(c, RT_ERR_ARG, f + ": too many pixels for one launch");
    return RT_OK;
}

static void progress_install(rt_context* c, int w, int h, int total, int done, int bounces, int off, int stride)
{
    RtProgress& P = c->prog;
    P.active = true;
    P.w = w, P.h = h, P.total = total, P.done = done, P.bounces = bounces, P.off = off, P.stride = stride;
    P.rows = (h - off + stride - 1) / stride;
}

int rt_progress_begin(rt_context* c, int w, int h, int total, int bounces, const float* base, int off, int stride)
{
    if (int r = progress_frame(c, "rt_progress_begin", w, h, total, bounces, off, stride)) return r;
    progress_drop(c);
    progress_install(c, w, h, total, 0, bounces, off, stride);
    if (int r = rt_backend_progress_begin(c, base, nullptr)) {
        progress_drop(c);
        return r;
    }
    return RT_OK;
}

static int progress_active(rt_context* c, const char* fn)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, std::string(fn) + ": ctx is NULL");
    if (!c->prog.active)
        return rt_fail(c, RT_ERR_STATE, std::string(fn) + ": no progression (none begun, or a rebind ended it)");
    return RT_OK;
}

int rt_progress_advance(rt_context* c, int samples, void* stream)
{
    if (int r = progress_active(c, "rt_progress_advance")) return r;
    if (samples <= 0) return rt_fail(c, RT_ERR_ARG, "rt_progress_advance: samples must be positive");
    RtProgress& P = c->prog;
    if (P.adaptive && P.tile_max != P.done)
        return rt_fail(c, RT_ERR_STATE, "rt_progress_advance: the tiles of this adaptive progression have different sample "
                                        "counts (rt_progress_advance_adaptive)");
    const int stop = P.done + std::min(samples, P.total - P.done);
    if (stop == P.done) return RT_OK;  // nothing left: no launch
    // (rt_render_variants or rt_set_stats since the last pass: the bound tables go up again)
    if (int r = check_ready(c, P.w, P.h, P.total, P.bounces)) return r;
    if (int r = rt_backend_progress_advance(c, P.done, stop, stream)) return r;
    if (P.adaptive)  // (equal counts: the tile arrays stay in step with the pass, once it is enqueued)
        if (int r = rt_backend_progress_adapt_bump(c, stop - P.done, P.next_is_a(), stream)) return r;
    if (P.tracked) {  // (the backend folded this pass into half if it was an A pass)
        if (P.next_is_a()) P.n_a += stop - P.done;
        else P.n_b += stop - P.done;
        P.passes++;
    }
    P.done = P.tile_max = stop;
    return RT_OK;
}

static bool threshold_ok(float t) { return std::isfinite(t) && t >= 0.0f; }

int rt_progress_advance_adaptive(rt_context* c, int samples, float threshold, void* stream, int info[8])
{
    const char* fn = "rt_progress_advance_adaptive";
    const std::string f = fn;
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, f + ": ctx is NULL");
    if (ctx_is_multi(c)) return rt_fail(c, RT_ERR_ARG, f + ": multi-device contexts are not supported");
    if (int r = progress_active(c, fn)) return r;
    RtProgress& P = c->prog;
    if (!P.tracked) return rt_fail(c, RT_ERR_STATE, f + ": the progression is not tracked (rt_progress_noise_track)");
    if (samples <= 0) return rt_fail(c, RT_ERR_ARG, f + ": samples must be positive");
    if (!threshold_ok(threshold)) return rt_fail(c, RT_ERR_ARG, f + ": the threshold is not finite and >= 0");
    if (!info) return rt_fail(c, RT_ERR_ARG, f + ": info is NULL");
    if (int r = check_ready(c, P.w, P.h, P.total, P.bounces)) return r;
    if (!P.adaptive) {  // (the counts every tile has so far)
        if (int r = rt_backend_progress_adapt_begin(c, nullptr, nullptr)) return r;
        P.adaptive = true;
        P.n_b = P.done - P.n_a;
        P.tile_max = P.done;
    }
    int32_t hdr[rtk::AD_WORDS];
    if (int r = rt_backend_progress_adapt_advance(c, samples, threshold, stream, hdr)) return r;
    if (hdr[rtk::AD_TILES_ACTIVE] > 0) {
        if (P.next_is_a()) P.n_a += samples;
        else P.n_b += samples;
        P.passes++;
    }
    P.done = hdr[rtk::AD_MIN];
    P.tile_max = hdr[rtk::AD_MAX];
    for (int i = 0; i < 8; i++) info[i] = hdr[i];
    return RT_OK;
}

int rt_progress_tile_counts(rt_context* c, int* tile_n, int* tile_nA)
{
    if (int r = progress_active(c, "rt_progress_tile_counts")) return r;
    const RtProgress& P = c->prog;
    if (!P.tracked) return rt_fail(c, RT_ERR_STATE, "rt_progress_tile_counts: the progression is not tracked");
    if (P.adaptive) return rt_backend_progress_adapt_counts(c, tile_n, tile_nA);
    const size_t n_tiles = (size_t)P.tiles_w() * P.tiles_h();
    if (tile_n) std::fill(tile_n, tile_n + n_tiles, P.done);
    if (tile_nA) std::fill(tile_nA, tile_nA + n_tiles, P.n_a);
    return RT_OK;
}

static int progress_resolve(rt_context* c, const char* fn, float* host_fb, void* dev_fb, void* stream,
                            bool linear = false)
{
    if (int r = progress_active(c, fn)) return r;
    if (!host_fb && !dev_fb) return rt_fail(c, RT_ERR_ARG, std::string(fn) + ": the output is NULL");
    if (c->prog.done == 0) return rt_fail(c, RT_ERR_STATE, std::string(fn) + ": no sample done yet");
    return rt_backend_progress_resolve(c, host_fb, dev_fb, stream, linear);
}

int rt_progress_resolve_linear(rt_context* c, float* fb)
{
    return progress_resolve(c, "rt_progress_resolve_linear", fb, nullptr, nullptr, true);
}

int rt_progress_resolve_linear_device(rt_context* c, void* d_fb, void* stream)
{
    return progress_resolve(c, "rt_progress_resolve_linear_device", nullptr, d_fb, stream, true);
}

int rt_progress_resolve(rt_context* c, float* fb) { return progress_resolve(c, "rt_progress_resolve", fb, nullptr, nullptr); }

int rt_progress_resolve_device(rt_context* c, void* d_fb, void* stream)
{
    return progress_resolve(c, "rt_progress_resolve_device", nullptr, d_fb, stream);
}

int rt_progress_info(const rt_context* c, int info[8])
{
    if (!c || !info) return rt_fail(nullptr, RT_ERR_ARG, "rt_progress_info: bad arguments");
    if (!c->prog.active) return RT_ERR_STATE;  // (const context: the message stays what it was)
    const RtProgress& P = c->prog;
    const int v[8] = {P.w, P.h, P.total, P.done, P.bounces, P.off, P.stride, P.rows};
    std::memcpy(info, v, sizeof v);
    return RT_OK;
}

long rt_progress_save(rt_context* c, void* buf, long capacity)
{
    if (int r = progress_active(c, "rt_progress_save")) return r;
    const RtProgress& P = c->prog;
    const size_t px = P.npx() * sizeof(float4_);
    const size_t extra = P.tracked ? 8 : 0, nbuf = P.tracked ? 3 : 2;
    const size_t counts = P.adaptive ? 4 * (size_t)P.tiles_w() * P.tiles_h() : 0;  // bytes of each count array
    const long size = (long)(RT_PROGRESS_HEADER * 4 + extra + nbuf * px + 2 * counts);
    if (!buf || capacity < size) return size;
    const int version = P.adaptive ? RT_PROGRESS_VERSION_ADAPTIVE : P.tracked ? RT_PROGRESS_VERSION_TRACKED : RT_PROGRESS_VERSION;
    const int32_t hd[RT_PROGRESS_HEADER] = {RT_PROGRESS_MAGIC, version, P.w, P.h, P.total, P.adaptive ? P.n_a + P.n_b : P.done,
                                            P.bounces, P.off, P.stride, P.rows};
    std::memcpy(buf, hd, sizeof hd);
    if (P.tracked) {
        const int32_t tr[2] = {P.passes, P.n_a};
        std::memcpy((char*)buf + sizeof hd, tr, sizeof tr);
    }
    // (the payload need not be aligned for float in the caller's buffer: staged)
    std::vector<float> tmp(nbuf * px / 4);
    if (int r = rt_backend_progress_read(c, tmp.data(), tmp.data() + px / 4)) return r;
    if (P.tracked)
        if (int r = rt_backend_progress_read_half(c, tmp.data() + 2 * px / 4)) return r;
    std::memcpy((char*)buf + sizeof hd + extra, tmp.data(), nbuf * px);
    if (P.adaptive) {
        std::vector<int32_t> tn(counts / 2);  // tile_n, then tile_nA
        if (int r = rt_backend_progress_adapt_counts(c, tn.data(), tn.data() + counts / 4)) return r;
        std::memcpy((char*)buf + sizeof hd + extra + nbuf * px, tn.data(), 2 * counts);
    }
    return size;
}

int rt_progress_load(rt_context* c, const void* buf, long bytes)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "rt_progress_load: ctx is NULL");
    if (!c->have_scene || !c->have_bvh || !c->have_env || !c->have_cam)
        return rt_fail(c, RT_ERR_STATE, "rt_progress_load: scene, BVH, environment map and camera must be bound first");
    if (!buf || bytes < RT_PROGRESS_HEADER * 4) return rt_fail(c, RT_ERR_ARG, "rt_progress_load: no header");
    int32_t hd[RT_PROGRESS_HEADER];
    std::memcpy(hd, buf, sizeof hd);
    if (hd[0] != RT_PROGRESS_MAGIC) return rt_fail(c, RT_ERR_ARG, "rt_progress_load: not a progression checkpoint (magic)");
    if (hd[1] != RT_PROGRESS_VERSION && hd[1] != RT_PROGRESS_VERSION_TRACKED && hd[1] != RT_PROGRESS_VERSION_ADAPTIVE)
        return rt_fail(c, RT_ERR_ARG, "rt_progress_load: unknown format version");
    const bool adaptive = hd[1] == RT_PROGRESS_VERSION_ADAPTIVE;
    const bool tracked = hd[1] == RT_PROGRESS_VERSION_TRACKED || adaptive;
    const size_t extra = tracked ? 8 : 0, nbuf = tracked ? 3 : 2;
    const int w = hd[2], h = hd[3], total = hd[4], done = hd[5], bounces = hd[6], off = hd[7], stride = hd[8], rows = hd[9];
    if (int r = progress_frame(c, "rt_progress_load", w, h, total, bounces, off, stride)) return r;
    // (version 3: done is nA + nB, which a threshold that changed between passes can take past the total)
    if (done < 0 || (done > total && !adaptive)) return rt_fail(c, RT_ERR_ARG, "rt_progress_load: done is outside 0..total");
    const int rows_h = (h - off + stride - 1) / stride;
    const size_t px = (size_t)rows_h * w * sizeof(float4_);
    const size_t n_tiles = (size_t)((rows_h + 7) / 8) * ((w + 7) / 8), counts = adaptive ? 4 * n_tiles : 0;
    if (rows != rows_h || (size_t)bytes != sizeof hd + extra + nbuf * px + 2 * counts)
        return rt_fail(c, RT_ERR_ARG, "rt_progress_load: the size does not match the header");
    int32_t tr[2] = {0, 0};  // passes, nA
    if (tracked) {
        std::memcpy(tr, (const char*)buf + sizeof hd, sizeof tr);
        if (tr[0] < 0) return rt_fail(c, RT_ERR_ARG, "rt_progress_load: a negative pass count");
        if (tr[1] < 0 || tr[1] > done) return rt_fail(c, RT_ERR_ARG, "rt_progress_load: the A passes' samples are outside 0..done");
    }
    std::vector<float> tmp(nbuf * px / 4);
    std::memcpy(tmp.data(), (const char*)buf + sizeof hd + extra, nbuf * px);
    std::vector<int32_t> tn(2 * n_tiles);  // tile_n, then tile_nA
    int t_min = done, t_max = done;
    if (adaptive) {
        std::memcpy(tn.data(), (const char*)buf + sizeof hd + extra + nbuf * px, 2 * counts);
        for (size_t t = 0; t < n_tiles; t++) {
            if (tn[t] < 0 || tn[t] > total) return rt_fail(c, RT_ERR_ARG, "rt_progress_load: a tile count is outside 0..total");
            if (tn[n_tiles + t] < 0 || tn[n_tiles + t] > tn[t])
                return rt_fail(c, RT_ERR_ARG, "rt_progress_load: a tile's A samples are outside 0..its count");
        }
        t_min = *std::min_element(tn.begin(), tn.begin() + n_tiles);
        t_max = *std::max_element(tn.begin(), tn.begin() + n_tiles);
        // (a pass starts its pixels' chains or goes on from their states, not both: no API call leaves such counts)
        if (t_min == 0 && t_max > 0) return rt_fail(c, RT_ERR_ARG, "rt_progress_load: tile counts mix zero and positive");
    }
    progress_drop(c);
    progress_install(c, w, h, total, adaptive ? t_min : done, bounces, off, stride);
    int r = rt_backend_progress_begin(c, tmp.data(), tmp.data() + px / 4);
    if (!r && tracked) r = rt_backend_progress_track(c, tmp.data() + 2 * px / 4);
    if (!r && adaptive) r = rt_backend_progress_adapt_begin(c, tn.data(), tn.data() + n_tiles);
    if (r) {
        progress_drop(c);
        return r;
    }
    c->prog.tracked = tracked;
    c->prog.passes = tr[0], c->prog.n_a = tr[1];
    c->prog.adaptive = adaptive;
    c->prog.n_b = done - tr[1];
    c->prog.tile_max = t_max;
    return RT_OK;
}

// ---- the noise estimate of a tracked progression (rt_noise.h)
int rt_progress_noise_track(rt_context* c)
{
    if (int r = progress_active(c, "rt_progress_noise_track")) return r;
    RtProgress& P = c->prog;
    if (P.tracked) return RT_OK;
    if (P.done > 0)
        return rt_fail(c, RT_ERR_STATE, "rt_progress_noise_track: samples are done already (track before the first pass)");
    if (int r = rt_backend_progress_track(c, nullptr)) return r;
    P.tracked = true;
    P.passes = P.n_a = 0;
    return RT_OK;
}

static int noise_ready(rt_context* c, const char* fn, float threshold, rtk::NoiseArgs& A)
{
    const std::string f = fn;
    if (int r = progress_active(c, fn)) return r;
    const RtProgress& P = c->prog;
    if (!P.tracked) return rt_fail(c, RT_ERR_STATE, f + ": the progression is not tracked (rt_progress_noise_track)");
    const int n_a = P.n_a, n_b = P.adaptive ? P.n_b : P.done - P.n_a;
    if (n_a <= 0 || n_b <= 0) return rt_fail(c, RT_ERR_STATE, f + ": needs a sample in both halves (two passes)");
    if (!threshold_ok(threshold)) return rt_fail(c, RT_ERR_ARG, f + ": the threshold is not finite and >= 0");
    A.n_all = (float)(n_a + n_b);
    A.n_a = (float)n_a;
    A.k = rt_sqrtf((float)n_a / (float)n_b);
    A.threshold = threshold;
    A.samples_a = n_a, A.samples_b = n_b, A.passes = P.passes;
    return RT_OK;
}

int rt_progress_noise(rt_context* c, float threshold, rt_noise_stats* stats, float* pixel_err, float* tile_err)
{
    rtk::NoiseArgs A;
    if (int r = noise_ready(c, "rt_progress_noise", threshold, A)) return r;
    if (!stats) return rt_fail(c, RT_ERR_ARG, "rt_progress_noise: stats is NULL");
    int32_t st[8];
    if (int r = c->prog.adaptive ? rt_backend_progress_adapt_noise(c, A, st, pixel_err, tile_err, false, nullptr)
                                 : rt_backend_progress_noise(c, A, st, pixel_err, tile_err, false, nullptr))
        return r;
    stats->max_tile = rt_asfloat((uint32_t)st[3]);
    stats->tiles = st[0], stats->tiles_over = st[1], stats->nonfinite = st[2];
    stats->samples_a = st[4], stats->samples_b = st[5], stats->passes = st[6];
    return RT_OK;
}

int rt_progress_noise_device(rt_context* c, float threshold, void* d_stats, void* d_pixel_err, void* d_tile_err,
                             void* stream)
{
    rtk::NoiseArgs A;
    if (int r = noise_ready(c, "rt_progress_noise_device", threshold, A)) return r;
    if (!d_stats) return rt_fail(c, RT_ERR_ARG, "rt_progress_noise_device: d_stats is NULL");
    if ((uintptr_t)d_stats % 4 != 0 || (uintptr_t)d_pixel_err % 4 != 0 || (uintptr_t)d_tile_err % 4 != 0)
        return rt_fail(c, RT_ERR_ARG, "rt_progress_noise_device: the buffers must be 4-byte aligned");
    if (c->prog.adaptive)  // (every tile with its own counts)
        return rt_backend_progress_adapt_noise(c, A, (int32_t*)d_stats, (float*)d_pixel_err, (float*)d_tile_err, true, stream);
    return rt_backend_progress_noise(c, A, (int32_t*)d_stats, (float*)d_pixel_err, (float*)d_tile_err, true, stream);
}

// ---- the estimate's numerator per pixel (rt_dnv.h): what rt_denoise_var takes as sigma
int rt_progress_noise_sigma(rt_context* c, float* sigma)
{
    rtk::NoiseArgs A;
    if (int r = noise_ready(c, "rt_progress_noise_sigma", 0.0f, A)) return r;
    if (!sigma) return rt_fail(c, RT_ERR_ARG, "rt_progress_noise_sigma: sigma is NULL");
    return rt_backend_progress_noise_sigma(c, A, sigma, false, nullptr);
}

int rt_progress_noise_sigma_device(rt_context* c, void* d_sigma, void* stream)
{
    rtk::NoiseArgs A;
    if (int r = noise_ready(c, "rt_progress_noise_sigma_device", 0.0f, A)) return r;
    if (!d_sigma) return rt_fail(c, RT_ERR_ARG, "rt_progress_noise_sigma_device: d_sigma is NULL");
    if ((uintptr_t)d_sigma % 4 != 0)
        return rt_fail(c, RT_ERR_ARG, "rt_progress_noise_sigma_device: the buffer must be 4-byte aligned");
    return rt_backend_progress_noise_sigma(c, A, (float*)d_sigma, true, stream);
}

void rt_progress_end(rt_context* c) { progress_drop(c); }

int rt_set_stats(rt_context* c, int enabled)
{
    if (!c) return RT_ERR_ARG;
    c->stats_enabled = enabled != 0;
    c->stats_seq = enabled == 2;
    return RT_OK;
}

int rt_get_stats(const rt_context* c, unsigned long long* out, int n)
{
    if (!c || !out) return RT_ERR_ARG;
    for (int i = 0; i < n && i < 2 * RT_STAT_COUNT; i++) out[i] = c->stats[i];
    return RT_OK;
}

double rt_last_kernel_ms(const rt_context* c) { return c ? c->last_kernel_ms : -1.0; }

// ------------------------------------------------------------- host helpers
struct rt_mesh {
    rt::Mesh m;
};

int rt_mesh_load(const char* path, rt_mesh** out)
{
    if (!path || !out) return rt_fail(nullptr, RT_ERR_ARG, "rt_mesh_load: bad arguments");
    *out = nullptr;
    rt_mesh* m = new rt_mesh();
    std::string err;
    int r = rt::load_obj(path, m->m, err);
    if (r) {
        delete m;
        return rt_fail(nullptr, RT_ERR_IO, "rt_mesh_load: " + err);
    }
    *out = m;
    return RT_OK;
}

int rt_mesh_counts(const rt_mesh* m, int* nt, int* nm, int* ne)
{
    if (!m) return RT_ERR_ARG;
    if (nt) *nt = m->m.ntris();
    if (nm) *nm = (int)(m->m.mats.size() / 10);
    if (ne) *ne = (int)m->m.emissive.size();
    return RT_OK;
}

int rt_mesh_copy(const rt_mesh* m, float* tris, int* mi, float* mats, int* em)
{
    if (!m) return RT_ERR_ARG;
    if (tris) std::memcpy(tris, m->m.tris.data(), m->m.tris.size() * 4);
    if (mi) std::memcpy(mi, m->m.mat_idx.data(), m->m.mat_idx.size() * 4);
    if (mats) std::memcpy(mats, m->m.mats.data(), m->m.mats.size() * 4);
    if (em) std::memcpy(em, m->m.emissive.data(), m->m.emissive.size() * 4);
    return RT_OK;
}

void rt_mesh_free(rt_mesh* m) { delete m; }

int rt_camera_preset(const char* name, float view[16], float* fov_dist)
{
    if (!name || !view || !fov_dist) return RT_ERR_ARG;
    return rt::camera_preset(name, view, fov_dist) ? rt_fail(nullptr, RT_ERR_ARG, "unknown camera preset") : RT_OK;
}

int rt_env_luminance_cdf(const float* px, int w, int h, int ch, float* lum, float* cdf)
{
    if (!px || w <= 0 || h <= 0 || (ch != 3 && ch != 4) || !lum || !cdf) return RT_ERR_ARG;
    rt::env_luminance_cdf(px, w, h, ch, lum, cdf);
    return RT_OK;
}

long rt_octree_dump(const float* tris, int n, int max_depth, int leaf_max, void* buf, long cap)
{
    if (!tris || n < 0) return RT_ERR_ARG;
    rt::Octree t;
    rt::build_octree(tris, n, max_depth, leaf_max, t);
    std::vector<char> d = rt::dump_octree(t);
    if (buf && cap >= (long)d.size()) std::memcpy(buf, d.data(), d.size());
    return (long)d.size();
}

}  // extern "C"

// ------------------------------------------------------------- image I/O
int rt_read_hdr(const char* path, int flip_y, int* width, int* height, float* pixels_rgba)
{
    if (!path || !width || !height) return rt_fail(nullptr, RT_ERR_ARG, "rt_read_hdr: bad arguments");
    int w = 0, h = 0;
    std::vector<float> rgb;
    std::string err;
    if (rt::read_hdr(path, flip_y != 0, w, h, rgb, err)) return rt_fail(nullptr, RT_ERR_IO, "rt_read_hdr: " + err);
    if (pixels_rgba) {
        if (*width != w || *height != h) return rt_fail(nullptr, RT_ERR_ARG, "rt_read_hdr: buffer size does not match the image");
        for (size_t i = 0; i < (size_t)w * h; i++) {  // Color(r, g, b, 0.0f): utils.cpp:114-120
            pixels_rgba[4 * i] = rgb[3 * i];
            pixels_rgba[4 * i + 1] = rgb[3 * i + 1];
            pixels_rgba[4 * i + 2] = rgb[3 * i + 2];
            pixels_rgba[4 * i + 3] = 0.0f;
        }
    }
    *width = w;
    *height = h;
    return RT_OK;
}

int rt_image_to_rgba8(const float* rgba, long n_pixels, unsigned char* out)
{
    if (n_pixels < 0 || (n_pixels > 0 && (!rgba || !out))) return rt_fail(nullptr, RT_ERR_ARG, "rt_image_to_rgba8: bad arguments");
    rt::rgba8(rgba, (size_t)n_pixels, out);
    return RT_OK;
}

int rt_write_hdr(const char* path, const float* rgba, int width, int height, int flip_y)
{
    if (!path || width <= 0 || height <= 0 || !rgba) return rt_fail(nullptr, RT_ERR_ARG, "rt_write_hdr: bad arguments");
    std::string err;
    if (rt::write_hdr(path, rgba, width, height, flip_y != 0, err)) return rt_fail(nullptr, RT_ERR_IO, "rt_write_hdr: " + err);
    return RT_OK;
}

int rt_write_png(const char* path, const float* rgba, int width, int height, int flip_y)
{
    if (!path || (width > 0 && height > 0 && !rgba)) return rt_fail(nullptr, RT_ERR_ARG, "rt_write_png: bad arguments");
    std::string err;
    if (rt::write_png(path, rgba, width, height, flip_y != 0, err)) return rt_fail(nullptr, RT_ERR_IO, "rt_write_png: " + err);
    return RT_OK;
}

