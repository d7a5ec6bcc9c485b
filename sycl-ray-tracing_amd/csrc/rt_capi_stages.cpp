// rt_capi_stages.cpp — the frame stages of the C ABI (include/rt_hip.h), backend-independent like
// rt_capi_host.cpp: camera rays and feature buffers, then denoise, denoise_var, temporal
// accumulation, firefly rejection, guided upscale, depth of field, motion vectors and motion blur, bloom, metering and display. Each stage is its defaults,
// a *_ready function that checks the call (the shared rules: rt_stage_args.h) and the two entry
// points, host form and device form, over its rt_backend_* hook.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rt_context.h"
#include "rt_bloom.h"
#include "rt_denoise.h"
#include "rt_dof.h"
#include "rt_firefly.h"
#include "rt_meter.h"
#include "rt_motion.h"
#include "rt_stage_args.h"
#include "rt_temporal.h"
#include "rt_upscale.h"

// ------------------------------------------------------------- post stage
int rt_camera_rays(rt_context* c, int w, int h, float* rays)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "rt_camera_rays: ctx is NULL");
    if (!c->have_cam) return rt_fail(c, RT_ERR_STATE, "rt_camera_rays: camera not set");
    if (w <= 0 || h <= 0 || !rays) return rt_fail(c, RT_ERR_ARG, "rt_camera_rays: bad arguments");
    const rtk::CamView V = rtk::cam_view(c->cam, w, h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            rtk::V3 o, d;
            rtk::feature_ray(V, x, y, o, d);
            float* r = rays + 6 * ((size_t)y * w + x);
            r[0] = o.x, r[1] = o.y, r[2] = o.z, r[3] = d.x, r[4] = d.y, r[5] = d.z;
        }
    return RT_OK;
}

static int features_ready(rt_context* c, int w, int h, const void* alb, const void* nd)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "rt_render_features: ctx is NULL");
    if (!c->have_scene || !c->have_bvh) return rt_fail(c, RT_ERR_STATE, "rt_render_features: scene/BVH not set");
    if (!c->have_cam) return rt_fail(c, RT_ERR_STATE, "rt_render_features: camera not set");
    if (w <= 0 || h <= 0 || !alb || !nd || alb == nd) return rt_fail(c, RT_ERR_ARG, "rt_render_features: bad buffers");
    if ((double)w * (double)h > 268435455.0) return rt_fail(c, RT_ERR_ARG, "rt_render_features: too many pixels");
    return rt_tables_current(c, true, true);
}

int rt_render_features(rt_context* c, int w, int h, float* albedo, float* normal_depth)
{
    if (int r = features_ready(c, w, h, albedo, normal_depth)) return r;
    return rt_backend_features(c, w, h, albedo, normal_depth, false, nullptr);
}

int rt_render_features_device(rt_context* c, int w, int h, void* d_albedo, void* d_normal_depth, void* stream)
{
    if (int r = features_ready(c, w, h, d_albedo, d_normal_depth)) return r;
    return rt_backend_features(c, w, h, d_albedo, d_normal_depth, true, stream);
}

// ---- the first-hit G-buffer on the render's walks (rt_gbuffer.h)
static int gbuffer_ready(rt_context* c, const char* fn, int w, int h, int flags, const void* alb, const void* nd,
                         const void* ids, bool device)
{
    const size_t n = w > 0 && h > 0 ? (size_t)w * h : 0;
    const StageArgs a{c, fn, device, {{alb, 16 * n, SA_OUT, SA_REQ, 16}, {nd, 16 * n, SA_OUT, SA_REQ, 16}, {ids, 8 * n, SA_OUT, SA_OPT, 8}}};
    if (!c) return a.fail(": ctx is NULL");
    if (!c->have_scene || !c->have_bvh) return a.fail(": scene/BVH not set", RT_ERR_STATE);
    if (!c->have_cam) return a.fail(": camera not set", RT_ERR_STATE);
    if (w <= 0 || h <= 0) return a.fail(": w and h must be at least 1");
    if (int r = a.frame_limits(w, h, false)) return r;
    if (flags & ~RT_GBUFFER_EXACT) return a.fail(": unknown flag bits");
    if (a.missing()) return a.fail(": albedo or normal_depth is NULL");
    if (int r = a.overlap()) return r;
    if (int r = a.aligned(": the float4 buffers must be 16-byte aligned, ids 8-byte aligned")) return r;
    return rt_tables_current(c, true, true);
}

// Spheres and the brute-force mode have no search-BVH walk and no octree answer to share (rt_query.h).
static bool gbuffer_all_exact(const rt_context* c, int flags)
{
    return (flags & RT_GBUFFER_EXACT) != 0 || !c->spheres.empty() || c->brute;
}

int rt_render_gbuffer(rt_context* c, int w, int h, int flags, float* albedo, float* normal_depth, int* ids)
{
    if (int r = gbuffer_ready(c, "rt_render_gbuffer", w, h, flags, albedo, normal_depth, ids, false)) return r;
    return rt_backend_gbuffer(c, w, h, gbuffer_all_exact(c, flags), albedo, normal_depth, ids, false, nullptr);
}

int rt_render_gbuffer_device(rt_context* c, int w, int h, int flags, void* d_albedo, void* d_normal_depth, void* d_ids,
                             void* stream)
{
    if (int r = gbuffer_ready(c, "rt_render_gbuffer_device", w, h, flags, d_albedo, d_normal_depth, d_ids, true)) return r;
    return rt_backend_gbuffer(c, w, h, gbuffer_all_exact(c, flags), d_albedo, d_normal_depth, d_ids, true, stream);
}

long rt_gbuffer_last_exact(rt_context* c)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "rt_gbuffer_last_exact: ctx is NULL");
    return rt_backend_gbuffer_last_exact(c);
}

// Defaults from the quality sweep on Cornell 64x64, 16 spp against 512 spp.
void rt_denoise_default_params(rt_denoise_params* p)
{
    if (!p) return;
    p->passes = 5;
    p->sigma_color = 1.0f;
    p->sigma_normal = 0.3f;
    p->sigma_albedo = 0.1f;
    p->sigma_depth = 0.1f;
}

// (both forms report as "rt_denoise"; no range-overlap and no alignment rule: only in == out is refused)
static int denoise_ready(rt_context* c, int w, int h, const void* in, const void* alb, const void* nd,
                         const rt_denoise_params* params, float blend, const void* out, rt_denoise_params& p)
{
    const StageArgs a{c, "rt_denoise", false, {{in, 0, SA_IN, SA_REQ, 16}, {out, 0, SA_OUT, SA_REQ, 16}}};
    if (!c) return a.fail(": ctx is NULL");
    if (w <= 0 || h <= 0 || a.missing()) return a.fail(": bad buffers");
    if (int r = a.frame_limits(w, h, true)) return r;
    if (in == out) return a.fail(": rgba_in and rgba_out are the same buffer");
    if ((alb == nullptr) != (nd == nullptr)) return a.fail(": albedo and normal_depth must both be given or both be NULL");
    p = params_or_defaults(params, rt_denoise_default_params);
    if (p.passes < 1 || p.passes > 10) return a.fail(": passes must be 1..10");
    const float sig[4] = {p.sigma_color, p.sigma_normal, p.sigma_albedo, p.sigma_depth};
    for (float s : sig)
        if (!std::isfinite(s) || !(s > 0.0f)) return a.fail(": a sigma is not finite and > 0");
    if (!std::isfinite(blend)) return a.fail(": blend is not finite");
    return RT_OK;
}

int rt_denoise(rt_context* c, int w, int h, const float* in, const float* alb, const float* nd,
               const rt_denoise_params* params, float blend, float* out)
{
    rt_denoise_params p;
    if (int r = denoise_ready(c, w, h, in, alb, nd, params, blend, out, p)) return r;
    return rt_backend_denoise(c, w, h, in, alb, nd, p, blend, out, false, nullptr);
}

int rt_denoise_device(rt_context* c, int w, int h, const void* in, const void* alb, const void* nd,
                      const rt_denoise_params* params, float blend, void* out, void* stream)
{
    rt_denoise_params p;
    if (int r = denoise_ready(c, w, h, in, alb, nd, params, blend, out, p)) return r;
    return rt_backend_denoise(c, w, h, in, alb, nd, p, blend, out, true, stream);
}

// ---- the variance-guided filter (rt_dnv.h)
// Defaults from the quality sweep on Cornell 64x64, a uniform and an adaptive 64-sample frame
// against 512 spp.
void rt_denoise_var_default_params(rt_denoise_var_params* p)
{
    if (!p) return;
    p->passes = 3;
    p->sigma_color = 1.0f;
    p->sigma_normal = 0.3f;
    p->sigma_albedo = 0.1f;
    p->sigma_depth = 0.1f;
    p->var_floor = 0.01f;
}

static int denoise_var_ready(rt_context* c, int w, int h, const void* in, const void* sigma, const void* alb, const void* nd,
                             const rt_denoise_var_params* params, float blend, const void* out, const void* sigma_out,
                             bool device, rt_denoise_var_params& p)
{
    if (!c) return rt_fail(nullptr, RT_ERR_ARG, "rt_denoise_var: ctx is NULL");
    p = params_or_defaults(params, rt_denoise_var_default_params);
    // (rt_denoise's own checks, on its share of the arguments)
    const rt_denoise_params q{p.passes, p.sigma_color, p.sigma_normal, p.sigma_albedo, p.sigma_depth};
    rt_denoise_params unused;
    if (int r = denoise_ready(c, w, h, in, alb, nd, &q, blend, out, unused)) return r;
    if (!sigma) return rt_fail(c, RT_ERR_ARG, "rt_denoise_var: sigma is NULL");
    if (!std::isfinite(p.var_floor) || !(p.var_floor > 0.0f))
        return rt_fail(c, RT_ERR_ARG, "rt_denoise_var: var_floor is not finite and > 0");
    // (the one rule that names the device form; no overlap rule, as in rt_denoise)
    const StageArgs a{c, "rt_denoise_var_device", device,
                      {{in, 0, SA_IN, SA_REQ, 16}, {sigma, 0, SA_IN, SA_REQ, 4}, {alb, 0, SA_IN, SA_OPT, 16},
                       {nd, 0, SA_IN, SA_OPT, 16}, {out, 0, SA_OUT, SA_REQ, 16}, {sigma_out, 0, SA_OUT, SA_OPT, 4}}};
    return a.aligned(": the float4 buffers must be 16-byte aligned, sigma and sigma_out 4-byte aligned");
}

int rt_denoise_var(rt_context* c, int w, int h, const float* in, const float* sigma, const float* alb, const float* nd,
                   const rt_denoise_var_params* params, float blend, float* out, float* sigma_out)
{
    rt_denoise_var_params p;
    if (int r = denoise_var_ready(c, w, h, in, sigma, alb, nd, params, blend, out, sigma_out, false, p)) return r;
    return rt_backend_denoise_var(c, w, h, in, sigma, alb, nd, p, blend, out, sigma_out, false, nullptr);
}

int rt_denoise_var_device(rt_context* c, int w, int h, const void* in, const void* sigma, const void* alb, const void* nd,
                          const rt_denoise_var_params* params, float blend, void* out, void* sigma_out, void* stream)
{
    rt_denoise_var_params p;
    if (int r = denoise_var_ready(c, w, h, in, sigma, alb, nd, params, blend, out, sigma_out, true, p)) return r;
    return rt_backend_denoise_var(c, w, h, in, sigma, alb, nd, p, blend, out, sigma_out, true, stream);
}

// ---- temporal accumulation (rt_temporal.h)
// Defaults: SVGF's depth and normal tests at the widths its authors' code uses for static scenes, a
// history of 32 frames.
void rt_temporal_default_params(rt_temporal_params* p)
{
    if (!p) return;
    p->depth_tol = 0.05f;
    p->normal_cos = 0.9f;
    p->min_weight = 0.1f;
    p->max_len = 32.0f;
}

// The inverse of a row-major 4x4 in double (Gauss-Jordan, partial pivoting), rounded to float.
// false: a non-finite entry, a zero pivot (singular) or a non-finite result.
static bool invert_view(const float m[16], float inv[16])
{
    double a[4][8];
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) {
            if (!std::isfinite(m[4 * r + k])) return false;
            a[r][k] = m[4 * r + k];
            a[r][4 + k] = r == k ? 1.0 : 0.0;
        }
    for (int col = 0; col < 4; col++) {
        int piv = col;
        for (int r = col + 1; r < 4; r++)
            if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (a[piv][col] == 0.0) return false;
        if (piv != col)
            for (int k = 0; k < 8; k++) std::swap(a[piv][k], a[col][k]);
        const double d = a[col][col];
        for (int k = 0; k < 8; k++) a[col][k] /= d;
        for (int r = 0; r < 4; r++) {
            if (r == col) continue;
            const double f = a[r][col];
            if (f == 0.0) continue;
            for (int k = 0; k < 8; k++) a[r][k] -= f * a[col][k];
        }
    }
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) {
            inv[4 * r + k] = (float)a[r][4 + k];
            if (!std::isfinite(inv[4 * r + k])) return false;
        }
    return true;
}

static int temporal_ready(rt_context* c, const char* fn, int w, int h, const void* in, const void* sigma, const void* nd,
                          const float* prev_view, float prev_fov, const void* h_rgba, const void* h_sigma,
                          const void* h_len, const void* h_nd, const rt_temporal_params* params, const void* out,
                          const void* sigma_out, const void* len_out, bool device, rtk::TemporalFrame& T)
{
    const size_t n = (size_t)w * h;
    const StageArgs a{c, fn, device,
                      {{in, 16 * n, SA_IN, SA_REQ, 16}, {sigma, 4 * n, SA_IN, SA_REQ, 4}, {nd, 16 * n, SA_IN, SA_REQ, 16},
                       {h_rgba, 16 * n, SA_IN, SA_OPT, 16}, {h_sigma, 4 * n, SA_IN, SA_OPT, 4}, {h_len, 4 * n, SA_IN, SA_OPT, 4},
                       {h_nd, 16 * n, SA_IN, SA_OPT, 16}, {out, 16 * n, SA_OUT, SA_REQ, 16}, {sigma_out, 4 * n, SA_OUT, SA_REQ, 4},
                       {len_out, 4 * n, SA_OUT, SA_REQ, 4}}};
    if (!c) return a.fail(": ctx is NULL");
    if (!c->have_cam) return a.fail(": camera not set", RT_ERR_STATE);
    if (w <= 0 || h <= 0 || a.missing() || !prev_view) return a.fail(": bad buffers");
    if (int r = a.frame_limits(w, h, true)) return r;
    const int given = (h_rgba != nullptr) + (h_sigma != nullptr) + (h_len != nullptr) + (h_nd != nullptr);
    if (given != 0 && given != 4) return a.fail(": the four history buffers must all be given or all be NULL");
    const rt_temporal_params p = params_or_defaults(params, rt_temporal_default_params);
    if (!std::isfinite(p.depth_tol) || !std::isfinite(p.normal_cos) || !std::isfinite(p.min_weight) || !std::isfinite(p.max_len))
        return a.fail(": a parameter is not finite");
    if (p.depth_tol < 0.0f) return a.fail(": depth_tol is negative");
    if (p.normal_cos < -1.0f || p.normal_cos > 1.0f) return a.fail(": normal_cos is outside [-1, 1]");
    if (p.min_weight < 0.0f || !(p.min_weight < 1.0f)) return a.fail(": min_weight is outside [0, 1)");
    if (p.max_len < 1.0f) return a.fail(": max_len is below 1");
    if (!std::isfinite(prev_fov) || prev_fov == 0.0f) return a.fail(": prev_fov_dist is zero or not finite");
    if (int r = a.overlap()) return r;
    if (int r = a.aligned()) return r;
    T.cur = rtk::cam_view(c->cam, w, h);
    if (!invert_view(prev_view, T.prev_inv.m)) return a.fail(": prev_view is singular or not finite");
    T.prev_inv.fov_dist = prev_fov;
    RtCamera prev;
    std::memcpy(prev.m, prev_view, 64);
    prev.fov_dist = prev_fov;
    const rtk::V3 op = rtk::xform_point(prev, rtk::v3(0.0f, 0.0f, 0.0f));
    T.o_prev[0] = op.x, T.o_prev[1] = op.y, T.o_prev[2] = op.z;
    T.depth_tol = p.depth_tol, T.normal_cos = p.normal_cos, T.min_weight = p.min_weight, T.max_len = p.max_len;
    T.in = (const float4_*)in, T.sigma = (const float*)sigma, T.nd = (const float4_*)nd;
    T.h_rgba = (const float4_*)h_rgba, T.h_sigma = (const float*)h_sigma, T.h_len = (const float*)h_len;
    T.h_nd = (const float4_*)h_nd;
    return RT_OK;
}

int rt_temporal_accumulate(rt_context* c, int w, int h, const float* in, const float* sigma, const float* nd,
                           const float prev_view[16], float prev_fov_dist, const float* hist_rgba, const float* hist_sigma,
                           const float* hist_len, const float* hist_nd, const rt_temporal_params* params, float* out,
                           float* sigma_out, float* len_out)
{
    rtk::TemporalFrame T;
    if (int r = temporal_ready(c, "rt_temporal_accumulate", w, h, in, sigma, nd, prev_view, prev_fov_dist, hist_rgba,
                               hist_sigma, hist_len, hist_nd, params, out, sigma_out, len_out, false, T))
        return r;
    return rt_backend_temporal(c, T, out, sigma_out, len_out, false, nullptr);
}

int rt_temporal_accumulate_device(rt_context* c, int w, int h, const void* in, const void* sigma, const void* nd,
                                  const float prev_view[16], float prev_fov_dist, const void* hist_rgba,
                                  const void* hist_sigma, const void* hist_len, const void* hist_nd,
                                  const rt_temporal_params* params, void* out, void* sigma_out, void* len_out, void* stream)
{
    rtk::TemporalFrame T;
    if (int r = temporal_ready(c, "rt_temporal_accumulate_device", w, h, in, sigma, nd, prev_view, prev_fov_dist, hist_rgba,
                               hist_sigma, hist_len, hist_nd, params, out, sigma_out, len_out, true, T))
        return r;
    return rt_backend_temporal(c, T, out, sigma_out, len_out, true, stream);
}

// ---- firefly rejection (rt_firefly.h)
// Defaults from the sweep on Cornell 64x64, a 4-sample frame against 256 spp.
void rt_firefly_default_params(rt_firefly_params* p)
{
    if (!p) return;
    p->radius = 1;
    p->rank = 2;
    p->gain = 2.0f;
    p->floor = 0.0f;
}

static int firefly_ready(rt_context* c, const char* fn, int w, int h, const void* in, const void* sigma,
                         const rt_firefly_params* params, const void* out, const void* sigma_out, const void* scale_out,
                         bool device, rtk::FireflyArgs& A)
{
    const size_t n = (size_t)w * h;
    const StageArgs a{c, fn, device,
                      {{in, 16 * n, SA_IN, SA_REQ, 16}, {sigma, 4 * n, SA_IN, SA_OPT, 4}, {out, 16 * n, SA_OUT, SA_REQ, 16},
                       {sigma_out, 4 * n, SA_OUT, SA_OPT, 4}, {scale_out, 4 * n, SA_OUT, SA_OPT, 4}}};
    if (!c) return a.fail(": ctx is NULL");
    if (w <= 0 || h <= 0) return a.fail(": w and h must be at least 1");
    if (a.missing()) return a.fail(": rgba_in or rgba_out is NULL");
    if (sigma_out && !sigma) return a.fail(": sigma_out without a sigma_in");
    if (int r = a.frame_limits(w, h, true)) return r;
    const rt_firefly_params p = params_or_defaults(params, rt_firefly_default_params);
    if (p.radius < 1 || p.radius > 2) return a.fail(": radius must be 1 or 2");
    if (p.rank < 1 || p.rank > rtk::FF_MAX_RANK) return a.fail(": rank must be 1..8");
    if (!(p.gain >= 0.0f)) return a.fail(": gain is negative or a NaN");
    if (p.floor != p.floor) return a.fail(": floor is a NaN");
    if (int r = a.overlap()) return r;
    if (int r = a.aligned()) return r;
    A = rtk::FireflyArgs{w, h, p.radius, p.rank, p.gain, p.floor, (const float4_*)in, (const float*)sigma};
    return RT_OK;
}

int rt_firefly(rt_context* c, int w, int h, const float* in, const float* sigma, const rt_firefly_params* params, float* out,
               float* sigma_out, float* scale_out)
{
    rtk::FireflyArgs A;
    if (int r = firefly_ready(c, "rt_firefly", w, h, in, sigma, params, out, sigma_out, scale_out, false, A)) return r;
    return rt_backend_firefly(c, A, out, sigma_out, scale_out, false, nullptr);
}

int rt_firefly_device(rt_context* c, int w, int h, const void* in, const void* sigma, const rt_firefly_params* params,
                      void* out, void* sigma_out, void* scale_out, void* stream)
{
    rtk::FireflyArgs A;
    if (int r = firefly_ready(c, "rt_firefly_device", w, h, in, sigma, params, out, sigma_out, scale_out, true, A)) return r;
    return rt_backend_firefly(c, A, out, sigma_out, scale_out, true, stream);
}

// ---- guided upscale (rt_upscale.h)
// The guide sigmas are rt_denoise's; min_weight is the share of a pixel's bilinear weight below which
// the four taps are taken as not seeing its surface.
void rt_upscale_default_params(rt_upscale_params* p)
{
    if (!p) return;
    rt_denoise_params d;
    rt_denoise_default_params(&d);
    p->sigma_normal = d.sigma_normal;
    p->sigma_albedo = d.sigma_albedo;
    p->sigma_depth = d.sigma_depth;
    p->min_weight = 0.1f;
}

static int upscale_ready(rt_context* c, const char* fn, int w_lo, int h_lo, int w, int h, const void* rgba_lo,
                         const void* sigma_lo, const void* alb_lo, const void* nd_lo, const void* alb_hi, const void* nd_hi,
                         const rt_upscale_params* params, const void* out, const void* sigma_out, bool device, rtk::UpArgs& A)
{
    // (the inputs of the low frame by its size, the guides and the outputs by the full frame's)
    const size_t n_lo = (size_t)w_lo * h_lo, n = (size_t)w * h;
    const StageArgs a{c, fn, device,
                      {{rgba_lo, 16 * n_lo, SA_IN, SA_REQ, 16}, {sigma_lo, 4 * n_lo, SA_IN, SA_OPT, 4},
                       {alb_lo, 16 * n_lo, SA_IN, SA_REQ, 16}, {nd_lo, 16 * n_lo, SA_IN, SA_REQ, 16},
                       {alb_hi, 16 * n, SA_IN, SA_REQ, 16}, {nd_hi, 16 * n, SA_IN, SA_REQ, 16},
                       {out, 16 * n, SA_OUT, SA_REQ, 16}, {sigma_out, 4 * n, SA_OUT, SA_OPT, 4}}};
    if (!c) return a.fail(": ctx is NULL");
    if (w_lo <= 0 || h_lo <= 0 || w <= 0 || h <= 0) return a.fail(": every size must be at least 1");
    if (w_lo > w || h_lo > h) return a.fail(": the low frame is larger than the output (w_lo > w or h_lo > h)");
    if (a.missing()) return a.fail(": a frame, a guide buffer or rgba_out is NULL");
    if (sigma_out && !sigma_lo) return a.fail(": sigma_out without a sigma_lo");
    if (sigma_lo && !sigma_out) return a.fail(": sigma_lo without a sigma_out");
    // (the limits on the output: the kernels tile it)
    if (int r = a.frame_limits(w, h, true)) return r;
    const rt_upscale_params p = params_or_defaults(params, rt_upscale_default_params);
    const float sig[3] = {p.sigma_normal, p.sigma_albedo, p.sigma_depth};
    for (float s : sig)
        if (!(s > 0.0f) || !std::isfinite(s)) return a.fail(": sigma_normal, sigma_albedo and sigma_depth must be positive and finite");
    if (!(p.min_weight >= 0.0f && p.min_weight < 1.0f)) return a.fail(": min_weight must lie in [0, 1)");
    if (int r = a.overlap(true)) return r;
    if (int r = a.aligned()) return r;
    A = rtk::UpArgs{w_lo, h_lo, w, h, (float)w_lo / (float)w, (float)h_lo / (float)h, rtk::dn_inv_sigma2(p.sigma_normal),
                    rtk::dn_inv_sigma2(p.sigma_albedo), rtk::dn_inv_sigma2(p.sigma_depth), p.min_weight,
                    (const float4_*)rgba_lo, (const float*)sigma_lo, (const float4_*)alb_lo, (const float4_*)nd_lo,
                    (const float4_*)alb_hi, (const float4_*)nd_hi};
    return RT_OK;
}

int rt_upscale(rt_context* c, int w_lo, int h_lo, int w, int h, const float* rgba_lo, const float* sigma_lo,
               const float* albedo_lo, const float* normal_depth_lo, const float* albedo_hi, const float* normal_depth_hi,
               const rt_upscale_params* params, float* rgba_out, float* sigma_out)
{
    rtk::UpArgs A;
    if (int r = upscale_ready(c, "rt_upscale", w_lo, h_lo, w, h, rgba_lo, sigma_lo, albedo_lo, normal_depth_lo, albedo_hi,
                              normal_depth_hi, params, rgba_out, sigma_out, false, A))
        return r;
    return rt_backend_upscale(c, A, rgba_out, sigma_out, false, nullptr);
}

int rt_upscale_device(rt_context* c, int w_lo, int h_lo, int w, int h, const void* rgba_lo, const void* sigma_lo,
                      const void* albedo_lo, const void* normal_depth_lo, const void* albedo_hi, const void* normal_depth_hi,
                      const rt_upscale_params* params, void* rgba_out, void* sigma_out, void* stream)
{
    rtk::UpArgs A;
    if (int r = upscale_ready(c, "rt_upscale_device", w_lo, h_lo, w, h, rgba_lo, sigma_lo, albedo_lo, normal_depth_lo,
                              albedo_hi, normal_depth_hi, params, rgba_out, sigma_out, true, A))
        return r;
    return rt_backend_upscale(c, A, rgba_out, sigma_out, true, stream);
}

// ---- bloom (rt_bloom.h)
// The usual starting point, not a measured optimum: everything above display white glows, with a soft knee
// half a unit wide, a fifth of the spread energy added back, five levels.
void rt_bloom_default_params(rt_bloom_params* p)
{
    if (!p) return;
    p->threshold = 1.0f;
    p->knee = 0.5f;
    p->intensity = 0.2f;
    p->levels = 5;
}

static int bloom_ready(rt_context* c, const char* fn, int w, int h, const void* in, const rt_bloom_params* params,
                       const void* out, const void* layer_out, bool device, rtk::BloomArgs& A)
{
    const size_t n = (size_t)w * h;
    const StageArgs a{c, fn, device,
                      {{in, 16 * n, SA_IN, SA_REQ, 16}, {out, 16 * n, SA_OUT, SA_REQ, 16}, {layer_out, 16 * n, SA_OUT, SA_OPT, 16}}};
    if (!c) return a.fail(": ctx is NULL");
    if (w <= 0 || h <= 0) return a.fail(": w and h must be at least 1");
    if (a.missing()) return a.fail(": linear_rgba or rgba_out is NULL");
    // (the composite tiles the frame 4 rows per block, as rt_denoise's kernels do)
    if (int r = a.frame_limits(w, h, true)) return r;
    const rt_bloom_params p = params_or_defaults(params, rt_bloom_default_params);
    if (p.levels < 1 || p.levels > rtk::BL_MAX_LEVELS) return a.fail(": levels must be 1..8");
    if (!std::isfinite(p.threshold) || !(p.threshold >= 0.0f)) return a.fail(": threshold is not finite and >= 0");
    if (!std::isfinite(p.knee) || !(p.knee >= 0.0f)) return a.fail(": knee is not finite and >= 0");
    if (!std::isfinite(p.intensity) || !(p.intensity >= 0.0f)) return a.fail(": intensity is not finite and >= 0");
    if (p.knee > p.threshold) return a.fail(": knee is above threshold");
    if (int r = a.overlap()) return r;
    if (int r = a.aligned(": the buffers must be 16-byte aligned")) return r;
    A = rtk::BloomArgs{w, h, p.levels, p.threshold, p.knee, p.intensity / (float)p.levels, (const float4_*)in};
    return RT_OK;
}

int rt_bloom(rt_context* c, int w, int h, const float* linear, const rt_bloom_params* params, float* out, float* layer_out)
{
    rtk::BloomArgs A;
    if (int r = bloom_ready(c, "rt_bloom", w, h, linear, params, out, layer_out, false, A)) return r;
    return rt_backend_bloom(c, A, out, layer_out, false, nullptr);
}

int rt_bloom_device(rt_context* c, int w, int h, const void* d_linear, const rt_bloom_params* params, void* d_out,
                    void* d_layer_out, void* stream)
{
    rtk::BloomArgs A;
    if (int r = bloom_ready(c, "rt_bloom_device", w, h, d_linear, params, d_out, d_layer_out, true, A)) return r;
    return rt_backend_bloom(c, A, d_out, d_layer_out, true, stream);
}

// ---- depth of field (rt_dof.h)
// A starting point, not a measured optimum: the focus distance is the scene's to choose (rt_amd.focus_at), a point at
// infinity blurs to a disc of 4 pixels' radius, and the window covers twice that.
void rt_dof_default_params(rt_dof_params* p)
{
    if (!p) return;
    p->focus = 1.0f;
    p->coc_inf = 4.0f;
    p->max_radius = 8;
}

static int dof_ready(rt_context* c, const char* fn, int w, int h, const void* in, const void* nd, const rt_dof_params* params,
                     const void* out, const void* coc_out, bool device, rtk::DofArgs& A)
{
    const size_t n = (size_t)w * h;
    const StageArgs a{c, fn, device,
                      {{in, 16 * n, SA_IN, SA_REQ, 16}, {nd, 16 * n, SA_IN, SA_REQ, 16}, {out, 16 * n, SA_OUT, SA_REQ, 16},
                       {coc_out, 4 * n, SA_OUT, SA_OPT, 4}}};
    if (!c) return a.fail(": ctx is NULL");
    if (w <= 0 || h <= 0) return a.fail(": w and h must be at least 1");
    if (a.missing()) return a.fail(": linear_rgba, normal_depth or rgba_out is NULL");
    // (k_dof_direct tiles the frame 4 rows per block, as rt_denoise's kernels do)
    if (int r = a.frame_limits(w, h, true)) return r;
    const rt_dof_params p = params_or_defaults(params, rt_dof_default_params);
    if (p.max_radius < 1 || p.max_radius > rtk::DOF_MAX_RADIUS) return a.fail(": max_radius must be 1..12");
    if (!std::isfinite(p.focus) || !(p.focus > 0.0f)) return a.fail(": focus is not finite and > 0");
    if (!std::isfinite(p.coc_inf) || !(p.coc_inf >= 0.0f)) return a.fail(": coc_inf is not finite and >= 0");
    if (int r = a.overlap()) return r;
    if (int r = a.aligned()) return r;
    A = rtk::DofArgs{w, h, p.max_radius, p.focus, p.coc_inf, (const float4_*)in, (const float4_*)nd, {}};
    rtk::dof_build_table(A.D);
    return RT_OK;
}

int rt_dof(rt_context* c, int w, int h, const float* linear, const float* normal_depth, const rt_dof_params* params, float* out,
           float* coc_out)
{
    rtk::DofArgs A;
    if (int r = dof_ready(c, "rt_dof", w, h, linear, normal_depth, params, out, coc_out, false, A)) return r;
    return rt_backend_dof(c, A, out, coc_out, false, nullptr);
}

int rt_dof_device(rt_context* c, int w, int h, const void* d_linear, const void* d_normal_depth, const rt_dof_params* params,
                  void* d_out, void* d_coc_out, void* stream)
{
    rtk::DofArgs A;
    if (int r = dof_ready(c, "rt_dof_device", w, h, d_linear, d_normal_depth, params, d_out, d_coc_out, true, A)) return r;
    return rt_backend_dof(c, A, d_out, d_coc_out, true, stream);
}

// ---- motion vectors and motion blur (rt_motion.h)
// A starting point, not a measured optimum: a 180-degree shutter, SVGF's relative depth width (rt_temporal's
// depth_tol) for the fade between fore and back, and streaks of at most 8 pixels either way.
void rt_motion_default_params(rt_motion_params* p)
{
    if (!p) return;
    p->shutter = 0.5f;
    p->depth_soft = 0.05f;
    p->max_radius = 8;
}

// The camera part of a vectors call, rt_temporal_accumulate's: the current view, the previous camera's inverse and origin.
static int motion_camera(const StageArgs& a, rt_context* c, int w, int h, const float* prev_view, float prev_fov, rtk::MotionVecArgs& A)
{
    if (!std::isfinite(prev_fov) || prev_fov == 0.0f) return a.fail(": prev_fov_dist is zero or not finite");
    A.cur = rtk::cam_view(c->cam, w, h);
    if (!invert_view(prev_view, A.prev_inv.m)) return a.fail(": prev_view is singular or not finite");
    A.prev_inv.fov_dist = prev_fov;
    RtCamera prev;
    std::memcpy(prev.m, prev_view, 64);
    prev.fov_dist = prev_fov;
    const rtk::V3 op = rtk::xform_point(prev, rtk::v3(0.0f, 0.0f, 0.0f));
    A.o_prev[0] = op.x, A.o_prev[1] = op.y, A.o_prev[2] = op.z;
    return RT_OK;
}

static int motion_vectors_ready(rt_context* c, const char* fn, int w, int h, const void* nd, const float* prev_view, float prev_fov,
                                const void* out, bool device, rtk::MotionVecArgs& A)
{
    const size_t n = (size_t)w * h;
    const StageArgs a{c, fn, device, {{nd, 16 * n, SA_IN, SA_REQ, 16}, {out, 8 * n, SA_OUT, SA_REQ, 8}}};
    if (!c) return a.fail(": ctx is NULL");
    if (!c->have_cam) return a.fail(": camera not set", RT_ERR_STATE);
    if (w <= 0 || h <= 0 || a.missing() || !prev_view) return a.fail(": bad buffers");
    if (int r = a.frame_limits(w, h, true)) return r;
    if (!std::isfinite(prev_fov) || prev_fov == 0.0f) return a.fail(": prev_fov_dist is zero or not finite");
    if (int r = a.overlap()) return r;
    if (int r = a.aligned(": normal_depth must be 16-byte aligned, motion_out 8-byte aligned")) return r;
    if (int r = motion_camera(a, c, w, h, prev_view, prev_fov, A)) return r;
    A.nd = (const float4_*)nd;
    return RT_OK;
}

int rt_motion_vec_args(rt_context* c, int w, int h, const void* nd, const float* prev_view, float prev_fov, rtk::MotionVecArgs& A)
{
    const StageArgs a{c, "rt_motion_vec_args", true, {}};
    if (int r = motion_camera(a, c, w, h, prev_view, prev_fov, A)) return r;
    A.nd = (const float4_*)nd;
    return RT_OK;
}

int rt_motion_vectors(rt_context* c, int w, int h, const float* normal_depth, const float prev_view[16], float prev_fov_dist,
                      float* motion_out)
{
    rtk::MotionVecArgs A;
    if (int r = motion_vectors_ready(c, "rt_motion_vectors", w, h, normal_depth, prev_view, prev_fov_dist, motion_out, false, A)) return r;
    return rt_backend_motion_vectors(c, A, motion_out, false, nullptr);
}

int rt_motion_vectors_device(rt_context* c, int w, int h, const void* d_normal_depth, const float prev_view[16], float prev_fov_dist,
                             void* d_motion_out, void* stream)
{
    rtk::MotionVecArgs A;
    if (int r = motion_vectors_ready(c, "rt_motion_vectors_device", w, h, d_normal_depth, prev_view, prev_fov_dist, d_motion_out, true, A))
        return r;
    return rt_backend_motion_vectors(c, A, d_motion_out, true, stream);
}

static int motion_ready(rt_context* c, const char* fn, int w, int h, const void* in, const void* nd, const void* motion,
                        const rt_motion_params* params, const void* out, const void* reach_out, bool device, rtk::MotionArgs& A)
{
    const size_t n = (size_t)w * h;
    const StageArgs a{c, fn, device,
                      {{in, 16 * n, SA_IN, SA_REQ, 16}, {nd, 16 * n, SA_IN, SA_REQ, 16}, {motion, 8 * n, SA_IN, SA_REQ, 8},
                       {out, 16 * n, SA_OUT, SA_REQ, 16}, {reach_out, 4 * n, SA_OUT, SA_OPT, 4}}};
    if (!c) return a.fail(": ctx is NULL");
    if (w <= 0 || h <= 0) return a.fail(": w and h must be at least 1");
    if (a.missing()) return a.fail(": linear_rgba, normal_depth, motion or rgba_out is NULL");
    if (int r = a.frame_limits(w, h, true)) return r;
    const rt_motion_params p = params_or_defaults(params, rt_motion_default_params);
    if (p.max_radius < 1 || p.max_radius > rtk::MB_MAX_RADIUS) return a.fail(": max_radius must be 1..16");
    if (!(p.shutter >= 0.0f && p.shutter <= 1.0f)) return a.fail(": shutter is outside [0, 1]");
    if (!std::isfinite(p.depth_soft) || !(p.depth_soft > 0.0f)) return a.fail(": depth_soft is not finite and > 0");
    if (int r = a.overlap()) return r;
    if (int r = a.aligned(": the float4 buffers must be 16-byte aligned, motion 8-byte aligned, reach_out 4-byte aligned")) return r;
    A = rtk::MotionArgs{w, h, p.max_radius, 0.5f * p.shutter, p.depth_soft, (const float4_*)in, (const float4_*)nd,
                        (const rtk::MbVec*)motion};
    return RT_OK;
}

int rt_motion_blur(rt_context* c, int w, int h, const float* linear, const float* normal_depth, const float* motion,
                   const rt_motion_params* params, float* out, float* reach_out)
{
    rtk::MotionArgs A;
    if (int r = motion_ready(c, "rt_motion_blur", w, h, linear, normal_depth, motion, params, out, reach_out, false, A)) return r;
    return rt_backend_motion_blur(c, A, out, reach_out, false, nullptr);
}

int rt_motion_blur_device(rt_context* c, int w, int h, const void* d_linear, const void* d_normal_depth, const void* d_motion,
                          const rt_motion_params* params, void* d_out, void* d_reach_out, void* stream)
{
    rtk::MotionArgs A;
    if (int r = motion_ready(c, "rt_motion_blur_device", w, h, d_linear, d_normal_depth, d_motion, params, d_out, d_reach_out, true, A))
        return r;
    return rt_backend_motion_blur(c, A, d_out, d_reach_out, true, stream);
}

// ---- exposure metering (rt_meter.h)
// The photographic convention (a log-average that displays as middle grey, 0.18), not a measured optimum;
// the trims keep a dark corner and the light source out of the average.
void rt_meter_default_params(rt_meter_params* p)
{
    if (!p) return;
    p->low = 0.10f;
    p->high = 0.95f;
    p->key = 0.18f;
    p->min_exposure = 0x1p-8f;
    p->max_exposure = 0x1p12f;
    p->tau_up = 0.0f;
    p->tau_down = 0.0f;
}

static int meter_ready(rt_context* c, const char* fn, int w, int h, const void* in, const void* hist, bool device)
{
    const StageArgs a{c, fn, device, {{in, 0, SA_IN, SA_REQ, 16}, {hist, 0, SA_OUT, SA_REQ, 4}}};
    if (!c) return a.fail(": ctx is NULL");
    if (w <= 0 || h <= 0) return a.fail(": w and h must be at least 1");
    if (a.missing()) return a.fail(": the frame or the histogram is NULL");
    // (rt_display's limit, no row limit; with it no word of the histogram can overflow. No overlap rule.)
    if (int r = a.frame_limits(w, h, false)) return r;
    return a.aligned(": d_linear must be 16-byte aligned, d_hist 4-byte aligned");
}

int rt_meter(rt_context* c, int w, int h, const float* linear, rt_meter_hist* out)
{
    static_assert(sizeof(rt_meter_hist) == rtk::MT_WORDS * sizeof(uint32_t), "rt_meter_hist is MT_WORDS words");
    if (int r = meter_ready(c, "rt_meter", w, h, linear, out, false)) return r;
    return rt_backend_meter(c, w, h, linear, out, false, nullptr);
}

int rt_meter_device(rt_context* c, int w, int h, const void* d_linear, void* d_hist, void* stream)
{
    if (int r = meter_ready(c, "rt_meter_device", w, h, d_linear, d_hist, true)) return r;
    return rt_backend_meter(c, w, h, d_linear, d_hist, true, stream);
}

// Host only, in double: the formulas of include/rt_hip.h, in their order.
int rt_meter_solve(const rt_meter_hist* hist, const rt_meter_params* params, float prev_exposure, float dt_seconds,
                   rt_meter_result* out)
{
    const std::string f = "rt_meter_solve";
    if (!hist || !out) return rt_fail(nullptr, RT_ERR_ARG, f + ": the histogram or the result is NULL");
    const rt_meter_params p = params_or_defaults(params, rt_meter_default_params);
    if (!(p.low >= 0.0f && p.low <= 1.0f) || !(p.high >= 0.0f && p.high <= 1.0f) || p.low > p.high)
        return rt_fail(nullptr, RT_ERR_ARG, f + ": low and high must lie in [0, 1] with low <= high");
    if (!(p.key > 0.0f && p.key < 1.0f)) return rt_fail(nullptr, RT_ERR_ARG, f + ": key must lie in (0, 1)");
    if (!std::isfinite(p.min_exposure) || !std::isfinite(p.max_exposure) || !(p.min_exposure > 0.0f) ||
        p.min_exposure > p.max_exposure)
        return rt_fail(nullptr, RT_ERR_ARG, f + ": the exposure bounds must be finite, positive and ordered");
    if (!(p.tau_up >= 0.0f) || !(p.tau_down >= 0.0f))
        return rt_fail(nullptr, RT_ERR_ARG, f + ": tau_up or tau_down is negative or a NaN");
    const double n = (double)hist->counted, prev = (double)prev_exposure, dt = (double)dt_seconds;
    double lo = std::floor((double)p.low * n), hi = std::floor((1.0 - (double)p.high) * n);
    if (lo + hi >= n) lo = hi = 0.0;
    uint64_t c[256];
    for (int b = 0; b < 256; b++) c[b] = hist->bins[b];
    uint64_t cut = (uint64_t)lo;
    for (int b = 0; b < 256 && cut; b++) {
        const uint64_t d = std::min(cut, c[b]);
        c[b] -= d, cut -= d;
    }
    cut = (uint64_t)hi;
    for (int b = 255; b >= 0 && cut; b--) {
        const uint64_t d = std::min(cut, c[b]);
        c[b] -= d, cut -= d;
    }
    uint64_t N = 0;
    int64_t S = 0;
    for (int b = 0; b < 256; b++) N += c[b], S += (int64_t)c[b] * (2 * b - 319);
    if (N == 0) {
        const float e = prev_exposure > 0.0f ? prev_exposure : 1.5f;
        *out = rt_meter_result{e, e, 0.0f, 0};
        return RT_OK;
    }
    const double log2_mean = (double)S / (16.0 * (double)N);
    const double Lm = std::exp2(log2_mean);
    const double target = std::min(std::max(-std::log1p(-(double)p.key) / Lm, (double)p.min_exposure), (double)p.max_exposure);
    const double tau = (double)(target > prev ? p.tau_up : p.tau_down);
    double e = target;
    if (prev > 0.0 && tau > 0.0 && dt >= 0.0) {
        const double l0 = std::log2(prev);
        e = std::exp2(l0 + (std::log2(target) - l0) * (1.0 - std::exp(-dt / tau)));
    }
    *out = rt_meter_result{(float)e, (float)target, (float)log2_mean, 1};
    return RT_OK;
}

// ---------------------------------------------------------- display stage
// The reference's literals (render_kernel.cpp:175, :178).
void rt_display_default_params(rt_display_params* p)
{
    if (!p) return;
    p->exposure = 1.5f;
    p->gamma = 2.2f;
    p->flip_y = 0;
}

static int display_ready(rt_context* c, const char* fn, int w, int h, const void* in, const rt_display_params* params,
                         const void* out, const void* out8, bool device, rt_display_params& p)
{
    const size_t n = (size_t)w * h;
    const StageArgs a{c, fn, device,
                      {{in, 16 * n, SA_IN, SA_REQ, 16}, {out, 16 * n, SA_OUT, SA_OPT, 16}, {out8, 4 * n, SA_OUT, SA_OPT, 4}}};
    if (!c) return a.fail(": ctx is NULL");
    if (w <= 0 || h <= 0 || a.missing()) return a.fail(": bad buffers");
    if (int r = a.frame_limits(w, h, false)) return r;
    if (!out && !out8) return a.fail(": rgba_out and rgba8_out are both NULL");
    // The stage's own overlap rule, not a.overlap(): the float output may be the input, pixel for pixel, or lies
    // apart from it (a partial overlap would read pixels already written); a pixel's bytes land at another pixel's place.
    if (out8 && ranges_overlap(out8, 4 * n, in, 16 * n)) return a.fail(": rgba8_out overlaps the input");
    if (out8 && out && ranges_overlap(out8, 4 * n, out, 16 * n)) return a.fail(": rgba8_out overlaps rgba_out");
    if (out && out != in && ranges_overlap(out, 16 * n, in, 16 * n)) return a.fail(": rgba_out overlaps the input without being it");
    // (k_display moves a pixel with one 16-byte load / store and its bytes with one 4-byte store;
    // the host form copies through buffers of its own and takes any alignment)
    if (int r = a.aligned(": d_linear and d_rgba_out must be 16-byte aligned, d_rgba8_out 4-byte aligned")) return r;
    p = params_or_defaults(params, rt_display_default_params);
    if (!std::isfinite(p.exposure)) return a.fail(": the exposure is not finite");
    if (!std::isfinite(p.gamma) || !(p.gamma > 0.0f)) return a.fail(": the gamma is not finite and > 0");
    return RT_OK;
}

int rt_display(rt_context* c, int w, int h, const float* linear, const rt_display_params* params, float* out,
               unsigned char* out8)
{
    rt_display_params p;
    if (int r = display_ready(c, "rt_display", w, h, linear, params, out, out8, false, p)) return r;
    // (an IEEE division at run time: at 2.2f it is the float the literal 1.0f / 2.2f of tonemap_pixel is)
    return rt_backend_display(c, w, h, linear, p.exposure, 1.0f / p.gamma, p.flip_y != 0, out, out8, false, nullptr);
}

int rt_display_device(rt_context* c, int w, int h, const void* d_linear, const rt_display_params* params, void* d_out,
                      void* d_out8, void* stream)
{
    rt_display_params p;
    if (int r = display_ready(c, "rt_display_device", w, h, d_linear, params, d_out, d_out8, true, p)) return r;
    return rt_backend_display(c, w, h, d_linear, p.exposure, 1.0f / p.gamma, p.flip_y != 0, d_out, d_out8, true, stream);
}
