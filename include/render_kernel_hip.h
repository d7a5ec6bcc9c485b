// render_kernel_hip.h — header-only C++ drop-in for the reference's RenderKernel
// (TomClabault/SYCL-ray-tracing include/render_kernel.h:21-96), forwarding to the
// C ABI of librt_hip.so (include/rt_hip.h).
//
// Include it INSTEAD of render_kernel.h, with the reference's include/ on the
// include path (it uses the reference's Triangle, SimpleMaterial, Sphere, BVH,
// Image, Camera types), and link -lrt_hip. Same constructor signature
// (render_kernel.h:24-46), set_camera (:48), render (:57, render_kernel.cpp:189-211)
// and ray_trace_pixel (:56, render_kernel.cpp:75-181).
//
// Semantics kept from the reference:
//  * the kernel holds REFERENCES to the caller's buffers (render_kernel.h:81-93):
//    the material vector is re-read on every render() / ray_trace_pixel() and
//    pushed with rt_set_materials when it changed (the cfg5 material sweep edits
//    it between renders without an octree rebuild). The triangles, the BVH& (handed
//    over as a pre-order walk of BVH::_root, so the GPU walks the caller's tree),
//    the sky and its CDF are bound at construction, as a rebuilt BVH would be.
//  * render() mutates the Image& in place: fb += sample average, then the tone-map
//    (render_kernel.cpp:167-180), alpha included.
// Differences: errors throw std::runtime_error (the reference's class has none);
// the devices are chosen by the trailing `device_count` argument or RT_DEVICES
// (default 1): N > 1 shards the frame's rows over devices 0..N-1 with RCCL
// (rt_create_multi), bit-identical to one device.
#ifndef RENDER_KERNEL_HIP_H
#define RENDER_KERNEL_HIP_H

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rt_hip.h"

#include "bvh.h"
#include "camera.h"
#include "image.h"
#include "simple_material.h"
#include "sphere.h"
#include "triangle.h"

class RenderKernel {
public:
    RenderKernel(int width, int height, int render_samples, int max_bounces, Image& image_buffer,
                 const std::vector<Triangle>& triangle_buffer, const std::vector<SimpleMaterial>& materials_buffer,
                 const std::vector<int>& emissive_triangle_indices_buffer,
                 const std::vector<int>& materials_indices_buffer, const std::vector<Sphere>& analytic_spheres_buffer,
                 BVH& bvh, const Image& skysphere, const std::vector<float>& env_map_cdf, int device_count = 0)
        : m_width(width), m_height(height), m_render_samples(render_samples), m_max_bounces(max_bounces),
          m_frame_buffer(image_buffer), m_materials_buffer(materials_buffer)
    {
        static_assert(sizeof(Triangle) == 9 * sizeof(float), "Triangle is 3 Points (triangle.h:67)");
        static_assert(sizeof(SimpleMaterial) == 10 * sizeof(float), "SimpleMaterial is 2 Colors + 2 floats");
        if (device_count <= 0) {
            const char* e = std::getenv("RT_DEVICES");
            device_count = e ? std::atoi(e) : 1;
        }
        if (device_count > 1)
            check(rt_create_multi(device_count, nullptr, &m_ctx));
        else
            check(rt_create(0, &m_ctx));
        std::vector<float> sph;
        for (const Sphere& s : analytic_spheres_buffer)
            sph.insert(sph.end(), {s.center.x, s.center.y, s.center.z, s.radius, (float)s.primitive_index});
        check(rt_set_scene(m_ctx, reinterpret_cast<const float*>(triangle_buffer.data()), (int)triangle_buffer.size(),
                           materials_indices_buffer.data(), (int)materials_indices_buffer.size(),
                           reinterpret_cast<const float*>(materials_buffer.data()), (int)materials_buffer.size(),
                           emissive_triangle_indices_buffer.data(), (int)emissive_triangle_indices_buffer.size(),
                           sph.data(), (int)analytic_spheres_buffer.size()));
        m_materials_sent = materials_bytes();
        // the caller's octree (BVH::_root is public, bvh.h:276-279), as a pre-order walk
        std::vector<char> dump;
        preorder(bvh._root, dump);
        check(rt_set_bvh_preorder(m_ctx, dump.data(), (long)dump.size()));
        check(rt_set_env(m_ctx, skysphere.data(), skysphere.width(), skysphere.height(), 4,
                         env_map_cdf.empty() ? nullptr : env_map_cdf.data()));
    }

    ~RenderKernel() { rt_destroy(m_ctx); }
    RenderKernel(const RenderKernel&) = delete;
    RenderKernel& operator=(const RenderKernel&) = delete;

    void set_camera(Camera camera)  // render_kernel.h:48
    {
        check(rt_set_camera(m_ctx, &camera.view_matrix.m[0][0], camera.fov_dist));
    }

    void render()  // render_kernel.cpp:189-211
    {
        std::lock_guard<std::mutex> lk(m_mu);
        sync_materials();
        check(rt_render(m_ctx, m_width, m_height, m_render_samples, m_max_bounces, m_frame_buffer.data()));
    }

    // render() without its tone-map (rt_render_linear): the Image& ends as entry.rgb +
    // final_color / samples with the entry alpha, the reference's hdrColor (render_kernel.cpp:173).
    // display() of it at the defaults is what render() would have left, bit for bit.
    void render_linear()
    {
        std::lock_guard<std::mutex> lk(m_mu);
        sync_materials();
        check(rt_render_linear(m_ctx, m_width, m_height, m_render_samples, m_max_bounces, m_frame_buffer.data()));
    }

    // The exposure / gamma tone-map of render_kernel.cpp:171-180 on a linear frame of any size
    // (rt_display): a new Image. The reference's literals are the defaults.
    Image display(const Image& linear, float exposure = 1.5f, float gamma = 2.2f) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        rt_display_params p;
        rt_display_default_params(&p);
        p.exposure = exposure;
        p.gamma = gamma;
        Image out(linear.width(), linear.height());
        check(rt_display(m_ctx, linear.width(), linear.height(), linear.data(), &p, out.data(), nullptr));
        return out;
    }

    // Exposure metering (rt_meter): the log-luminance histogram of a linear frame of any size, 256
    // bins of an eighth of an octave and the stat words. It needs no scene state and does not render.
    rt_meter_hist meter(const Image& linear) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        rt_meter_hist hist;
        check(rt_meter(m_ctx, linear.width(), linear.height(), linear.data(), &hist));
        return hist;
    }

    // meter(), then rt_meter_solve: the exposure display() should take for this frame. prev: the
    // last frame's exposure (<= 0: none) and dt the seconds since, for params' tau_up / tau_down
    // (null: the defaults, which jump to the target). result, when given, receives the whole answer.
    float auto_exposure(const Image& linear, float prev = 0.0f, float dt = 0.0f, const rt_meter_params* params = nullptr,
                        rt_meter_result* result = nullptr) const
    {
        const rt_meter_hist hist = meter(linear);
        rt_meter_result r;
        check(rt_meter_solve(&hist, params, prev, dt, &r));
        if (result) *result = r;
        return r.exposure;
    }

    // write_image_hdr (image_io.h:20, image_io.cpp:208-214) through rt_write_hdr: the rgb channels
    // as a Radiance RGBE file. A member, so that it does not collide with the reference's own
    // function when image_io.h is included too.
    static bool write_image_hdr(const Image& image, const char* filename, const bool flipY = true)
    {
        if (image.width() * image.height() == 0) return false;
        check(rt_write_hdr(filename, image.data(), image.width(), image.height(), flipY ? 1 : 0));
        return true;
    }

    // render() in passes of pass_samples samples (rt_progress_*): the Image& is the base the
    // frame adds to, and after each pass it holds the image so far and on_pass(image, done,
    // total) is called; returning false stops the progression there. After the last pass the
    // Image& holds what render() would have left, bit for bit. Before that it is a preview: the
    // mean of the first `done` samples of the render_samples chain (the reference seeds a pixel
    // with its sample count), not the frame a render of `done` samples gives. Single device only.
    template <class F>
    void render_progressive(int pass_samples, F&& on_pass)
    {
        std::lock_guard<std::mutex> lk(m_mu);
        sync_materials();
        check(rt_progress_begin(m_ctx, m_width, m_height, m_render_samples, m_max_bounces, m_frame_buffer.data(), 0, 1));
        if (m_track) check(rt_progress_noise_track(m_ctx));
        for (int done = 0; done < m_render_samples;) {
            int info[8];
            if (rt_progress_advance(m_ctx, pass_samples, nullptr) != RT_OK ||
                rt_progress_resolve(m_ctx, m_frame_buffer.data()) != RT_OK || rt_progress_info(m_ctx, info) != RT_OK) {
                const std::string err = std::string("librt_hip: ") + rt_last_error(nullptr);
                rt_progress_end(m_ctx);
                throw std::runtime_error(err);
            }
            done = info[3];
            if (!on_pass(static_cast<const Image&>(m_frame_buffer), done, m_render_samples)) break;
        }
        rt_progress_end(m_ctx);
    }

    // The noise estimate of a progression (rt_progress_noise_track, rt_progress_noise), for the
    // on_pass callback of render_progressive_tracked below. progress_track_noise: while a
    // progression has no sample yet (render_progressive_tracked calls it). progress_noise: after at
    // least two passes; stats.tiles_over == 0 means every 8x8 tile's error is at or below the
    // threshold. Neither takes the kernel's lock: on_pass runs under it.
    // context(): the C ABI's handle, for the calls the class does not wrap (rt_progress_noise's pixel
    // and tile maps, the device forms); on_pass may use it, other threads must not meanwhile.
    rt_context* context() const { return m_ctx; }
    void progress_track_noise() { check(rt_progress_noise_track(m_ctx)); }
    void progress_noise(float threshold, rt_noise_stats& stats) const
    {
        check(rt_progress_noise(m_ctx, threshold, &stats, nullptr, nullptr));
    }

    // render_progressive with the progression tracked: on_pass may call progress_noise from the
    // second pass on and return false to stop at a threshold.
    template <class F>
    void render_progressive_tracked(int pass_samples, F&& on_pass)
    {
        m_track = true;
        try {
            render_progressive(pass_samples, std::forward<F>(on_pass));
        } catch (...) {
            m_track = false;
            throw;
        }
        m_track = false;
    }

    // render() with the samples spent where the noise is (rt_progress_advance_adaptive): two uniform
    // passes of pass_samples, then passes that advance only the 8x8 tiles whose noise estimate is
    // above `threshold`, until none is (or none fits under render_samples any more: keep
    // render_samples a multiple of pass_samples), or after max_passes adaptive passes (0: no limit).
    // The Image& then holds every pixel's mean over its tile's samples, added to the base it held.
    // Returns tile_n, the samples per tile, ceil(height / 8) rows of ceil(width / 8). A pixel whose
    // tile has c samples is what render_progressive shows it to be after c samples. Single device only.
    std::vector<int> render_adaptive(float threshold, int pass_samples, int max_passes = 0)
    {
        std::lock_guard<std::mutex> lk(m_mu);
        sync_materials();
        check(rt_progress_begin(m_ctx, m_width, m_height, m_render_samples, m_max_bounces, m_frame_buffer.data(), 0, 1));
        std::vector<int> tile_n((size_t)((m_width + 7) / 8) * ((m_height + 7) / 8));
        int rc = rt_progress_noise_track(m_ctx);
        for (int p = 0; rc == RT_OK && p < 2; p++) rc = rt_progress_advance(m_ctx, pass_samples, nullptr);
        for (int p = 0; rc == RT_OK && (max_passes <= 0 || p < max_passes); p++) {
            int info[8];
            rc = rt_progress_advance_adaptive(m_ctx, pass_samples, threshold, nullptr, info);
            if (rc != RT_OK || info[0] == 0) break;
        }
        if (rc == RT_OK) rc = rt_progress_resolve(m_ctx, m_frame_buffer.data());
        if (rc == RT_OK) rc = rt_progress_tile_counts(m_ctx, tile_n.data(), nullptr);
        const std::string err = rc == RT_OK ? std::string() : std::string("librt_hip: ") + rt_last_error(nullptr);
        rt_progress_end(m_ctx);
        if (rc != RT_OK) throw std::runtime_error(err);
        return tile_n;
    }

    // Thread-safe like the reference's (whose render() calls it from an OpenMP parallel-for,
    // render_kernel.cpp:189-211): calls on one kernel are serialized, since they share the
    // context's device buffers and the material-sync state. For throughput, hand pixel
    // batches to rt_render_pixels (or call render()) instead of one pixel per call.
    void ray_trace_pixel(int x, int y) const  // render_kernel.cpp:75-181
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const_cast<RenderKernel*>(this)->sync_materials();
        const int xy[2] = {x, y};
        Color& px = m_frame_buffer.color_data()[y * m_width + x];
        check(rt_render_pixels(m_ctx, m_width, m_height, m_render_samples, m_max_bounces, xy, 1,
                               reinterpret_cast<float*>(&px)));
    }

    // The call shape of Utils::OIDN_denoise(image, blend_factor) (utils.cpp:144-196): a new
    // Image, blend_factor * filtered + (1 - blend_factor) * image, alpha 1. The filter is the
    // edge-avoiding a-trous of rt_denoise with its default parameters, guided by the first-hit
    // buffers rendered for the bound camera (image has the kernel's size).
    Image denoise(const Image& image, float blend_factor) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const_cast<RenderKernel*>(this)->sync_materials();
        const int w = image.width(), h = image.height();
        std::vector<float> albedo((size_t)w * h * 4), normal_depth((size_t)w * h * 4);
        check(rt_render_features(m_ctx, w, h, albedo.data(), normal_depth.data()));
        Image out(w, h);
        check(rt_denoise(m_ctx, w, h, image.data(), albedo.data(), normal_depth.data(), nullptr, blend_factor,
                         out.data()));
        return out;
    }

    // denoise() with the colour edge-stop scaled per pixel by sigma (rt_denoise_var with its default
    // parameters): sigma holds width * height standard deviations of the image's colour, such as
    // progress_noise_sigma() gives for the linear frame of a tracked progression (from the on_pass
    // callback of render_progressive_tracked, after at least two passes; it does not take the
    // kernel's lock: on_pass runs under it). sigma_out, when given, receives the standard deviation
    // left in the filtered colour.
    std::vector<float> progress_noise_sigma() const
    {
        std::vector<float> sigma((size_t)m_width * m_height);
        check(rt_progress_noise_sigma(m_ctx, sigma.data()));
        return sigma;
    }
    Image denoise_var(const Image& image, const std::vector<float>& sigma, float blend_factor,
                      std::vector<float>* sigma_out = nullptr) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const_cast<RenderKernel*>(this)->sync_materials();
        const int w = image.width(), h = image.height();
        if (sigma.size() != (size_t)w * h) throw std::runtime_error("librt_hip: denoise_var: sigma is not width * height floats");
        std::vector<float> albedo((size_t)w * h * 4), normal_depth((size_t)w * h * 4);
        check(rt_render_features(m_ctx, w, h, albedo.data(), normal_depth.data()));
        if (sigma_out) sigma_out->assign((size_t)w * h, 0.0f);
        Image out(w, h);
        check(rt_denoise_var(m_ctx, w, h, image.data(), sigma.data(), albedo.data(), normal_depth.data(), nullptr,
                             blend_factor, out.data(), sigma_out ? sigma_out->data() : nullptr));
        return out;
    }

    // Temporal accumulation (rt_temporal_accumulate with its default parameters): the history of the
    // previous frame, rendered under prev_camera, reprojected into the kernel's current camera and
    // blended with `linear` (a linear frame, as render_linear leaves it) whose per-pixel standard
    // deviation is sigma (progress_noise_sigma()). The feature pass runs under the current camera.
    // history: the previous call's result, or null for the first frame. The result's rgba and sigma
    // are what denoise_var takes; the whole result is the next call's history.
    struct TemporalFrame {
        Image rgba;
        std::vector<float> sigma, length, normal_depth;
    };
    TemporalFrame temporal_accumulate(const Image& linear, const std::vector<float>& sigma, Camera prev_camera,
                                      const TemporalFrame* history = nullptr) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const_cast<RenderKernel*>(this)->sync_materials();
        const int w = linear.width(), h = linear.height();
        const size_t n = (size_t)w * h;
        if (sigma.size() != n) throw std::runtime_error("librt_hip: temporal_accumulate: sigma is not width * height floats");
        if (history && (history->rgba.width() != w || history->rgba.height() != h || history->sigma.size() != n ||
                        history->length.size() != n || history->normal_depth.size() != 4 * n))
            throw std::runtime_error("librt_hip: temporal_accumulate: the history is not of the frame's size");
        std::vector<float> albedo(n * 4);
        TemporalFrame out{Image(w, h), std::vector<float>(n), std::vector<float>(n), std::vector<float>(n * 4)};
        check(rt_render_features(m_ctx, w, h, albedo.data(), out.normal_depth.data()));
        check(rt_temporal_accumulate(m_ctx, w, h, linear.data(), sigma.data(), out.normal_depth.data(),
                                     &prev_camera.view_matrix.m[0][0], prev_camera.fov_dist,
                                     history ? history->rgba.data() : nullptr, history ? history->sigma.data() : nullptr,
                                     history ? history->length.data() : nullptr,
                                     history ? history->normal_depth.data() : nullptr, nullptr, out.rgba.data(),
                                     out.sigma.data(), out.length.data()));
        return out;
    }

    // Guided upscale (rt_upscale): `low`, a linear frame rendered by a kernel of low.width() x low.height()
    // under this kernel's camera, taken to width x height along the first-hit guides, which this call
    // renders at both sizes (as denoise() renders its own). sigma: the low frame's per-pixel standard
    // deviation (progress_noise_sigma() of the low-resolution kernel), carried into *sigma_out at the
    // output size, or empty for none (sigma_out must then be null). params: null for the defaults.
    Image upscale(const Image& low, int width, int height, const std::vector<float>& sigma,
                  const rt_upscale_params* params = nullptr, std::vector<float>* sigma_out = nullptr) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const_cast<RenderKernel*>(this)->sync_materials();
        const int wl = low.width(), hl = low.height();
        if (width < wl || height < hl) throw std::runtime_error("librt_hip: upscale: the output is smaller than the low frame");
        const size_t n_lo = (size_t)wl * hl, n = (size_t)width * height;
        if (!sigma.empty() && sigma.size() != n_lo)
            throw std::runtime_error("librt_hip: upscale: sigma is not low.width() * low.height() floats");
        if (sigma.empty() != (sigma_out == nullptr))
            throw std::runtime_error("librt_hip: upscale: sigma and sigma_out go together");
        std::vector<float> alb_lo(n_lo * 4), nd_lo(n_lo * 4), alb_hi(n * 4), nd_hi(n * 4);
        check(rt_render_features(m_ctx, wl, hl, alb_lo.data(), nd_lo.data()));
        check(rt_render_features(m_ctx, width, height, alb_hi.data(), nd_hi.data()));
        if (sigma_out) sigma_out->assign(n, 0.0f);
        Image out(width, height);
        check(rt_upscale(m_ctx, wl, hl, width, height, low.data(), sigma.empty() ? nullptr : sigma.data(), alb_lo.data(),
                         nd_lo.data(), alb_hi.data(), nd_hi.data(), params, out.data(),
                         sigma_out ? sigma_out->data() : nullptr));
        return out;
    }

    // upscale() without a noise figure.
    Image upscale(const Image& low, int width, int height, const rt_upscale_params* params = nullptr) const
    {
        return upscale(low, width, height, std::vector<float>(), params, nullptr);
    }

    // Firefly rejection (rt_firefly): every pixel of `image` (a linear frame) whose luminance is above
    // gain * M + floor, M the rank-th largest luminance among its neighbours, scaled down to that limit.
    // sigma: the frame's per-pixel standard deviation (progress_noise_sigma()), scaled with the colour
    // into *sigma_out, or empty for none (sigma_out must then be null). scale_out, when given, receives
    // the factor per pixel: below 1 where clamped. The result and *sigma_out are what temporal_accumulate
    // and denoise_var take. It needs no scene state and does not render.
    Image firefly_clamp(const Image& image, const std::vector<float>& sigma, const rt_firefly_params& params,
                        std::vector<float>* sigma_out = nullptr, std::vector<float>* scale_out = nullptr) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const int w = image.width(), h = image.height();
        const size_t n = (size_t)w * h;
        if (!sigma.empty() && sigma.size() != n)
            throw std::runtime_error("librt_hip: firefly_clamp: sigma is not width * height floats");
        if (sigma.empty() && sigma_out) throw std::runtime_error("librt_hip: firefly_clamp: sigma_out without a sigma");
        if (sigma_out) sigma_out->assign(n, 0.0f);
        if (scale_out) scale_out->assign(n, 0.0f);
        Image out(w, h);
        check(rt_firefly(m_ctx, w, h, image.data(), sigma.empty() ? nullptr : sigma.data(), &params, out.data(),
                         sigma_out ? sigma_out->data() : nullptr, scale_out ? scale_out->data() : nullptr));
        return out;
    }

    // Bloom (rt_bloom): the energy of `linear` above params' luminance threshold spread by a Gaussian pyramid
    // and added back; it goes between render_linear() or the last filter and display(). params: null for
    // the defaults. layer_out, when given, receives what was added, 4 floats per pixel {rgb, 0}. It needs
    // no scene state and does not render.
    Image bloom(const Image& linear, const rt_bloom_params* params = nullptr, std::vector<float>* layer_out = nullptr) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const int w = linear.width(), h = linear.height();
        if (layer_out) layer_out->assign((size_t)w * h * 4, 0.0f);
        Image out(w, h);
        check(rt_bloom(m_ctx, w, h, linear.data(), params, out.data(), layer_out ? layer_out->data() : nullptr));
        return out;
    }

    // Depth of field (rt_dof): a thin lens's blur built from `linear` and the first-hit distances of
    // normal_depth (4 floats per pixel, .w = t: features() or gbuffer() at the frame's size); it goes behind
    // the last filter or upscale and in front of bloom() and display(). params: null for the defaults.
    // coc_out, when given, receives each pixel's radius in pixels. It needs no scene state and does not render.
    Image dof(const Image& linear, const std::vector<float>& normal_depth, const rt_dof_params* params = nullptr,
              std::vector<float>* coc_out = nullptr) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const int w = linear.width(), h = linear.height();
        if (normal_depth.size() != (size_t)w * h * 4) throw std::runtime_error("librt_hip: dof: normal_depth is not width * height * 4 floats");
        if (coc_out) coc_out->assign((size_t)w * h, 0.0f);
        Image out(w, h);
        check(rt_dof(m_ctx, w, h, linear.data(), normal_depth.data(), params, out.data(), coc_out ? coc_out->data() : nullptr));
        return out;
    }

    // Motion vectors (rt_motion_vectors): for every pixel, where its first hit stood in the frame of prev_camera minus
    // where it stands now, in pixels (2 floats per pixel). normal_depth: features() or gbuffer() under the kernel's
    // current camera at width x height.
    std::vector<float> motion_vectors(const std::vector<float>& normal_depth, int width, int height, Camera prev_camera) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        if (normal_depth.size() != (size_t)width * height * 4)
            throw std::runtime_error("librt_hip: motion_vectors: normal_depth is not width * height * 4 floats");
        std::vector<float> motion((size_t)width * height * 2);
        check(rt_motion_vectors(m_ctx, width, height, normal_depth.data(), &prev_camera.view_matrix.m[0][0], prev_camera.fov_dist,
                                motion.data()));
        return motion;
    }

    // Motion blur (rt_motion_blur): a shutter's blur built from `linear`, the first-hit distances of normal_depth and
    // `motion` (motion_vectors(), or the caller's own: 2 floats per pixel); it goes behind dof() and in front of bloom()
    // and display(). params: null for the defaults. reach_out, when given, receives each pixel's half streak in pixels.
    Image motion_blur(const Image& linear, const std::vector<float>& normal_depth, const std::vector<float>& motion,
                      const rt_motion_params* params = nullptr, std::vector<float>* reach_out = nullptr) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const int w = linear.width(), h = linear.height();
        if (normal_depth.size() != (size_t)w * h * 4) throw std::runtime_error("librt_hip: motion_blur: normal_depth is not width * height * 4 floats");
        if (motion.size() != (size_t)w * h * 2) throw std::runtime_error("librt_hip: motion_blur: motion is not width * height * 2 floats");
        if (reach_out) reach_out->assign((size_t)w * h, 0.0f);
        Image out(w, h);
        check(rt_motion_blur(m_ctx, w, h, linear.data(), normal_depth.data(), motion.data(), params, out.data(),
                             reach_out ? reach_out->data() : nullptr));
        return out;
    }

    // INTERSECT_SCENE for a batch of rays through rt_query (the render's search-BVH walks, the
    // exact walk behind them): hits[i] as BVH::intersect + the sphere loop fill it (t = -1 and
    // primitive_index = -1 without a hit).
    void query_closest(const std::vector<Ray>& rays, std::vector<HitInfo>& hits) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const std::vector<float> r = ray_floats(rays);
        std::vector<int> rec(rays.size() * 11);
        check(rt_query(m_ctx, RT_QUERY_CLOSEST, r.data(), (long)rays.size(), rec.data()));
        hits.assign(rays.size(), HitInfo());
        for (size_t i = 0; i < rays.size(); i++) {
            const int* w = &rec[11 * i];
            if (!w[0]) continue;
            float f[7];
            std::memcpy(f, w + 2, sizeof f);
            hits[i].t = f[0];
            hits[i].inter_point = Point(f[1], f[2], f[3]);
            hits[i].normal_at_intersection = Vector(f[4], f[5], f[6]);
            hits[i].primitive_index = w[1];
        }
    }

    // The same as an occlusion test: hit[i] = 1 where INTERSECT_SCENE finds a hit.
    void query_any(const std::vector<Ray>& rays, std::vector<char>& hit) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const std::vector<float> r = ray_floats(rays);
        std::vector<int> found(rays.size());
        check(rt_query(m_ctx, RT_QUERY_ANY, r.data(), (long)rays.size(), found.data()));
        hit.assign(found.begin(), found.end());
    }

    // The first-hit guides of the camera's frame from the render's own walks (rt_render_gbuffer): albedo =
    // {diffuse rgb, 0} and normal_depth = {n.xyz, t} (a miss: zeros and t = -1), each resized to the kernel's
    // width x height; ids, when given, 2 ints per pixel = {primitive, material index}, {-1, -1} for a miss.
    // exact: every pixel takes the exact walk (RT_GBUFFER_EXACT), rt_render_features' bits with no exception.
    void gbuffer(Image& albedo, Image& normal_depth, std::vector<int>* ids = nullptr, bool exact = false) const
    {
        std::lock_guard<std::mutex> lk(m_mu);
        const_cast<RenderKernel*>(this)->sync_materials();
        albedo = Image(m_width, m_height);
        normal_depth = Image(m_width, m_height);
        if (ids) ids->assign((size_t)m_width * m_height * 2, 0);
        check(rt_render_gbuffer(m_ctx, m_width, m_height, exact ? RT_GBUFFER_EXACT : 0, albedo.data(), normal_depth.data(),
                                ids ? ids->data() : nullptr));
    }

    int device_count() const { return rt_device_count(m_ctx); }

private:
    static void check(int rc)
    {
        if (rc != RT_OK) throw std::runtime_error(std::string("librt_hip: ") + rt_last_error(nullptr));
    }

    static std::vector<float> ray_floats(const std::vector<Ray>& rays)  // rays[n][6] = origin, direction
    {
        std::vector<float> r;
        r.reserve(rays.size() * 6);
        for (const Ray& q : rays)
            r.insert(r.end(), {q.origin.x, q.origin.y, q.origin.z, q.direction.x, q.direction.y, q.direction.z});
        return r;
    }

    std::vector<char> materials_bytes() const
    {
        const char* p = reinterpret_cast<const char*>(m_materials_buffer.data());
        return std::vector<char>(p, p + m_materials_buffer.size() * sizeof(SimpleMaterial));
    }

    void sync_materials()
    {
        std::vector<char> now = materials_bytes();
        if (now == m_materials_sent) return;
        check(rt_set_materials(m_ctx, reinterpret_cast<const float*>(m_materials_buffer.data()),
                               (int)m_materials_buffer.size()));
        m_materials_sent.swap(now);
    }

    // {int is_leaf, int n, int tris[n], float min[3], max[3], d_near[7], d_far[7]}, children after
    // each internal node (the rt_set_bvh_preorder format)
    static void preorder(const BVH::OctreeNode* n, std::vector<char>& out)
    {
        auto put = [&](const void* p, size_t b) { out.insert(out.end(), (const char*)p, (const char*)p + b); };
        const int leaf = n->_is_leaf ? 1 : 0, cnt = (int)n->_triangles.size();
        put(&leaf, 4);
        put(&cnt, 4);
        put(n->_triangles.data(), 4 * (size_t)cnt);
        put(&n->_min.x, 12);
        put(&n->_max.x, 12);
        put(n->_bounding_volume._d_near.data(), 28);
        put(n->_bounding_volume._d_far.data(), 28);
        if (!n->_is_leaf)
            for (int i = 0; i < 8; i++) preorder(n->_children[i], out);
    }

    rt_context* m_ctx = nullptr;
    int m_width, m_height, m_render_samples, m_max_bounces;
    Image& m_frame_buffer;
    const std::vector<SimpleMaterial>& m_materials_buffer;
    std::vector<char> m_materials_sent;
    bool m_track = false;     // render_progressive_tracked: the progression render_progressive begins is tracked
    mutable std::mutex m_mu;  // one call on the context at a time (ray_trace_pixel is const and may be threaded)
};

#endif  // RENDER_KERNEL_HIP_H
