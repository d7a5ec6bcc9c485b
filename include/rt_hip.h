/* rt_hip.h — C ABI of librt_hip.so, the MI355X (gfx950) drop-in for the
 * reference's render kernel.
 *
 * Reference interface replaced (TomClabault/SYCL-ray-tracing @ 2024-08-07):
 *   class RenderKernel            include/render_kernel.h:21-96
 *     RenderKernel(...)           include/render_kernel.h:24-46   -> rt_create + rt_set_scene
 *                                                                   + rt_build_bvh / rt_set_bvh_preorder
 *                                                                   + rt_set_env
 *     set_camera(Camera)          include/render_kernel.h:48      -> rt_set_camera
 *     render()                    include/render_kernel.h:57,
 *                                 source/render_kernel.cpp:189-211 -> rt_render / rt_render_device
 *     ray_trace_pixel(x, y)       include/render_kernel.h:56,
 *                                 source/render_kernel.cpp:75-181  -> rt_render_pixels
 *   BVH(triangles, 32, 8)         source/bvh.cpp:19-37            -> rt_build_bvh
 *   BVH::intersect(ray, hit)      source/bvh.cpp:62-65            -> rt_intersect
 *   Camera presets                source/camera.cpp:3-8           -> rt_camera_preset
 *   Utils::parse_obj              source/utils.cpp:16-98          -> rt_mesh_load (+ rt_mesh_*)
 *   Utils::compute_env_map_cdf    source/utils.cpp:126-142        -> rt_env_luminance_cdf
 *
 * Conventions: every function returns 0 (RT_OK) or a negative RT_ERR_*;
 * rt_last_error() gives the message. Inputs are copied (the caller keeps
 * ownership, like the reference's const std::vector& members). Calls are
 * synchronous unless a stream is passed. One context per host thread.
 * Buffer layouts are the reference's in-memory layouts:
 *   triangles  float[n][9]  Triangle{Point m_a, m_b, m_c}       (triangle.h:67)
 *   materials  float[m][10] SimpleMaterial{Color emission (rgba), Color diffuse (rgba),
 *                           metalness, roughness}                (simple_material.h:6-13)
 *   spheres    float[s][5]  Sphere{center xyz, radius, primitive_index (as float)} (sphere.h:7-59)
 *   image      float[h][w][4] Image / Color RGBA                 (image.h:25-178)
 *   view       float[16]    Transform::m row-major, + Camera::fov_dist (camera.h:38-40)
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_ERR_ARG (-1)
#define RT_ERR_HIP (-2)
#define RT_ERR_STATE (-3)
#define RT_ERR_IO (-4)
#define RT_ERR_NODEV (-5)

typedef struct rt_context rt_context;
typedef struct rt_mesh rt_mesh;
/* Parameters of rt_denoise (rt_denoise_default_params fills the defaults). */
typedef struct rt_denoise_params {
    int passes;          /* a-trous iterations, 1..10; pass i has step 1 << i */
    float sigma_color;   /* colour edge-stopping width; pass i uses sigma_color * 2^-i */
    float sigma_normal;  /* the same for the first-hit normals, */
    float sigma_albedo;  /* ... albedo */
    float sigma_depth;   /* ... and relative depth (t_p - t_q) / max(t_p, t_q) */
} rt_denoise_params;
/* Parameters of rt_display (rt_display_default_params fills the defaults). */
typedef struct rt_display_params {
    float exposure;      /* finite; the reference's 1.5f (render_kernel.cpp:175) */
    float gamma;         /* finite and > 0; the reference's 2.2f (render_kernel.cpp:178) */
    int flip_y;          /* rows of the 8-bit output reversed, as write_image_png writes them */
} rt_display_params;
/* What rt_progress_noise reports about the frame. */
typedef struct rt_noise_stats {
    float max_tile;      /* the largest tile error */
    int tiles;           /* 8x8 tiles of the row shard */
    int tiles_over;      /* tiles whose error is > threshold */
    int nonfinite;       /* in-frame pixels whose error is not finite (they count 0 in their tile) */
    int samples_a;       /* samples in the A passes (the even-numbered ones) */
    int samples_b;       /* ... and in the B passes */
    int passes;          /* passes so far */
} rt_noise_stats;

/* ---------------------------------------------------------------- context */
int rt_create(int device, rt_context** out);
/* One context over n_devices GPUs of this process (devices[] = HIP ordinals,
 * NULL = 0..n-1; devices[0] is the root). Scene, BVH and env are replicated on
 * every device; a render shards the frame's rows (row j of the request ->
 * device j mod n), ncclScatter's the root framebuffer's rows to their devices,
 * renders every shard on its own device and ncclGather's them back to the root
 * (single-process RCCL clique, ncclCommInitAll). The result is bit-identical to
 * a single-device render. Replaces the OpenMP row loop of RenderKernel::render
 * (render_kernel.cpp:189-211) for a whole node. RT_ERR_NODEV if a device or
 * librccl.so.1 is missing. */
int rt_create_multi(int n_devices, const int* devices, rt_context** out);
int rt_device_count(const rt_context* ctx);
/* TEST ONLY (no reference counterpart). rt_create_multi_loopback: as
 * rt_create_multi, but devices[] may name one GPU more than once and the
 * shards are exchanged by device copies instead of RCCL, so the whole
 * multi-device driver (threads, streams, pack / un-permute) runs on a
 * one-GPU box. rt_test_fail_device: every later multi-device render of ctx
 * fails device d (0..n-1) before its work starts (-1: off), to exercise the
 * per-device error slots. Never called by the product paths. */
int rt_create_multi_loopback(int n_devices, const int* devices, rt_context** out);
/* TEST ONLY. rt_test_create_multi_rccl: as rt_create_multi, but the multi-device
 * driver runs even for one listed device, through a one-rank RCCL clique
 * (ncclCommInitAll over [device]): pack, ncclScatter, render, ncclGather and
 * un-permute, so that a one-GPU box executes the RCCL path the 8-GPU node runs. */
int rt_test_create_multi_rccl(int n_devices, const int* devices, rt_context** out);
int rt_test_fail_device(rt_context* ctx, int device);
/* TEST ONLY. rt_test_schedule: override one wavefront-schedule parameter of
 * ctx's later renders (keys: "lanes", "tail_paths" (0: no tail kernel),
 * "tail_enter", "tail_rows", "drain_rows", "heavy_calls", "spec_cam",
 * "tail_spec_cam", "step_budget", "fast_k" (fast lane: that many of the slowest
 * paths go to a tail kernel early; 0: off), "fast_spp" (... from iteration
 * fast_spp x spp on), "near_scale" (the near box, scene box widened by this x its
 * largest extent: queries from outside it take the exact octree walk), "dn_variant"
 * (rt_denoise's and rt_denoise_var's filter kernel: 0 the product's choice per step, 1 direct
 * loads, 2 the LDS-halo tile at every step that has one), "ff_variant" (rt_firefly's kernel: 0 the
 * product's choice, 1 direct loads, 2 the LDS tile of luminances), "mt_variant" (rt_meter's kernel: 0 the
 * product's choice, 1 global atomics per pixel, 2 per-wave bins in LDS), "mt_blocks" (rt_meter's grid: 0 the
 * product's cap, n > 0 that many blocks, at most 65536), "up_variant" (rt_upscale's kernel: 0 the product's
 * choice, 1 direct loads, 2 the low-resolution footprint staged in LDS), "bloom_variant" (rt_bloom's reduce kernel:
 * 0 the product's choice, 1 direct loads, 2 the source footprint staged in LDS), "dof_variant" (rt_dof's kernel: 0 the
 * product's choice, 1 direct loads, 2 the footprint staged in LDS), "motion_variant" (rt_motion_blur's gather kernel, the
 * same three: in every two-kernel stage 1 is direct loads and 2 the LDS kernel), "rq_variant" (rt_query's search-BVH kernel:
 * 0 the product's choice, 1 plain rounds of one query per quad, 2 per-quad refill), "gb_variant" (the same three
 * for rt_render_gbuffer's search-BVH kernel), the stressor "gb_force_every" (N > 0: G-buffer pixels with
 * i mod N == 0 go to the exact walk's list instead of the search-BVH walk; 0: off),
 * "chain_full" (1: the scene view reports an unmonotone tree, so the leaf verification
 * walks the whole ancestor chain instead of one slab test), the
 * stressor "force_fallback" (every k-th query by a ray hash skips to the exact
 * octree walk), "reset"). No parameter changes a result; the product never calls
 * it and reads no schedule from the environment. RT_ERR_ARG for an unknown key or
 * a value that is not a finite number in int range. */
int rt_test_schedule(rt_context* ctx, const char* key, double value);
/* TEST ONLY. Walk log of stats renders (rt_set_stats): every search-BVH walk of
 * at least min_calls quad_visit calls (a row trip counts 2) is recorded, up to
 * capacity records (min_calls 0: off); sample_every > 1 keeps only the walks
 * whose (path slot, iteration, kind) hash is 0 modulo it, sample_every < 0 only
 * the k_trace walks left to the exact octree walk (their triangle field then
 * says why: 1 a tie, 2 the octree chain check, 3 the bounded stack). A record is RT_WLOG_FLOATS floats:
 * origin xyz, kind | where << 8 (int bits; where 0 k_trace quads, 1 a k_trace
 * drain's rows, 2 k_tail), direction xyz, calls (int bits), t (closest: the
 * answer, -1 none, -2 left to the exact walk; occlusion: 1 occluded / 0 not),
 * triangle (int bits), iteration (int bits), path slot (int bits).
 * rt_test_walk_log_read copies up to capacity records of the last stats render
 * and returns how many walks qualified (>= the records copied). */
#define RT_WLOG_FLOATS 12
int rt_test_walk_log(rt_context* ctx, int min_calls, int sample_every, int capacity);
long rt_test_walk_log_read(const rt_context* ctx, float* out, long capacity);
/* TEST ONLY. rt_device_env_search: the env-map CDF search (sample_environment_map's two
 * searches, render_kernel.cpp:532-567) alone, for n caller values over ctx's env:
 * xy_out[2 i] = x, xy_out[2 i + 1] = y. form 0: what the shading kernels run (on the GPU
 * with their LDS staging of the row tables), form 1: the same tables read from global
 * memory whatever the env's height. The hostsim build runs its one host form for both.
 * Never called by the product paths. */
int rt_device_env_search(rt_context* ctx, int form, const float* values, int n, int* xy_out);
void rt_destroy(rt_context* ctx);
const char* rt_last_error(const rt_context* ctx); /* ctx may be NULL: last global error */
int rt_version(void);
/* The build of this library: "src=<hash of its kernel sources> defs=<experiment
 * flags>" (Makefile), so a measurement reports the binary it ran. */
const char* rt_build_id(void);

/* Scene buffers bound by the RenderKernel constructor (render_kernel.h:27-31). */
int rt_set_scene(rt_context* ctx, const float* triangles, int n_triangles, const int* material_indices,
                 int n_material_indices, const float* materials, int n_materials, const int* emissive_triangles,
                 int n_emissive, const float* spheres, int n_spheres);

/* The material buffer alone, for a context whose scene is set: the reference
 * keeps `const std::vector<SimpleMaterial>&` (render_kernel.h:81-93), so a
 * caller may edit materials between render() calls (the cfg5 material sweep);
 * this pushes the new table without rebuilding the octree / search BVH.
 * Material indices must stay in range. */
int rt_set_materials(rt_context* ctx, const float* materials, int n_materials);

/* BVH(&triangles, max_depth, leaf_max_obj_count): native octree build,
 * bit-identical to bvh.h:55-125 (child-box quirk included). */
int rt_build_bvh(rt_context* ctx, int max_depth, int leaf_max_obj_count);
/* Drop-in for a reference-built BVH&: a pre-order walk of BVH::_root, per node
 * {int is_leaf, int n, int tris[n], float min[3], max[3], d_near[7], d_far[7]},
 * children 0..7 after each internal node (INTEGRATION.md shows the walker). */
int rt_set_bvh_preorder(rt_context* ctx, const void* dump, long bytes);
/* Pre-order dump of the context's octree in the same format; returns the size. */
long rt_bvh_dump(const rt_context* ctx, void* buf, long capacity);
/* info[0..4] = octree nodes, GPU child records, triangles, max depth, GPU bytes */
int rt_bvh_info(const rt_context* ctx, long* info);

/* skysphere Image + env_map_cdf (render_kernel.h:33-34). `pixels` has
 * `channels` (3 or 4) floats per texel, row 0 first (as read_image_float
 * leaves it). cdf may be NULL: computed exactly like compute_env_map_cdf. */
int rt_set_env(rt_context* ctx, const float* pixels, int width, int height, int channels, const float* cdf);

/* RenderKernel::set_camera. */
int rt_set_camera(rt_context* ctx, const float view[16], float fov_dist);

/* RenderKernel::render(): fb_rgba (host, w*h*4) is read (accumulated into)
 * and overwritten with the tone-mapped result, exactly as the reference
 * mutates its Image&. */
int rt_render(rt_context* ctx, int width, int height, int samples, int max_bounces, float* fb_rgba);

/* Device-resident render for benchmarking / multi-GPU sharding: renders image
 * rows y = row_offset + j*row_stride (j = 0..) into d_fb (device, rows_local*w*4
 * floats, row j of the shard at offset j*w*4). stream may be NULL (default).
 * Multi-device context: d_fb and stream live on the root device. */
int rt_render_device(rt_context* ctx, int width, int height, int samples, int max_bounces, void* d_fb,
                     int row_offset, int row_stride, void* stream);

/* The Cook-Torrance material sweep (BASELINE config 5) as replicas: n_variants
 * material tables materials[n_variants][n_materials][10] over the bound scene
 * (rt_set_materials semantics for each: no octree / BVH rebuild). Variant v
 * renders rows y = row_offset + j*row_stride of its own frame on device
 * v mod N of the context, each device walking its variants in order on its own
 * stream; the devices run concurrently and exchange nothing. Output: either
 * fb_rgba (host, n_variants blocks of rows_local*w*4 floats, read and overwritten
 * like rt_render's) or d_fbs[v] (device buffers of rows_local*w*4 floats, d_fbs[v]
 * on device v mod N). Synchronous; rt_last_kernel_ms is the slowest device's time.
 * The context's own material table (rt_set_scene / rt_set_materials) is what the
 * next render uses again. Replaces the caller loop of render_kernel.h:81-93
 * (edit the bound std::vector<SimpleMaterial>, render(), repeat). */
int rt_render_variants(rt_context* ctx, int width, int height, int samples, int max_bounces, int n_variants,
                       const float* materials, int n_materials, int row_offset, int row_stride, float* fb_rgba,
                       void* const* d_fbs);

/* ray_trace_pixel for a list of n pixels xy[n][2]: rgba[n][4] holds each
 * pixel's framebuffer value on entry and the tone-mapped value on return. */
int rt_render_pixels(rt_context* ctx, int width, int height, int samples, int max_bounces, const int* xy, int n,
                     float* rgba);

/* BVH::intersect + sphere loop (INTERSECT_SCENE) for n rays rays[n][6]
 * (origin, direction); out[n][11] = {found, primitive, t, point[3],
 * normal[3], u, v} with u = v = -1 (unused downstream). */
int rt_intersect(rt_context* ctx, const float* rays, int n, void* out);

/* ------------------------------------------------------------ ray queries
 * INTERSECT_SCENE for a batch of n rays rays[n][6] (origin, direction) through the walks
 * the render uses: visibility, ambient-occlusion, depth or picking rays from the caller's
 * own buffers. Answers are rt_intersect's, bit for bit; the rays keep the caller's order.
 *
 * Routing (the render's policy): a query whose origin lies inside the near box (the
 * scene's box widened on every side by half its largest extent) takes the search-BVH
 * walk, four lanes per query; a walk that does not settle (a tie between octree leaves,
 * a failed octree chain check, an overflow of the bounded stack) hands its query to the
 * exact octree walk, as do all queries from outside the near box. A context with
 * spheres, or in rt_set_intersect_mode(0), sends every query to the exact walk, and so
 * does the flag RT_QUERY_EXACT. The shell limit of DESIGN.md §4 applies as it does to
 * the render: from origins inside the near box but far outside the scene's box, the
 * search-BVH walk can miss a grazing hit that the exact walk finds. A caller that needs
 * the exact walk's answer for every origin passes RT_QUERY_EXACT.
 *
 * There is no t_max: the reference's shadow test is the closest hit followed by
 * `t + 1e-4 < t_max` (render_kernel.cpp:744-759), and the render's occlusion walk has
 * no distance either. A distance-limited test is RT_QUERY_CLOSEST plus that comparison
 * on word 2 of the record.
 *
 * rt_query: host buffers; uploads, runs, waits, downloads; rt_last_kernel_ms is the
 * kernels' time. rt_query_device: device buffers on `stream` (NULL: default), returns
 * without waiting; rt_last_kernel_ms is -1 and rt_device_last_kernel_ms reads the
 * events once the stream is synchronized. The workspace (the fallback list) belongs to
 * the context and grows when n does; calls on one context must not overlap in time on
 * different streams. A multi-device context runs queries on its root device (where
 * d_rays, d_out and stream live) and restores the caller's current device.
 * rt_query_last_exact: how many queries of the last call took the exact walk; waits for
 * that call. RT_ERR_STATE without scene and BVH; RT_ERR_ARG for an unknown mode, n < 0,
 * n >= 2^27 or a NULL buffer with n > 0; n == 0 is RT_OK and launches nothing. NaN and
 * zero-direction rays answer as rt_intersect answers them (no hit). */
#define RT_QUERY_CLOSEST 0   /* out[n][11], rt_intersect's record, bit for bit */
#define RT_QUERY_ANY     1   /* out[n] int32: 1 if INTERSECT_SCENE finds a hit, else 0
                                (the `found` word of rt_intersect) */
#define RT_QUERY_EXACT   0x100 /* flag: every query takes the exact walk */
int rt_query(rt_context* ctx, int mode, const float* rays /*[n][6]*/, long n, void* out);
int rt_query_device(rt_context* ctx, int mode, const void* d_rays, long n, void* d_out, void* stream);
long rt_query_last_exact(rt_context* ctx); /* queries of the last call that took the exact walk; waits */

/* USE_BVH (render_kernel.h:13, render_kernel.cpp:504-511): 1 (the reference's
 * build, the default) answers INTERSECT_SCENE with the octree walk
 * (intersect_scene_bvh :485-502); 0 with the brute-force triangle loop
 * (intersect_scene :453-483: closest by strict `<` in buffer order, so the
 * lowest triangle index wins a tie). */
int rt_set_intersect_mode(rt_context* ctx, int use_bvh);

/* ------------------------------------------------------------ post stage
 * What replaces Utils::OIDN_denoise (utils.cpp:144-196; main.cpp:116-124 calls it at
 * blend 1.0 / 0.75 / 0.5): first-hit feature buffers and an edge-avoiding a-trous
 * filter (Dammertz et al. 2010) guided by them. A different algorithm from OIDN's
 * network, so there is no parity with the reference's denoised images; the blend and
 * alpha arithmetic are the reference's (utils.cpp:184-186).
 *
 * rt_render_features: for every pixel (x, y) of a w x h frame the camera ray through the
 * centre of the pixel's jitter window (x_j = (float)x, y_j = (float)y in
 * get_camera_ray, render_kernel.cpp:56-73, :88-89) and its first hit, bitwise what
 * rt_intersect answers for that ray (rt_set_intersect_mode honoured). Two float[h][w][4]
 * buffers: normal_depth = {n.xyz, t} (miss: {0, 0, 0, -1}) and albedo = {diffuse rgb of
 * materials[material_indices[prim]], 0} (miss: zeros). RT_ERR_STATE without scene, BVH or
 * camera. rt_camera_rays (host only) writes those rays, rays[h*w][6] = origin, direction.
 *
 * rt_denoise: `passes` a-trous iterations over rgba_in (float[h][w][4]), ping-pong; pass i
 * has step s = 1 << i and, for pixel p, visits the taps q = p + s (dx, dy), (dy, dx) in
 * {-2..2}^2 in that order (dy outer), skipping taps outside the image:
 *   k = h[dy+2] h[dx+2], h = {1/16, 1/4, 3/8, 1/4, 1/16}
 *   e = |c_p - c_q|^2 / (sigma_color 2^-i)^2 + |n_p - n_q|^2 / sigma_normal^2
 *     + |a_p - a_q|^2 / sigma_albedo^2 + ((t_p - t_q) / max(t_p, t_q))^2 / sigma_depth^2
 *   out_p = sum k expf(-e) c_q / sum k expf(-e)
 * The depth term is 0 between two misses (t <= 0) and a tap is skipped between a hit and
 * a miss; a tap whose colour is not finite is skipped and a centre that is not finite
 * passes through. albedo and normal_depth both NULL: the guide terms drop out (the
 * colour-only call the reference makes). Then rgb = blend * filtered + (1.0f - blend) *
 * input, alpha 1.0f. Alpha plays no part in the filter. RT_ERR_ARG for passes outside
 * 1..10, a sigma that is not finite and > 0, a non-finite blend, exactly one guide NULL,
 * rgba_in == rgba_out, or a frame of more than 262140 rows or 2^27 - 1 pixels. params
 * NULL: the defaults. Guides that hold a NaN give the taps they touch no weight; a pixel
 * whose own guide is NaN passes through.
 *
 * The *_device forms take device pointers and a stream (NULL: default) and return
 * without waiting. A multi-device context runs the post stage on its root device; the
 * caller's current device is restored. rt_last_kernel_ms reports the stage's time (the
 * device forms: -1, read rt_device_last_kernel_ms after synchronizing). */
int rt_camera_rays(rt_context* ctx, int w, int h, float* rays); /* host only */
int rt_render_features(rt_context* ctx, int w, int h, float* albedo, float* normal_depth);
int rt_render_features_device(rt_context* ctx, int w, int h, void* d_albedo, void* d_normal_depth, void* stream);
void rt_denoise_default_params(rt_denoise_params* params);
int rt_denoise(rt_context* ctx, int w, int h, const float* rgba_in, const float* albedo, const float* normal_depth,
               const rt_denoise_params* params, float blend, float* rgba_out);
int rt_denoise_device(rt_context* ctx, int w, int h, const void* d_rgba_in, const void* d_albedo,
                      const void* d_normal_depth, const rt_denoise_params* params, float blend, void* d_rgba_out,
                      void* stream);

/* ------------------------------------------- first-hit G-buffer on the walks
 * rt_render_features' two buffers, and the optional primitive and material ids, from the
 * walks the render uses instead of one exact octree walk per lane: the guide pass for
 * scenes where that walk's chain of dependent loads sets the pass's time.
 *
 * albedo and normal_depth are rt_render_features' records for the same ray (the centre of
 * the pixel's jitter window); ids, when given, is int32[h][w][2] = {primitive,
 * material_indices[primitive]}, {-1, -1} for a miss. The output is what
 * rt_query(RT_QUERY_CLOSEST) answers for rt_camera_rays(w, h), bit for bit, turned into
 * records by rt_render_features' rule: a hit where word 0 says so, t word 2, the normal
 * words 6..8, the primitive word 1.
 *
 * Routing is rt_query's: a pixel whose origin lies inside the near box takes the
 * search-BVH walk, four lanes per pixel; a walk that does not settle hands its pixel to
 * the exact octree walk, eight lanes per walk, as do all pixels of a camera outside the
 * near box. A context with spheres, or in rt_set_intersect_mode(0), has no octree answer
 * to share: every pixel takes rt_render_features' own one-lane walk there. The flag
 * RT_GBUFFER_EXACT sends every pixel to the exact walk, and the output then equals
 * rt_render_features bit for bit, with no exception. Without the flag the shell limit of
 * DESIGN.md §4 applies as it does to the render and to rt_query: from a camera inside the
 * near box but far outside the scene's box, the search-BVH walk can miss a grazing hit that
 * the exact walk finds. A guide taken from the walks is the first hit the render saw.
 *
 * rt_render_gbuffer: host buffers; runs, waits, downloads; rt_last_kernel_ms is the
 * kernels' time. rt_render_gbuffer_device: device buffers on `stream` (NULL: default),
 * returns without waiting; rt_last_kernel_ms is -1 and rt_device_last_kernel_ms reads the
 * events once the stream is synchronized. The workspace (the fallback list, the octets'
 * spill areas) belongs to the context and grows with the frame; calls on one context must
 * not overlap in time on different streams. A multi-device context runs the stage on its
 * root device and restores the caller's current device. rt_gbuffer_last_exact: how many
 * pixels of the last call took the exact walk; waits for that call.
 * RT_ERR_STATE without scene, BVH or camera; RT_ERR_ARG for w or h <= 0, more than
 * 2^27 - 1 pixels, unknown flag bits, a NULL albedo or normal_depth, any two buffers that
 * overlap by range, or (device form) a float4 buffer not 16-byte aligned or ids not 8-byte
 * aligned. */
#define RT_GBUFFER_EXACT 0x100 /* flag: every pixel takes the exact walk */
int rt_render_gbuffer(rt_context* ctx, int w, int h, int flags, float* albedo, float* normal_depth,
                      int* ids /*optional*/);
int rt_render_gbuffer_device(rt_context* ctx, int w, int h, int flags, void* d_albedo, void* d_normal_depth, void* d_ids,
                             void* stream);
long rt_gbuffer_last_exact(rt_context* ctx); /* pixels of the last call that took the exact walk; waits */

/* ---------------------------------------------------- progressive rendering
 * A frame of samples_total samples rendered in passes: previews after the first few
 * samples, slices that fit a time budget, checkpoints that another process resumes.
 *
 * The reference seeds a pixel's chain with 31 + x*y*samples (render_kernel.cpp:77), so
 * samples 0..s-1 of an N-sample frame are not the s-sample frame: the total is declared at
 * rt_progress_begin and fixed. Between passes the context keeps, per pixel of the row shard
 * (rows y = row_offset + j*row_stride, as rt_render_device), the base value the frame adds
 * to and one float4 of state {final_color rgb, RNG bits}, in buffers of its own: other
 * renders, queries and post-stage calls on the context between passes leave them alone.
 * Every pixel pauses at its pass's last sample, so `done` is one number.
 *
 * rt_progress_begin: fb_rgba_base is host memory, rows_local*w*4 floats, row j of the
 *   shard at offset j*w*4 (NULL: (0, 0, 0, 1) per pixel). Replaces a running progression.
 * rt_progress_advance: the next min(samples, remaining) samples of every pixel on `stream`
 *   (NULL: default), returning without waiting for the device. Nothing left: RT_OK, no launch.
 * rt_progress_resolve / _device: writes tonemap(base + final_color / (float)done) for every
 *   pixel of the shard (rows_local*w*4 floats; host: waits; device: on `stream`), with the
 *   render's own division and tone-map operations, so after passes that sum to the total the
 *   words are rt_render's / rt_render_device's into a framebuffer holding the base, however
 *   the total was split. It changes no state. Before that point it is a preview: the mean of
 *   the first `done` samples of the N-sample chain, which is not the reference's
 *   `done`-sample frame (except where x*y == 0: there the seed is 31 for every count).
 *   done == 0: RT_ERR_STATE. rt_last_kernel_ms reports the resolve's time (the device form: -1,
 *   read rt_device_last_kernel_ms after synchronizing), as for every stage with both forms.
 * rt_progress_info: info = {w, h, total, done, bounces, row_offset, row_stride, rows_local}.
 * rt_progress_save: header (magic, format version, the eight info words; 10 int32), then
 *   the base, then the state; returns the size (buf NULL or capacity too small: only the
 *   size). Waits for the passes. rt_progress_load installs a saved progression at its `done`
 *   (scene, BVH, env and camera bound, as for begin). RT_ERR_ARG for a bad magic or version,
 *   a size that does not match the header, or done > total. The header does not fingerprint
 *   the scene: the caller must bind the scene, env, camera and intersect mode it saved under.
 * rt_progress_end: drops the progression and its buffers; harmless without one.
 *
 * rt_set_scene, rt_build_bvh, rt_set_bvh_preorder, rt_set_env, rt_set_camera,
 * rt_set_materials and rt_set_intersect_mode end a progression. RT_ERR_STATE: no scene,
 * BVH, env or camera bound; no progression. RT_ERR_ARG: non-positive sizes, total or
 * `samples`, negative bounces, a row shard outside the frame, a NULL output, a multi-device
 * context (not supported: run one process per GPU with its own row shard). */
int rt_progress_begin(rt_context* ctx, int width, int height, int samples_total, int max_bounces,
                      const float* fb_rgba_base, int row_offset, int row_stride);
int rt_progress_advance(rt_context* ctx, int samples, void* stream);
int rt_progress_resolve(rt_context* ctx, float* fb_rgba);
int rt_progress_resolve_device(rt_context* ctx, void* d_fb, void* stream);
int rt_progress_info(const rt_context* ctx, int info[8]);
long rt_progress_save(rt_context* ctx, void* buf, long capacity);
int rt_progress_load(rt_context* ctx, const void* buf, long bytes);
void rt_progress_end(rt_context* ctx);

/* ------------------------------------------- linear radiance and the display stage
 * The reference ends a pixel with hdrColor = entry + final_color / samples and then its
 * exposure / gamma tone-map with the literals 1.5 and 2.2 (render_kernel.cpp:171-180).
 * rt_render returns the tone-mapped frame; these calls return the linear one and apply the
 * tone-map, with a caller's exposure and gamma, as a stage of its own.
 *
 * rt_render_linear / _device: rt_render / rt_render_device without the tone-map pass. On
 *   return the buffer holds, per pixel, entry.rgb + final_color / (float)samples and the entry
 *   alpha untouched. Same argument checks, row shards, multi-device support and
 *   rt_last_kernel_ms conventions as their tone-mapped twins.
 * rt_progress_resolve_linear / _device: base + state.rgb / (float)done, alpha = the base's:
 *   rt_progress_resolve's division and sum, stopped before its tone-map. Changes no state;
 *   RT_ERR_STATE without a progression or with done == 0.
 * rt_display / _device: for every pixel of a w x h linear frame
 *     rgb = powf(1 - expf(-x * exposure), 1 / gamma),  a = 1 - (-(a + 0)) * exposure
 *   in the reference's operation order, so rt_display(rt_render_linear(fb)) at the defaults is
 *   rt_render(fb), bit for bit. rgba_out (w*h*4 floats, frame order) may be the input (in
 *   place). rgba8_out (w*h*4 bytes) is rt_image_to_rgba8 of that result, rows reversed when
 *   params->flip_y; flip_y affects nothing else. Either output may be NULL, not both. params
 *   NULL: the defaults (1.5, 2.2, 0). No scene has to be bound. RT_ERR_ARG: non-positive
 *   sizes, an exposure that is not finite, a gamma that is not finite and > 0, both outputs
 *   NULL, more than 2^27 - 1 pixels, rgba8_out overlapping the input or rgba_out, rgba_out
 *   overlapping the input without being it. The device form takes device pointers and a
 *   stream (NULL: default) and returns without waiting; d_linear and d_rgba_out must be 16-byte
 *   aligned and d_rgba8_out 4-byte aligned (the kernel moves a pixel with one 16-byte access
 *   and its four bytes with one 4-byte store; any hipMalloc pointer and any whole-pixel offset
 *   into one is; RT_ERR_ARG otherwise), while the host form takes any alignment. A multi-device
 *   context runs the stage on its root device and restores the caller's current device.
 *   rt_last_kernel_ms reports the stage's time (the device form: -1, read
 *   rt_device_last_kernel_ms after synchronizing).
 * rt_write_hdr (host only): write_image_hdr (image_io.cpp:208-214): a Radiance RGBE file of
 *   the rgb channels (alpha dropped), rows reversed when flip_y, that rt_read_hdr decodes.
 *   Per pixel the exponent is frexp's of the largest channel and the mantissas are truncated
 *   (each channel comes back within 2^(e - 8)); a largest channel below 1e-32 is four zero
 *   bytes; negative and NaN channels are written as 0 and anything above the format's largest
 *   value, 255 * 2^119, as that value. Flat (not run-length encoded) scanlines. RT_ERR_ARG for
 *   a NULL path or image or a non-positive size, RT_ERR_IO if the path cannot be written. */
void rt_display_default_params(rt_display_params* params);
int rt_render_linear(rt_context* ctx, int width, int height, int samples, int max_bounces, float* fb_rgba);
int rt_render_linear_device(rt_context* ctx, int width, int height, int samples, int max_bounces, void* d_fb,
                            int row_offset, int row_stride, void* stream);
int rt_progress_resolve_linear(rt_context* ctx, float* fb_rgba);
int rt_progress_resolve_linear_device(rt_context* ctx, void* d_fb, void* stream);
int rt_display(rt_context* ctx, int w, int h, const float* linear_rgba, const rt_display_params* params,
               float* rgba_out, unsigned char* rgba8_out);
int rt_display_device(rt_context* ctx, int w, int h, const void* d_linear, const rt_display_params* params,
                      void* d_rgba_out, void* d_rgba8_out, void* stream);
int rt_write_hdr(const char* path, const float* rgba, int width, int height, int flip_y);

/* ------------------------------------------- noise estimate of a progression
 * How noisy the preview is, so that a caller can stop at a threshold instead of guessing the
 * sample count. A tracked progression keeps one more float4 per pixel, `half`: the rgb sum of
 * the samples rendered by its A passes (fourth word 0). Passes are counted from 0 over the
 * rt_progress_advance calls that rendered a sample; the even ones are A passes, the odd ones B
 * passes, with nA and nB samples. Around an A pass, on the pass's stream:
 *     before   half.c = half.c - state.c        after   half.c = half.c + state.c
 * so half gains what the pass added to the state. With N = nA + nB, in float32, no contraction,
 * IEEE division and square root, per pixel:
 *     m.c = state.c / (float)N          a.c = half.c / (float)nA
 *     d   = (|m.r - a.r| + |m.g - a.g|) + |m.b - a.b|
 *     e   = (k * d) / sqrtf(0.01f + ((m.r + m.g) + m.b)),     k = sqrtf((float)nA / (float)nB)
 * The base plays no part. Tiles are 8x8 pixels of the shard's local rows (tile (tx, ty): columns
 * 8tx.., local rows 8ty..; th = ceil(rows_local / 8), tw = ceil(w / 8)); element l of a tile is
 * pixel (8tx + l % 8, 8ty + l / 8), 0 when outside the frame or when e is not finite; the 64
 * elements are summed pairwise (v = v[0::2] + v[1::2], six times) and divided by the tile's
 * in-frame pixel count.
 *
 * rt_progress_noise_track: turns tracking on for the running progression. RT_ERR_STATE without
 *   one or once a sample is done; a second call is harmless. Whatever ends a progression ends
 *   its tracking.
 * rt_progress_noise: stats (required), pixel_err (rows_local*w floats: e as computed, non-finite
 *   values included; or NULL) and tile_err (th*tw floats, or NULL). Waits. RT_ERR_STATE when the
 *   progression is not tracked or nA == 0 or nB == 0 (fewer than two passes); RT_ERR_ARG for a
 *   threshold that is not finite and >= 0 or a NULL stats.
 * rt_progress_noise_device: device buffers (4-byte aligned) on `stream`, no wait. d_stats is
 *   eight int32 words {tiles, tiles_over, nonfinite, bits of max_tile, nA, nB, passes, 0}.
 * Neither form changes any state. rt_last_kernel_ms reports the query's time (the device form:
 * -1, read rt_device_last_kernel_ms after synchronizing).
 *
 * Checkpoints: rt_progress_save of a tracked progression writes format version 2: the 10-word
 * header with version 2, {passes, nA} as two int32 words, then base, state and half. An
 * untracked one writes version 1 as before. rt_progress_load takes both; a version-2 checkpoint
 * loads as a tracked progression and continues as the uninterrupted one would. RT_ERR_ARG for a
 * size that does not match, nA outside 0..done or passes < 0. */
int rt_progress_noise_track(rt_context* ctx);
int rt_progress_noise(rt_context* ctx, float threshold, rt_noise_stats* stats, float* pixel_err, float* tile_err);
int rt_progress_noise_device(rt_context* ctx, float threshold, void* d_stats, void* d_pixel_err, void* d_tile_err,
                             void* stream);

/* ------------------------------------------- adaptive sampling of a progression
 * A frame that spends its samples where the noise is: a pass advances only the 8x8 tiles (the
 * noise estimate's tiles, over the shard's local rows, t = ty*tw + tx) whose error is still above
 * a threshold. Every pixel stays a bit-exact prefix of the chain rt_render runs for it: a pixel
 * with c samples holds the state an untracked progression of the same total holds at done = c.
 *
 * An adaptive progression is a tracked progression plus two int32 per tile: tile_n[t], the
 * samples done by every pixel of the tile, and tile_nA[t], how many of them fell in A passes.
 *
 * rt_progress_advance_adaptive: on a tracked progression; the first call makes it adaptive with
 *   tile_n = done and tile_nA = nA in every tile. Tile t is active in the pass iff
 *       tile_n[t] + samples <= total    and    (passes < 2  or  tile_err[t] > threshold)
 *   where tile_err is the noise estimate's tile value computed with the tile's own counts
 *   (N = tile_n[t], nA = tile_nA[t], nB = N - nA; a NaN compares false). While passes < 2 there is
 *   no estimate and every tile that fits is active. A tile with tile_err > threshold that does not
 *   fit under the total is capped, not active: choose a total that is a multiple of the pass size.
 *   Active tiles get tile_n += samples and, on an A pass, tile_nA += samples; the half fold runs
 *   over their pixels only, and no word of an inactive pixel is touched. Pass parity stays global:
 *   the pass is an A pass iff `passes` is even; passes, nA and nB advance as for rt_progress_advance
 *   when a pass is launched (they are what a tile active in every pass has, and rt_noise_stats keeps
 *   reporting them). A tile that was active in A passes only has a lopsided split; k still
 *   normalises it, the estimate is valid but less sharp.
 *   The call waits for the work already queued on the progression, reads one small header back to
 *   size the launch, enqueues the pass on `stream` and returns without waiting for it.
 *   info = {active tiles, active pixels, capped tiles, min tile_n after, max tile_n after, tiles,
 *   0, 0}. No active tile: RT_OK, nothing launched, passes unchanged.
 *   The active pixels are listed by ascending tile, row-major inside a tile, so the pass is a pure
 *   function of the state: runs, checkpoints and the two builds agree.
 * On an adaptive progression:
 *   rt_progress_resolve*, _linear*: divide by the pixel's tile count, same operations.
 *   rt_progress_noise / _device: the tile's counts in k and both divisions; a tile with nA == 0 or
 *     nB == 0 gives non-finite elements, which count 0.
 *   rt_progress_info: done is the smallest tile_n.
 *   rt_progress_advance: RT_ERR_STATE once the tile counts differ; with equal counts it behaves as
 *     before and keeps the tile arrays in step.
 *   rt_progress_save writes format version 3: the version-2 layout (its done word holds nA + nB),
 *     then tile_n[th*tw], then tile_nA[th*tw]. It loads as an adaptive progression and continues to
 *     the uninterrupted run's bits. RT_ERR_ARG for a size that does not match, tile_nA outside
 *     0..tile_n, tile_n outside 0..total, or counts that mix zero and positive (no call leaves
 *     such a state: a pass either starts its pixels' chains or resumes them). Versions 1 and 2 are
 *     written and read as before.
 * rt_progress_tile_counts: th*tw int32 each (either may be NULL); waits. A tracked progression that
 *   is not adaptive yet reports done and nA in every tile.
 * RT_ERR_STATE: no progression, or an untracked one. RT_ERR_ARG: samples <= 0, a threshold that
 * is not finite and >= 0, a NULL info, a multi-device context. */
int rt_progress_advance_adaptive(rt_context* ctx, int samples, float threshold, void* stream, int info[8]);
int rt_progress_tile_counts(rt_context* ctx, int* tile_n, int* tile_nA);

/* ------------------------------------------- variance-guided denoise
 * The a-trous filter of rt_denoise with its colour edge-stop scaled per pixel by an estimate
 * of the input's variance (the spatial half of SVGF, Schied et al. 2017), and the query that
 * gives a tracked or adaptive progression's estimate in the units of the linear frame.
 * Float32 throughout, no contraction, IEEE division and square root, the library's expf.
 *
 * rt_progress_noise_sigma / _device: sigma (rows_local*w floats, required; device: 4-byte
 *   aligned, on `stream`, no wait; host: waits) receives, per pixel of the shard,
 *       s = k * d
 *   with m, a, d and k exactly as the noise estimate above computes them (s is e's numerator,
 *   before the division by sqrtf(0.01f + (m.r + m.g) + m.b)); in an adaptive progression with the
 *   pixel's tile's own counts (N = tile_n[t], nA = tile_nA[t]) in k and both divisions. A pixel
 *   whose tile has nA == 0 or nB == 0 gets what the arithmetic gives, which is not finite; it is
 *   written as it is. Changes no state. RT_ERR_STATE and RT_ERR_ARG as rt_progress_noise (not
 *   tracked, fewer than two passes; no progression on a multi-device context), RT_ERR_ARG for a
 *   NULL or misaligned sigma.
 *
 * rt_denoise_var / _device: rt_denoise's buffers plus sigma (float[h][w], required: a per-pixel
 *   standard deviation of rgba_in's colour, such as the query's) and sigma_out (float[h][w], or
 *   NULL). Prep: v_p = sigma_p * sigma_p; a NaN v becomes 0, an infinite one the largest finite
 *   float, so every v is finite and >= 0 from here on. Then `passes` iterations over the records
 *   {r, g, b, v}; pass i has step s = 1 << i and, for pixel p:
 *     g_p = sum b v_q / sum b over the 3x3 pixels q around p at unit spacing that lie inside the
 *           image (dy outer), b = {1/4, 1/2, 1/4}[dy+1] * {1/4, 1/2, 1/4}[dx+1]; every such pixel
 *           counts whatever its colour; a quotient above the largest finite float is that float
 *     r_p = (1 / sigma_color^2) / (g_p + var_floor)        the same sigma_color in every pass
 *     the taps q = p + s (dx, dy) of rt_denoise, in its order and with its skips, with
 *     e   = |c_p - c_q|^2 * r_p + |n_p - n_q|^2 / sigma_normal^2 + |a_p - a_q|^2 / sigma_albedo^2
 *         + ((t_p - t_q) / max(t_p, t_q))^2 / sigma_depth^2
 *     w   = k expf(-e)                                     k = h[dy+2] h[dx+2] as in rt_denoise
 *     out.rgb = sum w c_q / sum w      out.v = sum w (w v_q) / ((sum w) (sum w))
 *   evaluated as written (w (w v_q): w w would leave the normal range from w = 1e-19 down)
 *   (the four 1 / sigma^2 are floats computed once and multiplied in, clamped to the normal range).
 *   A tap is skipped, in all five sums, when it is outside the image, its colour is not finite,
 *   one of p and q is a hit and the other a miss, or e is not >= 0 (a NaN guide; a colour distance
 *   that overflowed while r_p is 0, which it is once g_p + var_floor is infinite). A centre whose
 *   colour is not finite, and a centre left without any tap (its own guide is NaN), keeps its
 *   record, v included. The centre tap always has e = 0, so sum w >= 9/64 wherever it is > 0; an
 *   out.v above the largest finite float is that float. After the last pass rgb = blend *
 *   filtered + (1.0f - blend) * rgba_in and alpha 1.0f, as rt_denoise, and sigma_out = sqrtf(out.v):
 *   the standard deviation left in the filtered colour, before the blend. rgba_in's alpha plays no
 *   part. A finite colour input never gives a NaN colour.
 *   RT_ERR_ARG as rt_denoise (passes outside 1..10, a sigma_* parameter that is not finite and
 *   > 0, a non-finite blend, exactly one guide NULL, rgba_in == rgba_out, more than 262140 rows
 *   or 2^27 - 1 pixels), and for a NULL sigma and a var_floor that is not finite and > 0. The
 *   device form takes device pointers (the float4 buffers 16-byte aligned, sigma and sigma_out
 *   4-byte aligned: RT_ERR_ARG otherwise) and a stream (NULL: default) and returns without
 *   waiting. params NULL: the defaults (rt_denoise_var_default_params). Runs on the root device;
 *   rt_last_kernel_ms as for rt_denoise. */
typedef struct rt_denoise_var_params {
    int passes;          /* a-trous iterations, 1..10 */
    float sigma_color;   /* colour distance in standard deviations of the input */
    float sigma_normal, sigma_albedo, sigma_depth; /* as rt_denoise_params */
    float var_floor;     /* added to the variance estimate: the edge-stop's width where sigma is 0 */
} rt_denoise_var_params;
int rt_progress_noise_sigma(rt_context* ctx, float* sigma);
int rt_progress_noise_sigma_device(rt_context* ctx, void* d_sigma, void* stream);
void rt_denoise_var_default_params(rt_denoise_var_params* params);
int rt_denoise_var(rt_context* ctx, int w, int h, const float* rgba_in, const float* sigma, const float* albedo,
                   const float* normal_depth, const rt_denoise_var_params* params, float blend, float* rgba_out,
                   float* sigma_out);
int rt_denoise_var_device(rt_context* ctx, int w, int h, const void* d_rgba_in, const void* d_sigma, const void* d_albedo,
                          const void* d_normal_depth, const rt_denoise_var_params* params, float blend, void* d_rgba_out,
                          void* d_sigma_out, void* stream);

/* ---------------------------------------------- temporal accumulation
 * The previous frame's accumulated colour, variance and history length reprojected into the
 * current camera and blended with the new frame (the temporal half of SVGF, Schied et al. 2017):
 * what rt_denoise_var then takes is an image of lower variance and a sigma map that says so.
 * Stateless: the caller owns every buffer, and one call's rgba_out, sigma_out and len_out with
 * the frame's normal_depth are the next call's history. Only the camera moves between frames.
 * Float32 throughout, no contraction, IEEE division and square root, floorf; no expf.
 *
 * rt_temporal_accumulate / _device: rgba_in (float4[h][w], a linear frame such as
 *   rt_progress_resolve_linear gives), sigma_in (float[h][w], its per-pixel standard deviation,
 *   such as rt_progress_noise_sigma's) and normal_depth (float4[h][w], rt_render_features' buffer
 *   under the context's current camera) describe this frame; prev_view (row-major 4x4) and
 *   prev_fov_dist are the camera of the history; hist_rgba, hist_sigma, hist_len and
 *   hist_normal_depth are the previous call's three outputs and the previous frame's
 *   normal_depth, all four NULL for the first frame. Outputs, all required: rgba_out
 *   (float4[h][w]), sigma_out and len_out (float[h][w]). For pixel p = (x, y), c = rgba_in[p],
 *   {n_p, t} = normal_depth[p]:
 *   1 v_c = sigma_in[p] * sigma_in[p]; a NaN v_c is 0, an infinite one the largest finite float.
 *   2 The pixel is carried over, out = {c.rgb, 1}, sigma_out = sqrtf(v_c), len_out = 1, when
 *     c.rgb is not finite, one of normal_depth[p]'s four floats is a NaN, the history is NULL,
 *     or steps 4 and 5 find no history for it.
 *   3 (o, d) = the feature pass's ray of the pixel (the context's camera, x_j = (float)x,
 *     y_j = (float)y). A hit (t > 0): P = o + t d and t_exp = |P - o_prev|, the square root of
 *     the squared distance, o_prev = the history camera's origin (its view matrix applied to 0,
 *     in float, as the render computes its own). A miss: P = o_prev + d (the environment is at
 *     infinity: only the rotation counts) and no depth or normal test below.
 *   4 q = prev_inv applied to P as a point, prev_inv being the inverse of prev_view, computed
 *     once per call in double by a general 4x4 inverse and rounded to float.
 *     ratio = q.z / prev_fov_dist; unless ratio > 0 there is no history.
 *       fx = (((q.x / ratio) / aspect + 1) * 0.5) * (float)w        aspect = (float)w / (float)h
 *       fy = ((q.y / ratio + 1) * 0.5) * (float)h
 *     the camera ray run backwards: with the same camera pixel x sits at fx = x. Unless
 *     -1 < fx < w and -1 < fy < h there is no history (every tap would lie outside the image).
 *     ix = floorf(fx), tx = fx - ix; iy and ty the same.
 *   5 The four taps (ix + dx, iy + dy), dy outer, with the bilinear weight
 *     b = (dy ? ty : 1 - ty) * (dx ? tx : 1 - tx). A tap q is skipped when b == 0, it lies
 *     outside the image, hist_len[q] is not > 0, hist_rgba[q].rgb or hist_sigma[q] is not
 *     finite, or its hit state (t_q > 0) differs from p's; for a hit p also unless
 *     |t_q - t_exp| <= depth_tol * t_exp and dot(n_p, n_q) >= normal_cos (a NaN in the tap's
 *     guide fails them). S = sum b; unless S > min_weight there is no history. Otherwise
 *       c_h = sum b c_q / S     len_h = sum b len_q / S     v_h = sum b (sigma_q sigma_q) / S
 *     v_h above the largest finite float is that float. An infinite hist_len counts.
 *   6 len = min(len_h + 1, max_len); a = 1 / len; rgb = c_h + a (c - c_h), alpha 1;
 *     v = ((1 - a) (1 - a)) v_h + a (a v_c), above the largest finite float that float;
 *     sigma_out = sqrtf(v); len_out = len.
 *   The alphas of rgba_in and hist_rgba play no part. The inputs are not written.
 *   RT_ERR_STATE without a camera (no scene, BVH or environment map is needed). RT_ERR_ARG for a
 *   NULL ctx, required buffer or prev_view; a parameter that is not finite, depth_tol < 0,
 *   normal_cos outside [-1, 1], min_weight outside [0, 1), max_len < 1; a prev_fov_dist that is
 *   zero or not finite; a prev_view that is singular or holds a non-finite entry; some but not
 *   all of the four history buffers; an output whose bytes overlap an input's or another
 *   output's; more than 262140 rows or 2^27 - 1 pixels (rt_denoise's limits). The device form
 *   takes device pointers (the float4 buffers 16-byte aligned, the float buffers 4-byte aligned:
 *   RT_ERR_ARG otherwise) and a stream (NULL: default) and returns without waiting. params NULL:
 *   the defaults (rt_temporal_default_params). Runs on the root device of a multi-device
 *   context; rt_last_kernel_ms as for rt_denoise. */
typedef struct rt_temporal_params {
    float depth_tol;   /* relative: |t_q - t_exp| <= depth_tol * t_exp             default 0.05 */
    float normal_cos;  /* dot(n_p, n_q) >= normal_cos                              default 0.9  */
    float min_weight;  /* the valid taps' bilinear weights must sum above this     default 0.1  */
    float max_len;     /* history length cap, >= 1: alpha never below 1 / max_len  default 32   */
} rt_temporal_params;
void rt_temporal_default_params(rt_temporal_params* params);
int rt_temporal_accumulate(rt_context* ctx, int w, int h, const float* rgba_in, const float* sigma_in,
                           const float* normal_depth, const float prev_view[16], float prev_fov_dist,
                           const float* hist_rgba, const float* hist_sigma, const float* hist_len,
                           const float* hist_normal_depth, const rt_temporal_params* params, float* rgba_out,
                           float* sigma_out, float* len_out);
int rt_temporal_accumulate_device(rt_context* ctx, int w, int h, const void* d_rgba_in, const void* d_sigma_in,
                                  const void* d_normal_depth, const float prev_view[16], float prev_fov_dist,
                                  const void* d_hist_rgba, const void* d_hist_sigma, const void* d_hist_len,
                                  const void* d_hist_normal_depth, const rt_temporal_params* params, void* d_rgba_out,
                                  void* d_sigma_out, void* d_len_out, void* stream);

/* ---------------------------------------------- firefly rejection
 * A linear frame of few samples carries its error in a few very bright pixels. This stage limits
 * a pixel's luminance to a multiple of a high rank of its neighbours' luminances and scales the
 * colour and the noise figure together; it goes between the linear resolve (with its
 * rt_progress_noise_sigma) and rt_temporal_accumulate / rt_denoise_var. Stateless, no scene or
 * camera needed. Float32 throughout, no contraction, IEEE division; no expf, no square root.
 *
 * rt_firefly / _device: rgba_in (float4[h][w]) and sigma_in (float[h][w], or NULL) in; rgba_out
 *   (float4[h][w], required), sigma_out (float[h][w], NULL allowed; needs a sigma_in) and
 *   scale_out (float[h][w], NULL allowed) out. For pixel p, c = rgba_in[p], s = sigma_in[p]:
 *   1 L(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b.
 *   2 The neighbours are the (2 radius + 1)^2 - 1 pixels around p. One outside the image, or whose
 *     rgb is not all finite, is dropped. Every neighbour is read from rgba_in.
 *   3 M = the rank-th largest L over the neighbours kept, each L taken as at least -FLT_MAX. With
 *     fewer than `rank` neighbours kept the pixel is untouched.
 *   4 limit = gain * M + floor.
 *   5 When c.rgb is all finite, limit > 0 and L(c) > limit: f = limit / L(c), rgba_out = {f c.rgb,
 *     c.a}, sigma_out = f s (a NaN or infinite s is copied instead), scale_out = f, which lies in
 *     (0, 1) (0 only where the division underflows). Otherwise rgba_out = c and sigma_out = s bit
 *     for bit and scale_out = 1: a centre that is not finite (rt_denoise_var's rule for it), a
 *     limit that is zero, negative or a NaN, a centre luminance that is negative or not above it.
 *   gain = +inf is the identity. The caller counts the clamped pixels as scale_out < 1.
 *   RT_ERR_ARG for a NULL ctx, rgba_in or rgba_out; sigma_out without sigma_in; w or h below 1;
 *   radius outside {1, 2}; rank outside 1..8; a NaN or negative gain; a NaN floor; an output whose
 *   bytes overlap an input's or another output's; more than 262140 rows or 2^27 - 1 pixels
 *   (rt_denoise's limits). The device form takes device pointers (the float4 buffers 16-byte
 *   aligned, the float buffers 4-byte aligned: RT_ERR_ARG otherwise) and a stream (NULL: default)
 *   and returns without waiting. params NULL: the defaults (rt_firefly_default_params). Runs on
 *   the root device of a multi-device context; rt_last_kernel_ms as for rt_denoise. */
typedef struct rt_firefly_params {
    int radius;   /* neighbourhood half-width, 1 (3x3) or 2 (5x5)                            default 1 */
    int rank;     /* M is the rank-th largest neighbour luminance, 1..8                      default 2 */
    float gain;   /* limit = gain * M + floor; >= 0, +inf: the identity                      default 2 */
    float floor;  /* added to the limit: the luminance below which nothing is ever clamped   default 0 */
} rt_firefly_params;
void rt_firefly_default_params(rt_firefly_params* params);
int rt_firefly(rt_context* ctx, int w, int h, const float* rgba_in, const float* sigma_in, const rt_firefly_params* params,
               float* rgba_out, float* sigma_out, float* scale_out);
int rt_firefly_device(rt_context* ctx, int w, int h, const void* d_rgba_in, const void* d_sigma_in,
                      const rt_firefly_params* params, void* d_rgba_out, void* d_sigma_out, void* d_scale_out, void* stream);

/* ---------------------------------------------- exposure metering
 * What exposure rt_display should take for a linear frame: a log-luminance histogram of the frame
 * (a gfx950 kernel, integer counts: the same words as the CPU build in any execution order) and a
 * host-only solve that turns the histogram into the exposure of rt_display's curve 1 - exp(-x e).
 * It goes behind the last stage that changes the linear frame and in front of rt_display.
 *
 * rt_meter / _device: every pixel of a w x h float4 linear frame is classified; alpha is ignored.
 *   1 L = (0.2126f * r + 0.7152f * g) + 0.0722f * b (rt_firefly's luminance, no contraction).
 *   2 r, g, b or L not finite: nonfinite. Else L <= 0 (-0 too): nonpositive. Neither is binned.
 *   3 Else k = bits(L) >> 20 (exponent and top 3 mantissa bits), bin = clamp(k - 856, 0, 255):
 *     256 bins, eight per octave, over [2^-20, 2^12); bin b starts at asfloat((b + 856) << 20).
 *     k < 856 (denormals too) counts `under` and lands in bin 0; k > 1111 counts `over` and lands
 *     in bin 255. `counted` goes up; bits(L) is folded into max_bits and min_bits (0 and
 *     0xFFFFFFFF when nothing was counted). No libm call.
 *   The bins sum to counted, and counted + nonpositive + nonfinite = w h. No scene has to be bound.
 *   RT_ERR_ARG: a NULL ctx, frame or histogram, non-positive sizes, more than 2^27 - 1 pixels
 *   (rt_display's limit: no word can overflow). The device form takes device pointers (d_linear
 *   16-byte aligned, d_hist 4-byte aligned with room for 264 words: RT_ERR_ARG otherwise) and a
 *   stream (NULL: default), clears d_hist on that stream itself and returns without waiting; the
 *   host form takes any alignment. The input is not written. Runs on the root device of a
 *   multi-device context and restores the caller's current device; rt_last_kernel_ms as for
 *   rt_display.
 * rt_meter_solve (host only, no context, double arithmetic): n = counted, lo = floor(low n),
 *   hi = floor((1 - high) n); with lo + hi >= n nothing is trimmed.
 *   1 lo samples are removed from the lowest bins upward and hi from the highest downward: c'_b,
 *     N' = sum c'_b.
 *   2 Bin b stands for the log2 luminance (2 b - 319) / 16, its middle. S = sum c'_b (2 b - 319),
 *     an exact integer; log2_mean = S / (16 N'), L_m = exp2(log2_mean).
 *   3 target = clamp(-log1p(-key) / L_m, min_exposure, max_exposure): the exposure at which L_m
 *     displays as `key` before the gamma.
 *   4 tau = tau_up if target > prev_exposure, else tau_down. With prev_exposure > 0, tau > 0 and
 *     dt_seconds >= 0: log2 e = log2 prev + (log2 target - log2 prev) (1 - exp(-dt / tau)).
 *     Otherwise e = target.
 *   5 N' = 0: exposure = target = prev_exposure when that is > 0, else 1.5; log2_mean = 0, valid = 0.
 *   params NULL: the defaults. RT_ERR_ARG: a NULL histogram or result; low or high outside [0, 1]
 *   or low > high; key outside (0, 1); bounds that are not finite, not positive or inverted; a
 *   negative or NaN tau_up or tau_down. The message is rt_last_error(NULL)'s. */
typedef struct rt_meter_hist {
    unsigned int bins[256];
    unsigned int counted;      /* pixels binned: finite, luminance > 0 */
    unsigned int under;        /* of those, below 2^-20 (in bin 0) */
    unsigned int over;         /* of those, at or above 2^12 (in bin 255) */
    unsigned int nonpositive;  /* finite pixels of luminance <= 0, not binned */
    unsigned int nonfinite;    /* pixels with a NaN or an infinity in r, g, b or the luminance, not binned */
    unsigned int max_bits;     /* the largest and ... */
    unsigned int min_bits;     /* ... smallest binned luminance, as the float's bits */
    unsigned int reserved;     /* 0 */
} rt_meter_hist;
typedef struct rt_meter_params {
    float low;           /* share of the counted pixels trimmed from the dark end     default 0.10 */
    float high;          /* ... 1 - the share trimmed from the bright end             default 0.95 */
    float key;           /* the display value, before the gamma, the log-average luminance maps to; the
                            photographic convention, not a measured optimum            default 0.18 */
    float min_exposure;  /* the target is clamped to [min_exposure, ...               default 2^-8 */
    float max_exposure;  /* ... max_exposure]                                          default 2^12 */
    float tau_up;        /* time constant in seconds while the exposure rises; 0: at once   default 0 */
    float tau_down;      /* ... and while it falls                                     default 0 */
} rt_meter_params;
typedef struct rt_meter_result {
    float exposure;      /* what rt_display_params.exposure takes */
    float target;        /* the exposure before the adaptation */
    float log2_mean;     /* log2 of the trimmed log-average luminance */
    int valid;           /* 0: no pixel was left to average */
} rt_meter_result;
void rt_meter_default_params(rt_meter_params* params);
int rt_meter(rt_context* ctx, int w, int h, const float* linear_rgba, rt_meter_hist* out);
int rt_meter_device(rt_context* ctx, int w, int h, const void* d_linear, void* d_hist, void* stream);
int rt_meter_solve(const rt_meter_hist* hist, const rt_meter_params* params, float prev_exposure, float dt_seconds,
                   rt_meter_result* out);

/* ---------------------------------------------- guided upscale
 * Render small, reconstruct at full size: a frame of w_lo x h_lo pixels (rt_render_linear or a
 * progression's linear resolve, optionally with its rt_progress_noise_sigma) is taken to w x h by
 * joint-bilateral upsampling. Each low-resolution tap is weighted by how well its first-hit guides
 * (rt_render_features at w_lo x h_lo) agree with the output pixel's (rt_render_features at w x h),
 * so geometry, material and silhouette edges come out at output resolution; the colour itself is
 * never compared. The camera maps a pixel through x / w, so the two sizes see the same field of
 * view when their aspects agree. Stateless, no scene or camera needed. Float32 throughout, no
 * contraction, IEEE division and square root, rt_libm's expf.
 *
 * rt_upscale / _device: rgba_lo, albedo_lo, normal_depth_lo (float4[h_lo][w_lo]), sigma_lo
 *   (float[h_lo][w_lo], or NULL), albedo_hi, normal_depth_hi (float4[h][w]) in; rgba_out
 *   (float4[h][w], alpha 1) and sigma_out (float[h][w]; required exactly when sigma_lo is given) out.
 *   With sx = (float)w_lo / (float)w, sy = (float)h_lo / (float)h, for output pixel (X, Y):
 *   fx = (float)X * sx, x0 = (int)fx, tx = fx - (float)x0, the same in y (no half-pixel term: the
 *   feature rays aim at x_j = x).
 *   Guide weight of low tap q against output pixel p: skipped when their hit states (t > 0) differ;
 *   e = |n_p - n_q|^2 / sigma_normal^2 + |a_p - a_q|^2 / sigma_albedo^2, plus ((t_p - t_q) /
 *   max(t_p, t_q))^2 / sigma_depth^2 when both hit; skipped when !(e >= 0); g = expf(-e). A tap
 *   outside the low frame, with a colour that is not finite, with a sigma that is not finite (when
 *   given) or with a spatial weight of exactly 0 is skipped too.
 *   1 The taps (x0 + dx, y0 + dy), dx, dy in {0, 1}, dy outer, spatial weight b = (1 - ty, ty)[dy] *
 *     (1 - tx, tx)[dx], wgt = b g; sums of wgt c, S = sum wgt, V = sum wgt (wgt v_q) in tap order,
 *     v_q = sigma_q^2, at most the largest float. Taken when S > min_weight.
 *   2 Otherwise dx, dy in {-1, 0, 1, 2}, dy outer, b = k(y) k(x), k(d) = 1 - |d| / 2 at d =
 *     (float)(x0 + dx) - fx; the same guide weight and sums. Taken when S > 0.
 *   3 Otherwise the taps and weights of 1 with g = 1: plain bilinear over the finite taps inside the
 *     frame. Taken when S > 0. Otherwise rgba_out = {0, 0, 0, 1} and sigma_out = +inf.
 *   rgb = sums / S; sigma_out = sqrtf(min(V, largest float)) / S. Neighbouring outputs share taps:
 *   sigma_out is each pixel's marginal figure, not that of an independent sample. Where step 2 is
 *   taken with no agreeing tap (every weight below about 1e-19, S of that order) V is a denormal
 *   float and sigma_out is unreliable, off by up to sqrt(2^-144) / S: a caller that feeds sigma_out
 *   to rt_denoise_var or a history should not trust it at such pixels. rgba_out is not affected.
 *   A NaN or infinite output guide, or an output pixel whose hit state no tap shares, therefore gets
 *   the bilinear value. With w_lo == w, h_lo == h (at most 2^24 a side) and the same guides on both
 *   sides rgba_out equals rgba_lo's rgb bit for bit wherever colour and sigma are finite, and
 *   sigma_out equals a sigma_lo >= 0 whose square is a normal float.
 *   RT_ERR_ARG for a NULL ctx or required buffer; a size below 1; w_lo > w or h_lo > h; sigma_out
 *   without sigma_lo or the reverse; a sigma that is not positive and finite; min_weight outside
 *   [0, 1); an output whose bytes overlap an input's or the other output's; more than 262140 output
 *   rows or 2^27 - 1 output pixels (rt_denoise's limits). The device form takes device pointers (the
 *   float4 buffers 16-byte aligned, the float buffers 4-byte aligned: RT_ERR_ARG otherwise) and a
 *   stream (NULL: default) and returns without waiting. params NULL: the defaults. Runs on the
 *   root device of a multi-device context; rt_last_kernel_ms as for rt_denoise. */
typedef struct rt_upscale_params {
    float sigma_normal; /* guide edge-stops, as rt_denoise_params'             defaults: rt_denoise's */
    float sigma_albedo;
    float sigma_depth;
    float min_weight;   /* tier 1 is taken when its weight sum is above this, [0, 1)      default 0.1 */
} rt_upscale_params;
void rt_upscale_default_params(rt_upscale_params* params);
int rt_upscale(rt_context* ctx, int w_lo, int h_lo, int w, int h, const float* rgba_lo, const float* sigma_lo,
               const float* albedo_lo, const float* normal_depth_lo, const float* albedo_hi, const float* normal_depth_hi,
               const rt_upscale_params* params, float* rgba_out, float* sigma_out);
int rt_upscale_device(rt_context* ctx, int w_lo, int h_lo, int w, int h, const void* d_rgba_lo, const void* d_sigma_lo,
                      const void* d_albedo_lo, const void* d_normal_depth_lo, const void* d_albedo_hi,
                      const void* d_normal_depth_hi, const rt_upscale_params* params, void* d_rgba_out, void* d_sigma_out,
                      void* stream);

/* ---------------------------------------------- bloom
 * A light many times brighter than what rt_display maps to white clips to a flat, hard-edged patch.
 * This stage spreads the energy above a luminance threshold with a Gaussian pyramid and adds it back;
 * it goes behind the last stage that changes the linear frame and in front of rt_display (meter the
 * frame before it, so that the exposure does not chase the glow). Stateless, no scene or camera
 * needed. Float32 throughout, no contraction, IEEE division; no expf, no square root.
 *
 * rt_bloom / _device: linear_rgba (float4[h][w]) in; rgba_out (float4[h][w], required) and layer_out
 *   (float4[h][w], NULL allowed) out. For pixel p, c = linear_rgba[p]:
 *   1 Bright pass. L = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b (rt_firefly's luminance);
 *     s = min(max((L - threshold) + knee, 0), 2 knee); q = knee > 0 ? s s / (4 knee) : 0;
 *     e = max(q, L - threshold); b = e > 0 ? c.rgb (e / L) : 0. A pixel whose rgb is not all finite,
 *     or whose L is not finite, gives b = 0.
 *   2 Reduce, k = 1..levels: level k has (w_{k-1} + 1) / 2 x (h_{k-1} + 1) / 2 texels (level 0: b at
 *     w x h); g_k(x, y) = sum over m, n = -2..2 of W[m] W[n] g_{k-1}(2x + m, 2y + n), W = {1, 4, 6,
 *     4, 1} / 16, coordinates clamped to the edge of level k-1; the five row sums first, each in
 *     ascending m, then the column sum in ascending n, every addition left to right.
 *   3 Expand and accumulate: u_levels = g_levels; k = levels-1 .. 1: u_k = g_k + expand(u_{k+1}).
 *     expand at (x, y) from a w' x h' level: xs = x >> 1, xn = clamp(xs + (x odd ? 1 : -1), 0, w' - 1),
 *     ys, yn likewise; row(yy) = 0.75 g(xs, yy) + 0.25 g(xn, yy); value = 0.75 row(ys) + 0.25 row(yn).
 *   4 B = expand(u_1) at w x h; scale = intensity / levels (one float division); rgba_out = {c.rgb +
 *     scale B, c.a}. A centre whose rgb is not all finite is copied bit for bit and, its b being 0,
 *     does not leak into its neighbours.
 *   5 layer_out = {scale B, 0}.
 *   A frame with nothing above threshold - knee, or intensity 0, comes back equal to its input as
 *   values (a -0 channel as +0; alpha bit for bit), with a layer of zeroes. Nothing is clamped: a
 *   negative channel of a bright pixel spreads as negative glow, and a sum that passes the largest
 *   float is an infinity. The input is not written.
 *   RT_ERR_ARG for a NULL ctx, linear_rgba or rgba_out; w or h below 1; levels outside 1..8; a
 *   threshold, knee or intensity that is negative, a NaN or an infinity; knee > threshold; an output
 *   whose bytes overlap the input's or the other output's; more than 262140 rows or 2^27 - 1 pixels
 *   (rt_denoise's limits). The device form takes device pointers (16-byte aligned: RT_ERR_ARG
 *   otherwise) and a stream (NULL: default) and returns without waiting; the pyramid, about a third of
 *   the frame's bytes, is a buffer of the context reused across calls and sizes, so two device-form
 *   calls of one context must not run at the same time on different streams. params NULL: the
 *   defaults (rt_bloom_default_params). Runs on the root device of a multi-device context;
 *   rt_last_kernel_ms as for rt_denoise. */
typedef struct rt_bloom_params {
    float threshold;  /* luminance above which a pixel glows; >= 0                              default 1   */
    float knee;       /* half-width of the soft transition below the threshold; 0 .. threshold  default 0.5 */
    float intensity;  /* the glow added is intensity / levels times the pyramid's sum; >= 0     default 0.2 */
    int levels;       /* pyramid levels, 1..8: each doubles the glow's reach                    default 5   */
} rt_bloom_params;
void rt_bloom_default_params(rt_bloom_params* params);
int rt_bloom(rt_context* ctx, int w, int h, const float* linear_rgba, const rt_bloom_params* params, float* rgba_out,
             float* layer_out);
int rt_bloom_device(rt_context* ctx, int w, int h, const void* d_linear, const rt_bloom_params* params, void* d_rgba_out,
                    void* d_layer_out, void* stream);

/* ---------------------------------------------- depth of field
 * The render's camera is a pinhole: every frame is sharp from the near plane to the sky. This stage
 * builds a thin lens's blur from the sharp linear frame and the first-hit distance the guides hold
 * (normal_depth.w of rt_render_features or rt_render_gbuffer at the same size). It goes behind the
 * last filter or upscale, which need pinhole guides, and in front of rt_bloom, rt_meter and
 * rt_display, so that a highlight many times over white becomes a disc in linear radiance and then
 * glows. Stateless, no scene or camera needed. Float32 throughout, no contraction, IEEE division; no
 * expf, and no square root on the device.
 *
 * rt_dof / _device: linear_rgba (float4[h][w]) and normal_depth (float4[h][w]; only .w = t, the
 *   distance along the camera ray, is read) in; rgba_out (float4[h][w], required) and coc_out
 *   (float[h][w], NULL allowed) out. R = (float)max_radius. For pixel p, c = linear_rgba[p]:
 *   1 Radius. far(p): t_p is not finite or not > 0 (a miss, a zero, a NaN). r_p = far ? min(coc_inf, R)
 *     : min(coc_inf * (fabsf(t_p - focus) / t_p), R); coc_out[p] = r_p. For the ordering below a far
 *     pixel's distance is +inf. The thin lens's circle of confusion with aperture and focal length
 *     folded into its limit at infinity, coc_inf, in pixels. t runs along the ray, so the surface in
 *     focus is a sphere about the eye; the planar form needs the camera and is not offered.
 *   2 Gather. The taps q = p + (dx, dy), dy outer, dx inner, both -max_radius .. max_radius
 *     ascending; a tap outside the image or whose rgb is not all finite is skipped. Else
 *     re = (t_q > t_p) ? min(r_q, r_p) : r_q (a background tap spreads no further onto p than p's
 *     own blur: a sharp foreground stays sharp); a = min((re + 0.5f) - D, 1.0f), D the float nearest
 *     sqrt(dx^2 + dy^2) from a table built on the host; the tap is skipped unless a > 0;
 *     k(r) = 1.0f / (max(r, 0.5f) * max(r, 0.5f)); wq = a * k(re); S += wq * c_q.rgb, W += wq, each
 *     product formed and then added, in tap order.
 *   3 rgba_out[p] = {S / W, c.a}. A centre whose rgb is not all finite is copied bit for bit; any
 *     other centre's own tap has a > 0, so W > 0.
 *   A skipped tap adds nothing. The gather is normalised, not energy-conserving: a pixel is a
 *   weighted mean of what reaches it. coc_inf 0, or every t equal to focus, returns the input as
 *   values (one tap of weight 2: 2c / 2). Nothing is clamped; a channel above half the largest
 *   float sums to an infinity; a -0 channel comes back +0 (S starts at +0). With coc_inf 0 every
 *   radius is 0, also where the ratio overflows. The input is not written.
 *   RT_ERR_ARG for a NULL ctx, linear_rgba, normal_depth or rgba_out; w or h below 1; max_radius
 *   outside 1..12; a focus that is not finite and > 0; a coc_inf that is negative, a NaN or an
 *   infinity; an output whose bytes overlap an input's or the other output's; more than 262140 rows
 *   or 2^27 - 1 pixels (rt_denoise's limits). The device form takes device pointers (the float4
 *   buffers 16-byte aligned, coc_out 4-byte aligned: RT_ERR_ARG otherwise) and a stream (NULL:
 *   default) and returns without waiting. params NULL: the defaults (rt_dof_default_params). Runs on
 *   the root device of a multi-device context; rt_last_kernel_ms as for rt_denoise. */
typedef struct rt_dof_params {
    float focus;      /* ray distance in focus, > 0, finite                          default 1  */
    float coc_inf;    /* radius in pixels of a point infinitely far away, >= 0       default 4  */
    int   max_radius; /* radii are clamped to it; gather window, 1..12               default 8  */
} rt_dof_params;
void rt_dof_default_params(rt_dof_params* params);
int rt_dof(rt_context* ctx, int w, int h, const float* linear_rgba, const float* normal_depth, const rt_dof_params* params,
           float* rgba_out, float* coc_out);
int rt_dof_device(rt_context* ctx, int w, int h, const void* d_linear, const void* d_normal_depth, const rt_dof_params* params,
                  void* d_rgba_out, void* d_coc_out, void* stream);

/* ---------------------------------------------- motion vectors and motion blur
 * The render has no shutter: every frame is an instantaneous exposure, and a camera flown through a
 * scene gives sharp, strobing frames. These two stages build a shutter's blur from the sharp linear
 * frame, the guides and the previous camera. rt_motion_blur goes behind rt_dof and in front of
 * rt_bloom, rt_meter and rt_display. Both are stateless. Float32 throughout, no contraction, IEEE
 * division, a correctly rounded square root, floorf; no expf.
 *
 * rt_motion_vectors / _device: normal_depth (float4[h][w], the guides under the context's current
 *   camera: rt_render_features or rt_render_gbuffer), prev_view[16] (row-major) and prev_fov_dist in;
 *   motion_out (float2[h][w]) out. For pixel p = (x, y): (fx, fy) are rt_temporal_accumulate's steps
 *   3 and 4, the same expressions in the same order (feature_ray; P = o + t d for a hit, o_prev + d
 *   for a miss; q = the point in the previous camera's frame; ratio = q.z / prev_fov_dist;
 *   fx = (((q.x / ratio) / aspect + 1) * 0.5) * (float)w, fy = ((q.y / ratio + 1) * 0.5) * (float)h);
 *   m_p = {fx - (float)x, fy - (float)y}: where the point was, minus where it is now. m_p = {0, 0}
 *   when one of the guide's four floats is a NaN, when ratio is not > 0, or when fx or fy is not
 *   finite. Temporal's range test is not applied: a point that came from off-screen still moved.
 *   A miss moves by the rotation only. RT_ERR_STATE without a camera; RT_ERR_ARG as
 *   rt_temporal_accumulate for prev_view (singular, not finite), prev_fov_dist (zero, not finite),
 *   NULL buffers, sizes and overlap; the device form takes device pointers (normal_depth 16-byte
 *   aligned, motion_out 8-byte aligned) and a stream (NULL: default) and returns without waiting.
 *
 * rt_motion_blur / _device: linear_rgba (float4[h][w]), normal_depth (float4[h][w]; only .w = t is
 *   read), motion (float2[h][w]: rt_motion_vectors' output or the caller's own, for example object
 *   motion from elsewhere) in; rgba_out (float4[h][w], required) and reach_out (float[h][w], NULL
 *   allowed) out. No scene or camera is needed. R = (float)max_radius. After McGuire et al. 2012, "A
 *   Reconstruction Filter for Plausible Motion Blur", with nearest taps and a hard cylinder.
 *   1 Reach per pixel. a = 0.5f * shutter, hx = a * m.x, hy = a * m.y, l2 = hx*hx + hy*hy. l2 not
 *     finite: h = 0, l = 0. Else l = sqrt(l2); when l > R: s = R / l, hx *= s, hy *= s, l = R.
 *     reach_out[p] = l. k_p = 1.0f / max(l, 0.5f). t'_p = (t finite and > 0) ? min(t, 1e30f) : 1e30f.
 *     iz_p = 1.0f / (depth_soft * t'_p).
 *   2 Tile max. Motion tiles are 16 x 16 pixels, partial at the right and bottom edges. A tile's
 *     record {hx, hy, l} is that of its pixel of largest l, the first in raster order among equals.
 *   3 Neighbour max. The tile and its up to eight neighbours inside the tile grid, dy outer, dx
 *     inner; the first one's record, then a strictly larger l replaces it: {Nx, Ny, L}.
 *   4 Gather. Unless L >= 0.5f every pixel of the tile is copied bit for bit. Else n = ceil(L) (as
 *     (int)floorf(L), plus one when (float)n < L), dx = Nx / (float)n, dy = Ny / (float)n,
 *     ds = L / (float)n. Taps j = -n .. n ascending; j = 0 is the centre with weight k_p; the others
 *     lie at q = p + (ox_j, oy_j), ox_j = (int)floorf((float)j * dx + 0.5f), oy_j likewise. A tap
 *     outside the image or whose rgb is not all finite is skipped. Else d = (float)|j| * ds,
 *     fore = clamp01(1 - (t'_q - t'_p) * iz_p), back = clamp01(1 - (t'_p - t'_q) * iz_p),
 *     cone(d, k) = max(1 - d * k, 0), cyl(d, l) = d <= l ? 1 : 0,
 *     alpha = fore * cone(d, k_q) + back * cone(d, k_p) + 2 * (cyl(d, l_q) * cyl(d, l_p)), products
 *     formed, then added left to right; S += alpha * c_q.rgb, W += alpha, in tap order.
 *   5 rgba_out[p] = {S / W, c.a}. A centre whose rgb is not all finite is copied bit for bit; any
 *     other centre has W >= k_p > 0.
 *   A skipped tap adds nothing. Nothing is clamped. clamp01 of a NaN is 0. The inputs are not
 *   written. A still pixel takes nothing from still neighbours at any depth, and nothing from moving
 *   taps more than depth_soft behind it: it then comes back exactly. A moving nearer tap bleeds
 *   over a still pixel up to its own reach and no further. shutter 0, or a motion of zeroes, returns
 *   the input's bits. A gathered channel of -0 comes back +0.
 *   RT_ERR_ARG for a NULL ctx, linear_rgba, normal_depth, motion or rgba_out; w or h below 1;
 *   max_radius outside 1..16; a shutter outside [0, 1] or a NaN; a depth_soft that is not finite and
 *   > 0; an output whose bytes overlap an input's or the other output's; more than 262140 rows or
 *   2^27 - 1 pixels (rt_denoise's limits). The device form takes device pointers (the float4 buffers
 *   16-byte aligned, motion 8-byte, reach_out 4-byte: RT_ERR_ARG otherwise) and a stream (NULL:
 *   default) and returns without waiting; the tile records live in a buffer of the context, so two
 *   device-form calls on different streams must not overlap in time. params NULL: the defaults
 *   (rt_motion_default_params). Both run on the root device of a multi-device context;
 *   rt_last_kernel_ms as for rt_denoise. */
typedef struct rt_motion_params {
    float shutter;     /* share of the frame interval the shutter is open, 0..1   default 0.5  */
    float depth_soft;  /* relative depth over which fore/back fade, > 0, finite   default 0.05 */
    int   max_radius;  /* half-length of the longest streak in pixels, 1..16      default 8    */
} rt_motion_params;
void rt_motion_default_params(rt_motion_params* params);
int rt_motion_vectors(rt_context* ctx, int w, int h, const float* normal_depth, const float prev_view[16], float prev_fov_dist,
                      float* motion_out);
int rt_motion_vectors_device(rt_context* ctx, int w, int h, const void* d_normal_depth, const float prev_view[16],
                             float prev_fov_dist, void* d_motion_out, void* stream);
int rt_motion_blur(rt_context* ctx, int w, int h, const float* linear_rgba, const float* normal_depth, const float* motion,
                   const rt_motion_params* params, float* rgba_out, float* reach_out);
int rt_motion_blur_device(rt_context* ctx, int w, int h, const void* d_linear, const void* d_normal_depth, const void* d_motion,
                          const rt_motion_params* params, void* d_rgba_out, void* d_reach_out, void* stream);

/* Counters of the last render when enabled (RT_STAT_* order, rt_device.h);
 * with n up to 2 * RT_STAT_COUNT the second block is the share of the
 * gfx950 tail kernel (k_tail) in those totals. */
/* enabled = 2: counters of a render whose occlusion walks take one node per trip
 * (the gfx950 walks otherwise pair the stack top's node into the same trip, testing
 * boxes a one-node walk may never reach) and whose walks are all quad walks (no
 * 16-wide row trips in k_trace's drains or the tail kernel): the box tests a walk
 * must make, for the roofline's necessary-bytes figure. Same answers, same frame. */
int rt_set_stats(rt_context* ctx, int enabled);
int rt_get_stats(const rt_context* ctx, unsigned long long* out, int n);
/* Average duration (ms) of the last render kernel measured with HIP events. */
double rt_last_kernel_ms(const rt_context* ctx);

/* ------------------------------------------------- host helpers (no GPU) */
int rt_mesh_load(const char* obj_path, rt_mesh** out);
int rt_mesh_counts(const rt_mesh* m, int* n_triangles, int* n_materials, int* n_emissive);
int rt_mesh_copy(const rt_mesh* m, float* triangles, int* material_indices, float* materials, int* emissive);
void rt_mesh_free(rt_mesh* m);
int rt_camera_preset(const char* name, float view[16], float* fov_dist);
int rt_env_luminance_cdf(const float* pixels, int width, int height, int channels, float* lum, float* cdf);
/* Utils::read_image_float (utils.cpp:100-124) on a Radiance .hdr file, decoded
 * like stb_image 2.28 (stb_image.h:7157-7286) and flipped vertically when
 * flip_y (the reference's default). Call with pixels_rgba == NULL to get the
 * size, then with a w*h*4 float buffer: RGBA, alpha 0 (utils.cpp:119). */
int rt_read_hdr(const char* path, int flip_y, int* width, int* height, float* pixels_rgba);
/* write_image_png (image_io.cpp:165-182): RGBA f32 -> 8 bit exactly as the
 * reference converts (x*255, clamp to [0,255], truncate), rows flipped when
 * flip_y, written as a PNG. rt_image_to_rgba8 is the conversion alone. */
int rt_write_png(const char* path, const float* rgba, int width, int height, int flip_y);
int rt_image_to_rgba8(const float* rgba, long n_pixels, unsigned char* out);
/* TEST ONLY. rt_mesh_load parses files of at least `bytes` in chunks on worker
 * threads (-1: the default, 4 MB; 0: every file, so small test files take the
 * chunked path). */
int rt_test_obj_parallel_min(long bytes);
/* Octree of a triangle buffer without a device (parity tests). */
long rt_octree_dump(const float* triangles, int n_triangles, int max_depth, int leaf_max, void* buf, long capacity);

#ifdef __cplusplus
}
#endif

#endif /* RT_HIP_H */
