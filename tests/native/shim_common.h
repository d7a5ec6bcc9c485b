// shim_common.h — what the drop-in's stand-alone checks (shim_test.cpp and the *_shim_test.cpp files beside
// it) share: the scene they load, the sky file they read, and the few helpers their verdicts are made of.
// Each program compiles include/render_kernel_hip.h against the reference's own headers and objects, links
// the hostsim build of the C ABI (build/X) or the product library (build/X_hip, for the GPU run), checks
// one part of the drop-in, prints one verdict line and returns 0 when every check held;
// tests/test_shims.py holds the table of invocations and runs both forms.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <stdexcept>
#include <vector>

#include "image.h"
#include "utils.h"
#include "render_kernel_hip.h"

namespace shim {

// A sky file (int w, h; float rgb[h][w][3]), or for "-" a flat grey sky of 8 x 4 texels.
inline Image read_sky_raw(const char* path)
{
    if (std::strcmp(path, "-") == 0) return Image(8, 4, Color(0.5f, 0.5f, 0.5f, 0.0f));
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(3);
    int wh[2];
    if (std::fread(wh, 4, 2, f) != 2) std::exit(3);
    std::vector<float> rgb((size_t)wh[0] * wh[1] * 3);
    if (std::fread(rgb.data(), 4, rgb.size(), f) != rgb.size()) std::exit(3);
    std::fclose(f);
    Image out(wh[0], wh[1]);
    for (int i = 0; i < wh[0] * wh[1]; i++) out[i] = Color(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f);
    return out;
}

// What the reference's main.cpp loads before it constructs a kernel: the parsed OBJ, its BVH, the sky with
// its CDF, and no analytic spheres. Without a sky path the sky is one black texel and the CDF is empty (the
// ray queries need neither). bvh points into obj.triangles and every kernel keeps references to the
// vectors, so a Scene is constructed in place and is neither copyable nor movable.
struct Scene {
    ParsedOBJ obj;
    BVH bvh;
    Image sky;
    std::vector<float> cdf;
    std::vector<Sphere> spheres;

    explicit Scene(const char* obj_path, const char* sky_path = nullptr)
        : obj(Utils::parse_obj(obj_path)), bvh(&obj.triangles), sky(sky_path ? read_sky_raw(sky_path) : Image(1, 1)),
          cdf(sky_path ? Utils::compute_env_map_cdf(sky) : std::vector<float>())
    {
    }
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;

    // the drop-in's constructor over this scene, rendering into fb (the result is constructed in the caller's
    // variable: a RenderKernel does not move either)
    RenderKernel kernel(int W, int H, int spp, int bounces, Image& fb)
    {
        return RenderKernel(W, H, spp, bounces, fb, obj.triangles, obj.materials, obj.emissive_triangle_indices,
                            obj.material_indices, spheres, bvh, sky, cdf);
    }

    // a second context for the C calls, bound to the same triangles and materials with the BVH built
    // (rc: the first failure of a chain of C calls, as in `rc = rc ? rc : rt_...`)
    rt_context* c_context(int& rc) const
    {
        rt_context* c = nullptr;
        rc = rc ? rc : rt_create(0, &c);
        rc = rc ? rc : rt_set_scene(c, reinterpret_cast<const float*>(obj.triangles.data()), (int)obj.triangles.size(),
                                    obj.material_indices.data(), (int)obj.material_indices.size(),
                                    reinterpret_cast<const float*>(obj.materials.data()), (int)obj.materials.size(),
                                    obj.emissive_triangle_indices.data(), (int)obj.emissive_triangle_indices.size(),
                                    nullptr, 0);
        rc = rc ? rc : rt_build_bvh(c, 32, 8);
        return c;
    }
};

// true when fn throws std::runtime_error (what the drop-in makes of a C call's failure)
template <class F>
bool throws(F&& fn)
{
    try {
        fn();
    } catch (const std::runtime_error&) {
        return true;
    }
    return false;
}

// a's floats equal b's bit for bit. a is an Image or a vector; b is one too, of the same length, or a raw
// buffer taken to be as long as a.
inline const float* floats(const Image& v) { return v.data(); }
inline const float* floats(const std::vector<float>& v) { return v.data(); }
inline const float* floats(const float* p) { return p; }
inline size_t n_floats(const Image& v, size_t = 0) { return (size_t)v.size() * 4; }
inline size_t n_floats(const std::vector<float>& v, size_t = 0) { return v.size(); }
inline size_t n_floats(const float*, size_t n) { return n; }
template <class A, class B>
bool same_bits(const A& a, const B& b)
{
    const size_t n = n_floats(a);
    return n == n_floats(b, n) && std::memcmp(floats(a), floats(b), n * sizeof(float)) == 0;
}

// after a chain of C calls: reports the first failure; the program then returns 1
inline bool c_abi_failed(int rc)
{
    if (rc) std::printf("C ABI failed: %d %s\n", rc, rt_last_error(nullptr));
    return rc != 0;
}

// the verdict line "TAG name 0|1 name 0|1 ..." and the exit status: 0 when every field is 1
struct Field {
    const char* name;
    bool ok;
};
inline int verdict(const char* tag, std::initializer_list<Field> fields)
{
    bool all = true;
    std::printf("%s", tag);
    for (const Field& f : fields) {
        std::printf(" %s %d", f.name, f.ok ? 1 : 0);
        all = all && f.ok;
    }
    std::printf("\n");
    return all ? 0 : 1;
}

}  // namespace shim
