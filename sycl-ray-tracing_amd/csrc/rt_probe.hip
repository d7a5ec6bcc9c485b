// rt_probe.hip — kernels no render launches, with their C hooks: rt_intersect's exact walk
// (k_intersect, rt_backend_intersect: product API), the search-BVH query micro-benchmark
// (k_query*, rt_device_queries) and the device self-tests of the numerics and the env-CDF
// search (k_libm, k_libm_digest, k_env_search). A translation unit of its own, so that an edit here leaves
// the render kernels of rt_render.hip compiled exactly as they were.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "rt_backend_hip.h"
#include "rt_digest.h"
#include "rt_wave.h"
#include "rt_wave_layout.h"
#include "rt_quad.h"
#include "rt_row.h"

namespace {

#define RT_LDS_CAP_FAST 16      // search-BVH stack: node + key in LDS ...
#define RT_SPILL_FAST RT_FAST_SPILL  // ... then in the lane's global spill area

// Search-BVH stack of a fast query: entries [0, N) in LDS (entry i of
// thread t at [i * 256 + t]: a wave at equal depth touches 64 consecutive
// words), the rest in the lane's global spill area (deep stacks are rare).
template <int N, int M>
struct FastStack {
    static constexpr int CAP = N + M;
    uint32_t* r;
    float* k;
    uint32_t* gr;
    float* gk;
    __device__ __forceinline__ uint32_t rec(int i) const { return i < N ? r[i * 256] : gr[i - N]; }
    __device__ __forceinline__ float key(int i) const { return i < N ? k[i * 256] : gk[i - N]; }
    __device__ __forceinline__ void set(int i, uint32_t rv, float kv)
    {
        if (i < N) {
            r[i * 256] = rv;
            k[i * 256] = kv;
        } else {
            gr[i - N] = rv;
            gk[i - N] = kv;
        }
    }
};

__global__ __launch_bounds__(256) void k_intersect(RtSceneView S, const float* __restrict__ rays, int32_t* __restrict__ out,
                                                   int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rtk::StackEnt stack[RT_STACK_CAP];
    const float* r = rays + 6 * (size_t)i;
    const rtk::V3 o = rtk::v3(r[0], r[1], r[2]), d = rtk::v3(r[3], r[4], r[5]);
    float t;
    int k;
    rtk::query_closest(S, o, d, stack, t, k, nullptr);
    rtk::Hit h;
    const bool f = rtk::hit_from(S, o, d, t, k, h);
    int32_t* ot = out + 11 * (size_t)i;
    ot[0] = f ? 1 : 0;
    ot[1] = h.prim;
    ot[2] = (int32_t)rt_asuint(t);
    const bool any = t != -1.0f;
    ot[3] = any ? (int32_t)rt_asuint(h.p.x) : 0;
    ot[4] = any ? (int32_t)rt_asuint(h.p.y) : 0;
    ot[5] = any ? (int32_t)rt_asuint(h.p.z) : 0;
    ot[6] = any ? (int32_t)rt_asuint(h.n.x) : 0;
    ot[7] = any ? (int32_t)rt_asuint(h.n.y) : 0;
    ot[8] = any ? (int32_t)rt_asuint(h.n.z) : 0;
    ot[9] = (int32_t)rt_asuint(-1.0f);
    ot[10] = (int32_t)rt_asuint(-1.0f);
}

// Search-BVH query micro-benchmark (tools/query_bench.py): one query per
// lane, the k_trace stack layout. out_t = t (closest) or 0/1 (any), -2 when
// the query needs the exact walk.
template <bool ANY, int WALK>
__global__ __launch_bounds__(256, 4) void k_query(RtSceneView S, const float4_* __restrict__ rays,
                                                  float* __restrict__ out_t, int* __restrict__ out_k, int n,
                                                  uint32_t* spill_r, float* spill_k)
{
    __shared__ uint32_t s_lds[2 * RT_LDS_CAP_FAST * 256];
    const size_t gl = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    FastStack<RT_LDS_CAP_FAST, RT_SPILL_FAST> stk{s_lds + threadIdx.x, (float*)s_lds + RT_LDS_CAP_FAST * 256 + threadIdx.x,
                                                  spill_r + gl * RT_SPILL_FAST, spill_k + gl * RT_SPILL_FAST};
    const int stride = (int)(gridDim.x * blockDim.x);
    for (int i = (int)gl; i < n; i += stride) {
        const rtk::V3 o = rtk::v3of(rays[2 * i]), d = rtk::v3of(rays[2 * i + 1]);
        if (ANY) {
            const int a = rtk::fast_query_any<decltype(stk), WALK>(S, o, d, stk, nullptr);
            out_t[i] = a < 0 ? -2.0f : (float)a;
            out_k[i] = 0;
        } else {
            float t = 0;
            int k = 0;
            const bool ok = rtk::fast_query_closest<decltype(stk), WALK>(S, o, d, stk, t, k, nullptr);
            out_t[i] = ok ? t : -2.0f;
            out_k[i] = ok ? (k >= 0 ? (int)rt_asuint(S.tri4[3 * (size_t)k].w) : -1) : -2;  // (the original triangle index)
        }
    }
}

// The same through the product's quad walks (rt_quad.h quad_visit, k_trace's per-trip
// code and answer): four lanes per query.
template <bool ANY, int OCC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(OCC, 8))) void k_query_quad(RtSceneView S, const float4_* __restrict__ rays,
                                                    float* __restrict__ out_t, int* __restrict__ out_k, int n)
{
    __shared__ uint32_t s_lds[2 * RT_QSTACK * 64];
    const int q = (int)(threadIdx.x >> 2), sub = (int)(threadIdx.x & 3);
    rtk::QuadStack<RT_QSTACK, 64> stk{s_lds + q, (float*)s_lds + RT_QSTACK * 64 + q};
    const int stride = (int)(gridDim.x * blockDim.x) >> 2;
    for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 2); i < n; i += stride) {
        rtk::QState qs;
        int res = 1;
        if (rtk::far_origin(S, rtk::v3of(rays[2 * i])))
            res = -1;  // (the exact walk's)
        else if (rtk::qstate_begin<ANY>(qs, rtk::v3of(rays[2 * i]), rtk::v3of(rays[2 * i + 1]), sub, nullptr))
            do {
                res = rtk::quad_visit<ANY>(S, qs, stk, sub, nullptr);
            } while (res == 0);
        float t = -1.0f;
        int k = -1;
        const bool ok = res > 0 && (ANY || rtk::quad_closest_answer(S, qs, sub, t, k, nullptr));
        if (sub == 0) {
            if (ANY) {
                out_t[i] = ok ? (float)(qs.h.k == 1 ? 1 : 0) : -2.0f;
                out_k[i] = 0;
            } else {
                out_t[i] = ok ? t : -2.0f;
                out_k[i] = ok ? (k >= 0 ? (int)rt_asuint(S.tri4[3 * (size_t)k].w) : -1) : -2;  // (the original triangle index)
            }
        }
    }
}

// The quad walks' visit counts per query (rt_device_query_trips; tests pin them: the same nodes in the same
// order take the same counts): out[3 i] = quad_visit calls, out[3 i + 1] = child boxes of the inner trips
// (4 per node), out[3 i + 2] = triangles of the leaf visits. A far origin (no walk) leaves zeros.
template <bool ANY>
__global__ __launch_bounds__(256) void k_query_quad_trips(RtSceneView S, const float4_* __restrict__ rays, int* __restrict__ out, int n)
{
    __shared__ uint32_t s_lds[2 * RT_QSTACK * 64];
    const int q = (int)(threadIdx.x >> 2), sub = (int)(threadIdx.x & 3);
    rtk::QuadStack<RT_QSTACK, 64> stk{s_lds + q, (float*)s_lds + RT_QSTACK * 64 + q};
    const int stride = (int)(gridDim.x * blockDim.x) >> 2;
    for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 2); i < n; i += stride) {
        rtk::QState qs;
        rtk::Stats st;
        for (int j = 0; j < RT_STAT_COUNT; j++) st.c[j] = 0;
        int calls = 0, res = 1;
        if (!rtk::far_origin(S, rtk::v3of(rays[2 * i])) &&
            rtk::qstate_begin<ANY>(qs, rtk::v3of(rays[2 * i]), rtk::v3of(rays[2 * i + 1]), sub, &st))
            do {
                res = rtk::quad_visit<ANY>(S, qs, stk, sub, &st);
                calls++;
            } while (res == 0);
        if (sub == 0) {
            out[3 * i] = calls;
            out[3 * i + 1] = (int)st.c[ANY ? RT_STAT_ANY_VOL : RT_STAT_VOL];
            out[3 * i + 2] = (int)st.c[ANY ? RT_STAT_ANY_TRI : RT_STAT_TRI];
        }
    }
}

// The same through the row walks (rt_row.h row_visit over the 16-wide BVH): 16 lanes per query.
template <bool ANY>
__global__ __launch_bounds__(256) void k_query_row(RtSceneView S, const float4_* __restrict__ rays,
                                                   float* __restrict__ out_t, int* __restrict__ out_k, int n)
{
    __shared__ uint32_t s_lds[2 * RT_RSTACK * 16];
    const int r = (int)(threadIdx.x >> 4), sub = (int)(threadIdx.x & 15);
    rtk::QuadStack<RT_RSTACK, 16> stk{s_lds + r, (float*)s_lds + RT_RSTACK * 16 + r};
    const int stride = (int)(gridDim.x * blockDim.x) >> 4;
    for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 4); i < n; i += stride) {
        rtk::QState qs;
        int res = 1;
        if (rtk::far_origin(S, rtk::v3of(rays[2 * i])))
            res = -1;  // (the exact walk's)
        else if (rtk::qstate_begin<ANY>(qs, rtk::v3of(rays[2 * i]), rtk::v3of(rays[2 * i + 1]), sub, nullptr))
            do {
                res = rtk::row_visit<ANY, RT_VISIT_DESCEND>(S, qs, stk, sub, nullptr);
            } while (res == 0);
        float t = -1.0f;
        int k = -1;
        const bool ok = res > 0 && (ANY || rtk::quad_closest_answer(S, qs, sub & 3, t, k, nullptr));
        if (sub == 0) {
            if (ANY) {
                out_t[i] = ok ? (float)(qs.h.k == 1 ? 1 : 0) : -2.0f;
                out_k[i] = 0;
            } else {
                out_t[i] = ok ? t : -2.0f;
                out_k[i] = ok ? (k >= 0 ? (int)rt_asuint(S.tri4[3 * (size_t)k].w) : -1) : -2;  // (the original triangle index)
            }
        }
    }
}

// numerics self-test kernel (tests/test_gpu_parity.py): out[i] = f(in[i])
__global__ void k_libm(int fn, const float* __restrict__ in, const float* __restrict__ in2, float* __restrict__ out, int n)
{
    rtlibm::lds_tables_init();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in[i];
    float r;
    switch (fn) {
        case 0: r = rt_expf(x); break;
        case 1: r = rt_powf(x, in2[i]); break;
        case 2: r = rt_sinf(x); break;
        case 3: r = rt_cosf(x); break;
        case 4: r = rt_acosf(x); break;
        case 5: r = rt_asinf(x); break;
        case 6: r = rt_atan2f(x, in2[i]); break;
        case 7: r = rt_sqrtf(x); break;
        case 8: r = x / in2[i]; break;
        case 9: r = (float)((double)x * 0.31830988618379067154 / (double)in2[i]); break;
        case 11: {  // rt_sincosf's sine
            float c;
            rt_sincosf(x, r, c);
            break;
        }
        case 12: {  // rt_sincosf's cosine
            float s;
            rt_sincosf(x, s, r);
            break;
        }
        case 13: r = rt_atan2f(x, 1.0f); break;  // atanf
        default: r = rtk::slab_div(x, 1.0 / (double)in2[i]); break;  // the slab quotient
    }
    out[i] = r;
}

// Digest of a whole sweep of rt_libm.h (rt_digest.h; tests/test_gpu_libm.py): RT_DIGEST_SPLIT workgroups
// per digest block of 2^22 indices, each over its own 2^19 consecutive indices. A thread sums the terms
// of its indices (every stride-th, 256 stride apart: a wave's lanes take neighbouring arguments, so they
// mostly take one branch) in a register; the workgroup's total goes to partial[blockIdx.x], and the host
// adds the partials of a block.
#define RT_DIGEST_SPLIT 8
template <int FN>
__global__ __launch_bounds__(256) void k_libm_digest(uint32_t param, uint32_t stride, uint64_t* __restrict__ partial)
{
    __shared__ uint64_t s_sum[256];
    rtlibm::lds_tables_init();
    const float p = rt_asfloat(param);
    const uint32_t span = (1u << rtdigest::BLOCK_BITS) / RT_DIGEST_SPLIT;
    const uint32_t base = blockIdx.x * span;  // (gridDim.x = 1024 * RT_DIGEST_SPLIT: below 2^32)
    uint64_t sum = 0;
    for (uint32_t k = threadIdx.x * stride; k < span; k += 256 * stride) {
        const uint32_t i = base + k;
        sum += rtdigest::term(i, rtdigest::eval<FN>(i, p));
    }
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) s_sum[threadIdx.x] += s_sum[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s_sum[0];
}

// TEST ONLY (rt_device_env_search): cdf_search alone over caller values. form 0: as the shading
// kernels run it, after lds_shade_init's staging; form 1: every table from global memory.
__global__ void k_env_search(RtSceneView S, int form, const float* __restrict__ values, int n, int* __restrict__ xy)
{
    if (form == 0) rtk::lds_shade_init(S);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int x, y;
        if (form == 0)
            rtk::cdf_search(S, values[i], x, y, nullptr);
        else
            rtk::cdf_search_global(S, values[i], x, y);
        xy[2 * i] = x;
        xy[2 * i + 1] = y;
    }
}

}  // namespace

int rt_backend_intersect(rt_context* c, const float* rays, int n, void* out)
{
    Backend* b = rt_backend_dev0(c);
    HIPCHK(c, hipSetDevice(b->device));
    const size_t br = (size_t)n * 24, bo = (size_t)n * 44;
    if (int r = ensure(c, b->xy, br + bo)) return r;
    float* dr = (float*)b->xy.p;
    int32_t* dout = (int32_t*)((char*)b->xy.p + br);
    HIPCHK(c, hipMemcpy(dr, rays, br, hipMemcpyHostToDevice));
    const int threads = 256, blocks = (n + threads - 1) / threads;
    HIPCHK(c, hipEventRecord(b->ev0, 0));
    hipLaunchKernelGGL(k_intersect, dim3(blocks), dim3(threads), 0, 0, b->view, dr, dout, n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(b->ev1, 0));
    HIPCHK(c, hipEventSynchronize(b->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, b->ev0, b->ev1));
    c->last_kernel_ms = ms;
    HIPCHK(c, hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost));
    return RT_OK;
}

// Device self-tests of the numerics (libm restatement, IEEE div/sqrt/f64).
extern "C" int rt_device_libm(int device, int fn, const float* in, const float* in2, float* out, int n)
{
    if (hipSetDevice(device) != hipSuccess) return RT_ERR_NODEV;
    const size_t b = (size_t)n * 4;
    DevBuf d_in, d_in2, d_out;
    if (ensure(nullptr, d_in, b) || ensure(nullptr, d_in2, b) || ensure(nullptr, d_out, b)) return RT_ERR_HIP;
    (void)hipMemcpy(d_in.p, in, b, hipMemcpyHostToDevice);
    if (in2) (void)hipMemcpy(d_in2.p, in2, b, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_libm, dim3((n + 255) / 256), dim3(256), 0, 0, fn, (const float*)d_in.p, (const float*)d_in2.p,
                       (float*)d_out.p, n);
    return hipMemcpy(out, d_out.p, b, hipMemcpyDeviceToHost) == hipSuccess ? RT_OK : RT_ERR_HIP;
}

// TEST ONLY, like rt_device_libm (gfx950 library only, not in include/rt_hip.h): the digest words
// out[1024] of one sweep of rt_libm.h on the device (rt_digest.h): sweep = the function code
// (rtdigest::Fn), param = the fixed argument's bits, stride = a power of two, every stride-th index summed.
extern "C" int rt_device_libm_digest(int device, int sweep, uint32_t param, int stride, uint64_t* out)
{
    if (!out || sweep < 0 || sweep >= rtdigest::FN_COUNT || stride < 1 || stride > 256 || (stride & (stride - 1))) return RT_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return RT_ERR_NODEV;
    const int groups = rtdigest::BLOCKS * RT_DIGEST_SPLIT;
    DevBuf d_part;
    if (ensure(nullptr, d_part, (size_t)groups * 8)) return RT_ERR_HIP;
    uint64_t* part = (uint64_t*)d_part.p;
#define RT_DIGEST_CASE(FN) \
    case FN: hipLaunchKernelGGL((k_libm_digest<FN>), dim3(groups), dim3(256), 0, 0, param, (uint32_t)stride, part); break;
    switch (sweep) {
        RT_DIGEST_CASE(0) RT_DIGEST_CASE(1) RT_DIGEST_CASE(2) RT_DIGEST_CASE(3) RT_DIGEST_CASE(4) RT_DIGEST_CASE(5)
        RT_DIGEST_CASE(6) RT_DIGEST_CASE(7) RT_DIGEST_CASE(8) RT_DIGEST_CASE(9) RT_DIGEST_CASE(10) RT_DIGEST_CASE(11)
    }
#undef RT_DIGEST_CASE
    if (hipGetLastError() != hipSuccess) return RT_ERR_HIP;
    std::vector<uint64_t> h((size_t)groups);
    if (hipMemcpy(h.data(), part, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return RT_ERR_HIP;
    for (int b = 0; b < rtdigest::BLOCKS; b++) {
        uint64_t s = 0;
        for (int k = 0; k < RT_DIGEST_SPLIT; k++) s += h[(size_t)b * RT_DIGEST_SPLIT + k];
        out[b] = s;
    }
    return RT_OK;
}

// TEST ONLY (include/rt_hip.h): the env-CDF search alone on the context's env, several blocks
// (each stages its own LDS copy in form 0).
extern "C" int rt_device_env_search(rt_context* c, int form, const float* values, int n, int* xy_out)
{
    if (!c || !c->backend || n <= 0 || !values || !xy_out || form < 0 || form > 1) return RT_ERR_ARG;
    if (!c->have_env) return RT_ERR_STATE;
    Backend* b = rt_backend_dev0(c);
    HIPCHK(c, hipSetDevice(b->device));
    if (c->dirty) {
        if (int r = rt_backend_upload(c)) return r;
        c->dirty = false;
    }
    DevBuf v, xy;
    if (int r = ensure(c, v, (size_t)n * 4)) return r;
    if (int r = ensure(c, xy, (size_t)n * 8)) return r;
    HIPCHK(c, hipMemcpy(v.p, values, (size_t)n * 4, hipMemcpyHostToDevice));
    const int threads = 256, blocks = std::min((n + threads - 1) / threads, 64);
    hipLaunchKernelGGL(k_env_search, dim3(blocks), dim3(threads), 0, 0, b->view, form, (const float*)v.p, n, (int*)xy.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy(xy_out, xy.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}

// Search-BVH query micro-benchmark: rays[n][8] (origin xyz _, direction xyz _),
// mode bit 0 = any (else closest), bits 1.. = walk variant (0-1 one lane, 2-3 lane + spill,
// 4-5 quads, 6-7 quads at 8 waves/SIMD, 8-9 rows);
// reps timed launches (HIP events), mean ms per launch into *ms.
extern "C" int rt_device_queries(rt_context* c, int mode, const float* rays, int n, int reps, float* out_t,
                                 int* out_k, double* ms)
{
    if (!c || !c->backend || n <= 0 || reps < 1 || mode < 0 || mode > 9) return RT_ERR_ARG;
    Backend* b = rt_backend_dev0(c);
    HIPCHK(c, hipSetDevice(b->device));
    if (c->dirty) {
        if (int r = rt_backend_upload(c)) return r;
        c->dirty = false;
    }
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device);
    const int threads = 256, blocks = std::min((n + threads - 1) / threads, cus * 8);
    const int qblocks = std::min((4 * n + threads - 1) / threads, cus * 16);
    const int rblocks = std::min((16 * n + threads - 1) / threads, cus * 16);
    const size_t lanes = (size_t)blocks * threads;
    DevBuf b_rays, b_t, b_k, b_sr, b_sk;
    if (int r = ensure(c, b_rays, (size_t)n * 32)) return r;
    if (int r = ensure(c, b_t, (size_t)n * 4)) return r;
    if (int r = ensure(c, b_k, (size_t)n * 4)) return r;
    if (int r = ensure(c, b_sr, lanes * RT_SPILL_FAST * 4)) return r;
    if (int r = ensure(c, b_sk, lanes * RT_SPILL_FAST * 4)) return r;
    float4_* d_rays = (float4_*)b_rays.p;
    float* d_t = (float*)b_t.p;
    int* d_k = (int*)b_k.p;
    uint32_t* sr = (uint32_t*)b_sr.p;
    float* sk = (float*)b_sk.p;
    HIPCHK(c, hipMemcpy(d_rays, rays, (size_t)n * 32, hipMemcpyHostToDevice));
    auto launch = [&]() {
        switch (mode) {
            case 0: hipLaunchKernelGGL((k_query<false, 0>), dim3(blocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n, sr, sk); break;
            case 1: hipLaunchKernelGGL((k_query<true, 0>), dim3(blocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n, sr, sk); break;
            case 2: hipLaunchKernelGGL((k_query<false, 1>), dim3(blocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n, sr, sk); break;
            case 3: hipLaunchKernelGGL((k_query<true, 1>), dim3(blocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n, sr, sk); break;
            case 4: hipLaunchKernelGGL((k_query_quad<false, 1>), dim3(qblocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n); break;
            case 5: hipLaunchKernelGGL((k_query_quad<true, 1>), dim3(qblocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n); break;
            case 6: hipLaunchKernelGGL((k_query_quad<false, 8>), dim3(qblocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n); break;
            case 7: hipLaunchKernelGGL((k_query_quad<true, 8>), dim3(qblocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n); break;
            case 8: hipLaunchKernelGGL((k_query_row<false>), dim3(rblocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n); break;
            default: hipLaunchKernelGGL((k_query_row<true>), dim3(rblocks), dim3(threads), 0, 0, b->view, d_rays, d_t, d_k, n); break;
        }
    };
    launch();  // warm-up
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(b->ev0, 0));
    for (int r = 0; r < reps; r++) launch();
    HIPCHK(c, hipEventRecord(b->ev1, 0));
    HIPCHK(c, hipEventSynchronize(b->ev1));
    float t = 0;
    HIPCHK(c, hipEventElapsedTime(&t, b->ev0, b->ev1));
    if (ms) *ms = t / reps;
    HIPCHK(c, hipMemcpy(out_t, d_t, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_k, d_k, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

// TEST ONLY. The quad walks' visit counts (k_query_quad_trips): rays[n][8] as rt_device_queries, any = 0 the
// closest-hit walk, 1 the occlusion walk; out[n][3] = quad_visit calls, child boxes, leaf triangles.
extern "C" int rt_device_query_trips(rt_context* c, int any, const float* rays, int n, int* out)
{
    if (!c || !c->backend || n <= 0 || !rays || !out || (any != 0 && any != 1)) return RT_ERR_ARG;
    Backend* b = rt_backend_dev0(c);
    HIPCHK(c, hipSetDevice(b->device));
    if (c->dirty) {
        if (int r = rt_backend_upload(c)) return r;
        c->dirty = false;
    }
    const int threads = 256, qblocks = std::min((4 * n + threads - 1) / threads, 4096);
    DevBuf b_rays, b_out;
    if (int r = ensure(c, b_rays, (size_t)n * 32)) return r;
    if (int r = ensure(c, b_out, (size_t)n * 12)) return r;
    HIPCHK(c, hipMemcpy(b_rays.p, rays, (size_t)n * 32, hipMemcpyHostToDevice));
    if (any)
        hipLaunchKernelGGL((k_query_quad_trips<true>), dim3(qblocks), dim3(threads), 0, 0, b->view, (const float4_*)b_rays.p, (int*)b_out.p, n);
    else
        hipLaunchKernelGGL((k_query_quad_trips<false>), dim3(qblocks), dim3(threads), 0, 0, b->view, (const float4_*)b_rays.p, (int*)b_out.p, n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, b_out.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    return RT_OK;
}
