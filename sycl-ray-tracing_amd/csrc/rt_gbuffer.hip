// rt_gbuffer.hip — gfx950 kernels and launches of the first-hit G-buffer on the render's walks
// (rt_gbuffer.h; include/rt_hip.h rt_render_gbuffer / rt_render_gbuffer_device). Its own
// translation unit, so that the render kernels of rt_render.hip compile exactly as they do without
// it; the device functions are the render's (rt_quad.h quad_visit / quad_closest_answer, rt_fast.h
// far_origin, rt_octet.h octg_setup / octc_node, rt_wave.h query_closest / hit_from).
//
//   k_gb_fast<REFILL>  k_rq_fast<false, REFILL>'s shape (rt_query.hip) without a ray buffer: four
//                  lanes (a quad) per pixel over the search BVH4, the quad's stack in LDS (QuadStack,
//                  16 KB per block of 64 quads); the quad computes feature_ray from the pixel index.
//                  Lane 0 of a quad whose walk settles writes the pixel's records; a pixel routed away
//                  (far_origin, the gb_force_every stressor) or left unsettled has its index appended
//                  to the fallback list: one ballot and one atomic per wave. REFILL = false: the wave
//                  takes 16 consecutive pixels per round. REFILL = true: the wave reads its stream
//                  through a cursor and refills once GB_REFILL quads are idle.
//   k_gb_exact_oct eight lanes (an octet, rt_octet.h) per entry of the fallback list (its length read
//                  from device memory, so the stream form needs no host round trip), or per pixel when
//                  every pixel takes the exact walk (list == nullptr): octg_setup, then octc_node until
//                  TM_DONE, no parking. The OctRing in LDS (16 KB per block of 32 octets), the spill
//                  areas in the context's workspace, one per octet of the launched grid. Octets take
//                  tickets with one atomic per wave, as k_step's exact role does.
//   k_gb_exact_lane one lane per pixel over query_closest, k_features' code path: contexts with
//                  spheres or in rt_set_intersect_mode(0) have no octree answer to share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "rt_backend_hip.h"
#include "rt_gbuffer.h"
#include "rt_octet.h"
#include "rt_quad.h"

#define GB_QSTACK 32  // stack entries per quad (item + key), k_trace's RT_QSTACK
#define GB_REFILL 4   // idle quads of a wave that trigger a refill, k_trace's RT_TRACE_REFILL
#define GB_OCT_REFILL 2  // idle octets of a wave that trigger a refill (k_step's RT_REFILL / 8)

namespace {

struct alignas(8) GbIds {
    int32_t prim, mat;
};

// The outputs of a call: two float4 per pixel and, where asked for, the int32 pair.
struct GbOut {
    float4_* __restrict__ alb;
    float4_* __restrict__ nd;
    GbIds* __restrict__ ids;
};

// Pixel i's records from a walk's answer: two 16-byte stores and the optional 8-byte one.
__device__ __forceinline__ void gb_write(const RtSceneView& S, rtk::V3 o, rtk::V3 d, float t, int k, const GbOut& O, int i)
{
    const rtk::GbRecord r = rtk::gb_record(S, o, d, t, k);
    O.nd[i] = r.nd;
    O.alb[i] = r.alb;
    if (O.ids) O.ids[i] = GbIds{r.prim, r.mat};
}

// Grid: whole waves; n > 0. fb_list has room for n indices, *fb_count starts at 0.
template <bool REFILL>
__global__ __launch_bounds__(256) void k_gb_fast(RtSceneView S, rtk::CamView V, GbOut O, int n, int force_every,
                                                 int32_t* __restrict__ fb_list, int32_t* __restrict__ fb_count)
{
    __shared__ uint32_t s_lds[2 * GB_QSTACK * 64];
    const int bq = (int)(threadIdx.x >> 2);  // the quad in its block
    rtk::QuadStack<GB_QSTACK, 64> stk{s_lds + bq, (float*)s_lds + GB_QSTACK * 64 + bq};
    const int lane = (int)__lane_id(), qd = lane >> 2, sub = lane & 3;
    const int wg = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);  // this wave in the grid
    const int wn = (int)((gridDim.x * blockDim.x) >> 6);                 // the grid's waves
    rtk::QState q;
    if (!REFILL) {
        // round r: pixels (wg + r wn) 16 .. + 15, one per quad (the bound is wave-uniform)
        for (int base = wg * 16; base < n; base += wn * 16) {
            const int i = base + qd;
            bool settled = false;
            float t = -1.0f;
            int k = -1;
            if (i < n) {
                rtk::V3 o, d;
                rtk::gb_ray(V, i, o, d);
                if (!rtk::gb_forced(force_every, i) && !rtk::far_origin(S, o)) {
                    int res = 1;
                    if (rtk::qstate_begin<false>(q, o, d, sub, nullptr))
                        do {
                            res = rtk::quad_visit<false>(S, q, stk, sub, nullptr);
                        } while (res == 0);
                    settled = res > 0 && rtk::quad_closest_answer(S, q, sub, t, k, nullptr);
                    if (settled && sub == 0) gb_write(S, q.o, q.d, t, k, O, i);
                }
            }
            const int slot = wave_append(fb_count, i < n && !settled && sub == 0);
            if (slot >= 0) fb_list[slot] = i;
        }
        return;
    }
    // The wave's stream: position j is pixel (wg + (j >> 4) wn) 16 + (j & 15).
    constexpr unsigned long long ALL_IDLE = 0x1111111111111111ull;
    int cursor = 0;                 // the wave's next stream position (uniform)
    bool exhausted = wg * 16 >= n;  // (uniform)
    bool active = false;
    int idx = -1;      // the quad's pixel
    int pending = -1;  // a pixel of the quad's that waits for its place in the fallback list
    for (;;) {
        {  // (the wave is converged here: the fallback entries of the last trip, one atomic)
            const int slot = wave_append(fb_count, pending >= 0 && sub == 0);
            if (slot >= 0) fb_list[slot] = pending;
            pending = -1;
        }
        const unsigned long long bidle = __ballot(!active && sub == 0);
        if (!exhausted && (__popcll(bidle) >= GB_REFILL || bidle == ALL_IDLE)) {
            if (!active) {
                const int j = cursor + __popcll(bidle & ((1ull << (qd * 4)) - 1ull));  // this quad's stream position
                idx = (wg + (j >> 4) * wn) * 16 + (j & 15);
                if (idx < n) {
                    rtk::V3 o, d;
                    rtk::gb_ray(V, idx, o, d);
                    if (rtk::gb_forced(force_every, idx) || rtk::far_origin(S, o)) {
                        pending = idx;
                    } else if (rtk::qstate_begin<false>(q, o, d, sub, nullptr)) {
                        active = true;
                    } else if (sub == 0) {  // (a NaN ray: no hit)
                        gb_write(S, q.o, q.d, -1.0f, -1, O, idx);
                    }
                }
            }
            cursor += __popcll(bidle);
            exhausted = (wg + (cursor >> 4) * wn) * 16 >= n;
        }
        const unsigned long long bact = __ballot(active && sub == 0);
        if (!bact) {
            if (exhausted) break;
            continue;
        }
        if (active) {
            const int res = rtk::quad_visit<false>(S, q, stk, sub, nullptr);
            if (res != 0) {
                active = false;
                float t = -1.0f;
                int k = -1;
                if (res > 0 && rtk::quad_closest_answer(S, q, sub, t, k, nullptr)) {
                    if (sub == 0) gb_write(S, q.o, q.d, t, k, O, idx);
                } else {
                    pending = idx;
                }
            }
        }
    }
    // (pixels routed away by the last refill)
    const int slot = wave_append(fb_count, pending >= 0 && sub == 0);
    if (slot >= 0) fb_list[slot] = pending;
}

// The exact octree walk, eight lanes per walk, for the entries of list (their number at *count), or,
// list == nullptr, for every pixel 0..n-1. *ticket starts at 0; spill_r / spill_k hold RT_STACK_CAP
// entries per octet of the grid. Octree contexts without spheres only (k_gb_exact_lane otherwise).
__global__ __launch_bounds__(256) void k_gb_exact_oct(RtSceneView S, rtk::CamView V, GbOut O, int n,
                                                      const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                      int32_t* __restrict__ ticket, uint32_t* __restrict__ spill_r,
                                                      float* __restrict__ spill_k)
{
    __shared__ uint32_t s_lds[4 * RT_OCT_CAP * 32];
    const int total = list ? min(*count, n) : n;
    if (total <= 0) return;  // (the usual frame: no walk was left unsettled)
    rtk::OctRing w = rtk::oct_ring(s_lds);
    const int lane = (int)__lane_id(), sub = lane & 7;
    const size_t oct = (size_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 3);  // this octet in the grid
    uint32_t* spr = spill_r + oct * RT_STACK_CAP;
    float* spk = spill_k + oct * RT_STACK_CAP;
    rtk::TravG T;
    bool has = false, drained = false;  // (has: octet-uniform; drained: wave-uniform)
    int pix = -1;
    for (;;) {
        const unsigned long long bneed = __ballot(!has && sub == 0);
        const int nneed = __popcll(bneed);
        if (!drained && (nneed >= GB_OCT_REFILL || nneed == 8)) {
            int base = 0;
            if (lane == 0) base = atomicAdd(ticket, nneed);
            base = __shfl(base, 0);
            if (base + nneed >= total) drained = true;
            if (!has) {
                const int e = base + __popcll(bneed & ((1ull << rtk::oct_lane0()) - 1ull));
                pix = e < total ? (list ? list[e] : e) : -1;
                if (pix >= 0 && pix < n) {  // (always below n: the list holds pixel indices)
                    rtk::V3 o, d;
                    rtk::gb_ray(V, pix, o, d);
                    has = rtk::octg_setup(S, T, o, d, nullptr, false, sub);
                    if (!has && sub == 0) gb_write(S, T.o, T.d, T.best_t, T.best_k, O, pix);
                }
            }
        }
        if (!__any(has)) {
            if (drained) break;
            continue;
        }
        if (has) {
            rtk::octc_node(S, T, w, spr, spk, sub, nullptr);
            if (T.mode == rtk::TM_DONE) {
                if (sub == 0) gb_write(S, T.o, T.d, T.best_t, T.best_k, O, pix);
                has = false;
            }
        }
    }
}

// One lane per pixel over query_closest (the octree walk or the brute-force loop, then the sphere
// loop): k_features' code path with the ids. Grid-stride.
__global__ __launch_bounds__(256) void k_gb_exact_lane(RtSceneView S, rtk::CamView V, GbOut O, int n)
{
    const int stride = (int)(gridDim.x * blockDim.x);
    rtk::StackEnt stack[RT_STACK_CAP];
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += stride) {
        rtk::V3 o, d;
        rtk::gb_ray(V, i, o, d);
        float t;
        int k;
        rtk::query_closest(S, o, d, stack, t, k, nullptr);
        gb_write(S, o, d, t, k, O, i);
    }
}

// gb_variant (rt_test_schedule): 1 the plain rounds, 2 the per-quad refill, 0 the product's choice:
// the refill, rt_query's choice for its closest-hit kernel (profiles/gbuffer_bench.json).
bool use_refill(int variant) { return variant != 1; }

}  // namespace

// The stage's workspace on the root device, cached across calls and grown on demand.
struct Gbuf {
    DevBuf list;   // 64 B (word 0 the fallback count, word 1 the octets' ticket), then n pixel indices
    DevBuf io;     // host-pointer calls: the three outputs
    DevBuf spill;  // the octets' spill areas: RT_STACK_CAP refs per octet of the grid, then as many keys
    Event done;    // the end of the last call's kernels (rt_gbuffer_last_exact waits for it)
    int blocks[3] = {0, 0, 0};  // resident blocks per CU of k_gb_fast<false>, k_gb_fast<true>, k_gb_exact_oct, asked once
    int cus = 0;
};

void GbufDelete::operator()(Gbuf* g) const { delete g; }

// (created on first use; b's device is current)
static int gbuf_of(rt_context* c, Backend* b, Gbuf** out)
{
    if (!b->gbuf) {
        Gbuf* g = new Gbuf();
        b->gbuf.reset(g);
        HIPCHK(c, hipEventCreate(&g->done.h));
        HIPCHK(c, hipDeviceGetAttribute(&g->cus, hipDeviceAttributeMultiprocessorCount, b->device));
        const void* fn[3] = {(const void*)k_gb_fast<false>, (const void*)k_gb_fast<true>, (const void*)k_gb_exact_oct};
        for (int i = 0; i < 3; i++) {
            HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&g->blocks[i], fn[i], 256, 0));
            g->blocks[i] = std::max(1, std::min(8, g->blocks[i]));
        }
    }
    *out = b->gbuf.get();
    return RT_OK;
}

int rt_backend_gbuffer(rt_context* c, int w, int h, bool all_exact, void* albedo, void* normal_depth, void* ids,
                       bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    Gbuf* G = nullptr;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    if (int r = gbuf_of(c, b, &G)) return r;
    hipStream_t s = st.s;
    const size_t n = (size_t)w * h, rec_bytes = n * sizeof(float4_), id_bytes = n * sizeof(GbIds);
    if (int r = st.staging(G->io, 2 * rec_bytes + st.pad(id_bytes))) return r;
    GbOut O;
    O.alb = (float4_*)st.out(albedo, rec_bytes);
    O.nd = (float4_*)st.out(normal_depth, rec_bytes);
    O.ids = (GbIds*)st.out(ids, id_bytes);  // (NULL: no ids)
    const rtk::CamView V = rtk::cam_view(c->cam, w, h);
    const int ni = (int)n;  // (n < 2^27, rt_capi_stages.cpp)
    // Every pixel's origin is the camera's: a far camera is seen here, and the frame takes the NULL-list form.
    const bool one_lane = c->brute || !c->spheres.empty();
    const bool far = rtk::far_origin(b->view, rtk::v3(V.cam_o[0], V.cam_o[1], V.cam_o[2]));
    const bool routed = !all_exact && !one_lane && !far;
    c->gbuffer_on_device = routed;
    c->gbuffer_exact = (long)n;
    if (int r = ensure(c, G->list, 64 + (routed ? n * 4 : 0))) return r;
    // the octets' grid: 32 per block; a routed frame's list is short (~1e-6 of the pixels), one block per CU
    const unsigned oct_blocks =
        std::min((unsigned)((n + 31) / 32), (unsigned)G->cus * (routed ? 1u : (unsigned)G->blocks[2]));
    const size_t spill_ents = (size_t)oct_blocks * 32 * RT_STACK_CAP;
    if (!one_lane)
        if (int r = ensure(c, G->spill, spill_ents * 8)) return r;
    int32_t* count = (int32_t*)G->list.p;
    int32_t* ticket = count + 1;
    int32_t* list = count + 16;
    uint32_t* spill_r = (uint32_t*)G->spill.p;
    float* spill_k = (float*)G->spill.p + spill_ents;
    if (int r = st.begin()) return r;
    if (one_lane) {
        const unsigned blocks = std::min((unsigned)((n + 255) / 256), (unsigned)G->cus * 8u);
        hipLaunchKernelGGL(k_gb_exact_lane, dim3(blocks), dim3(256), 0, s, b->view, V, O, ni);
        HIPCHK(c, hipGetLastError());
    } else {
        HIPCHK(c, hipMemsetAsync(count, 0, 8, s));
        if (routed) {
            const bool refill = use_refill(c->sched.variant[RT_VAR_GB]);
            // whole waves of 16 pixels; at most what is resident at once (the rest by stride)
            const unsigned resident = (unsigned)(G->cus * G->blocks[refill ? 1 : 0]);
            const unsigned fast_blocks = std::min((unsigned)((n + 63) / 64), resident);
            if (refill)
                hipLaunchKernelGGL((k_gb_fast<true>), dim3(fast_blocks), dim3(256), 0, s, b->view, V, O, ni,
                                   c->sched.gb_force_every, list, count);
            else
                hipLaunchKernelGGL((k_gb_fast<false>), dim3(fast_blocks), dim3(256), 0, s, b->view, V, O, ni,
                                   c->sched.gb_force_every, list, count);
            HIPCHK(c, hipGetLastError());
        }
        hipLaunchKernelGGL(k_gb_exact_oct, dim3(oct_blocks), dim3(256), 0, s, b->view, V, O, ni,
                           routed ? (const int32_t*)list : (const int32_t*)nullptr,
                           routed ? (const int32_t*)count : (const int32_t*)nullptr, ticket, spill_r, spill_k);
        HIPCHK(c, hipGetLastError());
    }
    if (int r = st.stop()) return r;
    HIPCHK(c, hipEventRecord(G->done, s));
    return st.finish();
}

long rt_backend_gbuffer_last_exact(rt_context* c)
{
    Backend* b = rt_backend_dev0(c);
    DeviceScope sc;
    Gbuf* G = nullptr;
    if (int r = sc.enter(c, b->device)) return r;
    if (int r = gbuf_of(c, b, &G)) return r;
    if (!c->gbuffer_on_device) {
        // (every pixel took the exact walk, or no call yet: known on the host; wait all the same)
        if (c->gbuffer_exact > 0) HIPCHK(c, hipEventSynchronize(G->done));
        return c->gbuffer_exact;
    }
    HIPCHK(c, hipEventSynchronize(G->done));
    int32_t v = 0;
    HIPCHK(c, hipMemcpy(&v, G->list.p, 4, hipMemcpyDeviceToHost));
    return v;
}
