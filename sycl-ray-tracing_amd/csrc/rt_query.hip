// rt_query.hip — gfx950 kernels and launches of the batched ray queries (rt_query.h;
// include/rt_hip.h rt_query / rt_query_device). Its own translation unit, so that the render
// kernels of rt_render.hip compile exactly as they do without it; the device functions are
// the render's (rt_quad.h quad_visit / quad_closest_answer, rt_fast.h far_origin,
// rt_wave.h query_closest / hit_from).
//
//   k_rq_fast<ANY, REFILL>  four lanes (a quad) per query over the search BVH4, the quad's
//                  stack in LDS (QuadStack, 16 KB per block of 64 quads). Lane 0 of a quad
//                  whose walk settles writes the answer; a query routed away (far_origin)
//                  or left unsettled (a tie, a failed chain check, a stack overflow) has its
//                  index appended to the fallback list: one ballot and one atomic per wave.
//                  REFILL = false: the wave takes 16 consecutive queries per round, one per
//                  quad, and the round ends with its longest walk. REFILL = true: the wave
//                  reads its stream (the same 16-query chunks, strided by the grid's waves)
//                  through a cursor; once RQ_REFILL quads are idle they take the next
//                  positions while the others walk on (k_trace's quad refill).
//   k_rq_exact     one thread per entry of the fallback list (count read from device memory,
//                  so the stream form needs no host round trip), or per query when every
//                  query takes the exact walk: query_closest + hit_from, k_intersect's code.
// The rays stay in the caller's order; nothing is searched or sorted.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "rt_backend_hip.h"
#include "rt_query.h"
#include "rt_quad.h"

#define RQ_QSTACK 32  // stack entries per quad (item + key), k_trace's RT_QSTACK
#define RQ_REFILL 4   // idle quads of a wave that trigger a refill, k_trace's RT_TRACE_REFILL

namespace {

struct RqRay {
    rtk::V3 o, d;
};
__device__ __forceinline__ RqRay load_ray(const float* __restrict__ rays, int i)
{
    const float* r = rays + 6 * (size_t)i;
    return RqRay{rtk::v3(r[0], r[1], r[2]), rtk::v3(r[3], r[4], r[5])};
}

// A settled walk's answer, written by lane 0 of its quad.
template <bool ANY>
__device__ __forceinline__ void write_answer(const RtSceneView& S, const rtk::QState& q, float t, int k,
                                             int32_t* __restrict__ out, int i)
{
    if (ANY)
        out[i] = q.h.k == 1 ? 1 : 0;
    else
        rtk::rq_closest_record(S, q.o, q.d, t, k, out + RQ_WORDS * (size_t)i);
}

// Grid: whole waves; n > 0. fb_list has room for n indices, *fb_count starts at 0.
template <bool ANY, bool REFILL>
__global__ __launch_bounds__(256) void k_rq_fast(RtSceneView S, const float* __restrict__ rays,
                                                 int32_t* __restrict__ out, int n, int32_t* __restrict__ fb_list,
                                                 int32_t* __restrict__ fb_count)
{
    __shared__ uint32_t s_lds[2 * RQ_QSTACK * 64];
    const int bq = (int)(threadIdx.x >> 2);  // the quad in its block
    rtk::QuadStack<RQ_QSTACK, 64> stk{s_lds + bq, (float*)s_lds + RQ_QSTACK * 64 + bq};
    const int lane = (int)__lane_id(), qd = lane >> 2, sub = lane & 3;
    const int wg = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);  // this wave in the grid
    const int wn = (int)((gridDim.x * blockDim.x) >> 6);                 // the grid's waves
    rtk::QState q;
    if (!REFILL) {
        // round r: queries (wg + r wn) 16 .. + 15, one per quad (the bound is wave-uniform)
        for (int base = wg * 16; base < n; base += wn * 16) {
            const int i = base + qd;
            bool settled = false;
            float t = -1.0f;
            int k = -1;
            if (i < n) {
                const RqRay r = load_ray(rays, i);
                if (!rtk::far_origin(S, r.o)) {
                    int res = 1;
                    if (rtk::qstate_begin<ANY>(q, r.o, r.d, sub, nullptr))
                        do {
                            res = rtk::quad_visit<ANY>(S, q, stk, sub, nullptr);
                        } while (res == 0);
                    settled = res > 0 && (ANY || rtk::quad_closest_answer(S, q, sub, t, k, nullptr));
                    if (settled && sub == 0) write_answer<ANY>(S, q, t, k, out, i);
                }
            }
            const int slot = wave_append(fb_count, i < n && !settled && sub == 0);
            if (slot >= 0) fb_list[slot] = i;
        }
        return;
    }
    // The wave's stream: position j is query (wg + (j >> 4) wn) 16 + (j & 15).
    constexpr unsigned long long ALL_IDLE = 0x1111111111111111ull;
    int cursor = 0;                 // the wave's next stream position (uniform)
    bool exhausted = wg * 16 >= n;  // (uniform)
    bool active = false;
    int idx = -1;      // the quad's query
    int pending = -1;  // a query of the quad's that waits for its place in the fallback list
    for (;;) {
        {  // (the wave is converged here: the fallback entries of the last trip, one atomic)
            const int slot = wave_append(fb_count, pending >= 0 && sub == 0);
            if (slot >= 0) fb_list[slot] = pending;
            pending = -1;
        }
        const unsigned long long bidle = __ballot(!active && sub == 0);
        if (!exhausted && (__popcll(bidle) >= RQ_REFILL || bidle == ALL_IDLE)) {
            if (!active) {
                const int j = cursor + __popcll(bidle & ((1ull << (qd * 4)) - 1ull));  // this quad's stream position
                idx = (wg + (j >> 4) * wn) * 16 + (j & 15);
                if (idx < n) {
                    const RqRay r = load_ray(rays, idx);
                    if (rtk::far_origin(S, r.o)) {
                        pending = idx;
                    } else if (rtk::qstate_begin<ANY>(q, r.o, r.d, sub, nullptr)) {
                        active = true;
                    } else if (sub == 0) {  // (a NaN ray: no hit)
                        write_answer<ANY>(S, q, -1.0f, -1, out, idx);
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
            const int res = rtk::quad_visit<ANY>(S, q, stk, sub, nullptr);
            if (res != 0) {
                active = false;
                float t = -1.0f;
                int k = -1;
                if (res > 0 && (ANY || rtk::quad_closest_answer(S, q, sub, t, k, nullptr))) {
                    if (sub == 0) write_answer<ANY>(S, q, t, k, out, idx);
                } else {
                    pending = idx;
                }
            }
        }
    }
    // (queries routed away by the last refill)
    const int slot = wave_append(fb_count, pending >= 0 && sub == 0);
    if (slot >= 0) fb_list[slot] = pending;
}

// The exact walk for the entries of list (their number at *count), or, list == nullptr, for
// every query 0..n-1. Grid-stride.
__global__ __launch_bounds__(256) void k_rq_exact(RtSceneView S, const float* __restrict__ rays,
                                                  int32_t* __restrict__ out, int n, const int32_t* __restrict__ list,
                                                  const int32_t* __restrict__ count, int any)
{
    const int m = list ? min(*count, n) : n;
    const int stride = (int)(gridDim.x * blockDim.x);
    rtk::StackEnt stack[RT_STACK_CAP];
    for (int e = (int)(blockIdx.x * blockDim.x + threadIdx.x); e < m; e += stride) {
        const int i = list ? list[e] : e;
        if (i < 0 || i >= n) continue;  // (never: the list holds indices below n)
        rtk::rq_exact(S, rays, (size_t)i, any != 0, stack, out);
    }
}

// rq_variant (rt_test_schedule): 1 the plain rounds, 2 the per-quad refill, 0 the product's
// choice: the refill (profiles/query_api_bench.json), plain / refill ms for 2 M
// rays over the cfg2 dragon on the MI355X: bounce rays closest 0.419 / 0.356, any 0.373 / 0.268;
// the same rays shuffled 0.613 / 0.353 and 0.518 / 0.289; 1080p camera rays any 0.118 / 0.124
// (the one set where plain wins) and closest 19.6 / 19.5 (the exact walks of the 61 queries
// handed over).
bool use_refill(int variant) { return variant != 1; }

}  // namespace

// The queries' workspace on the root device, cached across calls and grown on demand like
// the post stage's buffers.
struct Query {
    DevBuf list;     // 64 B (the fallback count in its first word), then n indices
    DevBuf io;       // host-pointer calls: the rays, then the answers
    Event done;  // the end of the last call's kernels (rt_query_last_exact waits for it)
    int blocks[4] = {0, 0, 0, 0};  // resident blocks per CU of k_rq_fast<ANY, REFILL>, asked once
    int cus = 0;
};

void QueryDelete::operator()(Query* q) const { delete q; }

// (created on first use; b's device is current)
static int query_of(rt_context* c, Backend* b, Query** out)
{
    if (!b->query) {
        Query* q = new Query();
        b->query.reset(q);
        HIPCHK(c, hipEventCreate(&q->done.h));
        HIPCHK(c, hipDeviceGetAttribute(&q->cus, hipDeviceAttributeMultiprocessorCount, b->device));
        const void* fn[4] = {(const void*)k_rq_fast<false, false>, (const void*)k_rq_fast<false, true>,
                             (const void*)k_rq_fast<true, false>, (const void*)k_rq_fast<true, true>};
        for (int i = 0; i < 4; i++) {
            HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&q->blocks[i], fn[i], 256, 0));
            q->blocks[i] = std::max(1, std::min(8, q->blocks[i]));
        }
    }
    *out = b->query.get();
    return RT_OK;
}

int rt_backend_query(rt_context* c, bool any, bool all_exact, const void* rays, long n, void* out, bool device,
                     void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    Query* Q = nullptr;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    if (int r = query_of(c, b, &Q)) return r;
    hipStream_t s = st.s;
    const size_t ray_bytes = (size_t)n * 24, out_bytes = (size_t)n * (any ? 4 : 4 * RQ_WORDS);
    if (int r = st.staging(Q->io, st.pad(ray_bytes) + out_bytes)) return r;
    const float* d_rays = (const float*)st.in(rays, ray_bytes);
    int32_t* d_out = (int32_t*)st.out(out, out_bytes);
    const int ni = (int)n;  // (n < 2^27, rt_capi_host.cpp)
    const unsigned per_thread = (unsigned)((n + 255) / 256);
    c->query_on_device = !all_exact;
    c->query_exact = n;
    if (!all_exact)
        if (int r = ensure(c, Q->list, 64 + (size_t)n * 4)) return r;
    if (int r = st.begin()) return r;
    if (all_exact) {
        hipLaunchKernelGGL(k_rq_exact, dim3(per_thread), dim3(256), 0, s, b->view, d_rays, d_out, ni,
                           (const int32_t*)nullptr, (const int32_t*)nullptr, any ? 1 : 0);
        HIPCHK(c, hipGetLastError());
    } else {
        int32_t* count = (int32_t*)Q->list.p;
        int32_t* list = count + 16;
        const bool refill = use_refill(c->sched.variant[RT_VAR_RQ]);
        // whole waves of 16 queries; at most what is resident at once (the rest by stride)
        const unsigned resident = (unsigned)(Q->cus * Q->blocks[(any ? 2 : 0) + (refill ? 1 : 0)]);
        const unsigned fast_blocks = std::min((unsigned)((n + 63) / 64), resident);
        // (the list's length is known on the device only: a grid for the near-box shares the
        // render sees, the rest by stride)
        const unsigned exact_blocks = std::min(per_thread, (unsigned)Q->cus * 8u);
        HIPCHK(c, hipMemsetAsync(count, 0, 4, s));
        if (any) {
            if (refill)
                hipLaunchKernelGGL((k_rq_fast<true, true>), dim3(fast_blocks), dim3(256), 0, s, b->view, d_rays, d_out, ni, list, count);
            else
                hipLaunchKernelGGL((k_rq_fast<true, false>), dim3(fast_blocks), dim3(256), 0, s, b->view, d_rays, d_out, ni, list, count);
        } else {
            if (refill)
                hipLaunchKernelGGL((k_rq_fast<false, true>), dim3(fast_blocks), dim3(256), 0, s, b->view, d_rays, d_out, ni, list, count);
            else
                hipLaunchKernelGGL((k_rq_fast<false, false>), dim3(fast_blocks), dim3(256), 0, s, b->view, d_rays, d_out, ni, list, count);
        }
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_rq_exact, dim3(exact_blocks), dim3(256), 0, s, b->view, d_rays, d_out, ni,
                           (const int32_t*)list, (const int32_t*)count, any ? 1 : 0);
        HIPCHK(c, hipGetLastError());
    }
    if (int r = st.stop()) return r;
    HIPCHK(c, hipEventRecord(Q->done, s));
    return st.finish();
}

long rt_backend_query_last_exact(rt_context* c)
{
    Backend* b = rt_backend_dev0(c);
    DeviceScope sc;
    Query* Q = nullptr;
    if (int r = sc.enter(c, b->device)) return r;
    if (int r = query_of(c, b, &Q)) return r;
    if (!c->query_on_device) {
        // (every query took the exact walk, or no call yet: known on the host; wait all the same)
        if (c->query_exact > 0) HIPCHK(c, hipEventSynchronize(Q->done));
        return c->query_exact;
    }
    HIPCHK(c, hipEventSynchronize(Q->done));
    int32_t v = 0;
    HIPCHK(c, hipMemcpy(&v, Q->list.p, 4, hipMemcpyDeviceToHost));
    return v;
}
