// rt_render.hip — gfx950 backend of librt_hip.so: device buffers, the
// wavefront render kernels and their launches.
//
// A render (run_wave) is a loop of iterations over the in-flight path slots
// (one slot per pixel of the launch), split into up to 3 independent lanes on
// their own streams:
//   k_trace  every closest-hit and occlusion query of the iteration, walked
//            by quads of lanes over the search BVH with octree verification
//            (rt_quad.h), as a per-wave stream with quad refill; queries it
//            cannot settle go to the fallback lists
//   k_step   its first blocks walk the fallbacks (and resume parked walks)
//            with the exact octree walk (rt_traverse.h); the rest resolve the
//            last bounce, shade the new hit (RNG draws, sampling) or end the
//            sample / start the next one, and append the emitted rays to five
//            per-kind queues (64-way sharded, wave-aggregated atomics)
//   k_tail   once few paths are left: all of them in one launch, each wave
//            stepping its own paths and tracing their rays with its quads
// Queue sizes live in device memory; the host only launches and, every 8
// iterations, reads the live-slot count.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>
#include <algorithm>

#include <chrono>
#include <thread>

#include "rt_backend_hip.h"
#include "rt_wave.h"
#include "rt_quad.h"
#include "rt_row.h"
#include "rt_octet.h"

namespace {

#ifndef RT_STEP_OCC
#define RT_STEP_OCC 3  // k_step waves per SIMD
#endif
#ifndef RT_STEP_FILL
// k_step: blocks per CU at most, one grid-fill at its occupancy (one slot per thread below
// that; above, each wave strides over 64-slot chunks). cfg2 over 4 A/B rounds on 2 boxes:
// 8 / 4 / 3 / 2 -> 128.8-129.3 / 128.5-128.9 / 128.0-128.4 / 127.3-128.4 ms
// (profiles/r06_step_fill_ab.json)
#define RT_STEP_FILL RT_STEP_OCC
#endif
#ifndef RT_TAIL_ROWS
#define RT_TAIL_ROWS 1  // k_tail walks with rows (rt_row.h)
#endif

// counters[] layout (int32). Iteration i (p = i & 1) runs k_trace(i) then
// k_step(i); every set is zeroed by a launch between its last reader and its
// next writer, so no reset launch is needed:
//   Q[p]      queue sizes     filled by k_step(i-1) / k_init, read by k_trace(i); k_trace(i) zeroes Q[p^1]
//   ACT[p]    live count      filled by k_step(i-1) / k_init, read by k_step(i);  k_trace(i) zeroes ACT[p^1]
//   FB[p]     fallback lists  filled by k_trace(i) (queries the quad walk could not settle), walked
//                             exactly by k_step(i); k_step(i) zeroes FB[p^1] for k_trace(i + 1)
//   PARK[p]   parked walks    filled by k_step(i), resumed by k_step(i + 1); k_trace(i) zeroes PARK[p]
//   DONE[p]   finished walks  slots, filled by k_step(i); k_trace(i + 1) releases them (r_park -= 1)
//                             and k_step(i + 1) zeroes DONE[p]. The release waits for a kernel
//                             boundary so the walk's results are visible before the path steps.
//   TK        exact-walk work tickets of k_step(i); k_trace(i) zeroes them
//
// Q and ACT are sharded: the appends of a 64-item input chunk go to one of
// RT_QSHARDS shards (append_emit), each a segment of W.seg_cap entries with
// its own counter on its own 128-B line. One counter per queue took every
// wave's atomic: ~630 us per 2 M appends on 6 counters against ~25 us
// sharded 64 ways (tools/micro/atomics.hip on the MI355X).
enum {
    C_FBC0 = 0,
    C_FBC1,
    C_FBA0,
    C_FBA1,
    C_PARKC0,
    C_PARKC1,
    C_PARKA0,
    C_PARKA1,
    C_TK_EXACT_C,
    C_TK_EXACT_A,
    C_TK_TAIL,       // k_tail: next live-list entry to take
    C_DONE0,
    C_DONE1,
    C_SHARDED = 64,  // sharded counters from here (qc_at / ac_at)
};
#define RT_QSHARDS 64
#define RT_HSHARDS 8   // heavy-class shards per kind (input shard sh -> heavy shard sh % 8)
#define RT_CSTRIDE 32  // ints from one sharded counter to the next (one 128-B line each)
#define C_HEAVY (C_SHARDED + (2 * rtk::RK_COUNT + 2) * RT_QSHARDS * RT_CSTRIDE)
#define C_COUNT (C_HEAVY + 2 * rtk::RK_COUNT * RT_HSHARDS * RT_CSTRIDE)
#define C_ZERO (C_SHARDED - 1)  // never written: the count of a padding segment
__host__ __device__ __forceinline__ int qc_at(int par, int kind, int shard)
{
    return C_SHARDED + ((par * rtk::RK_COUNT + kind) * RT_QSHARDS + shard) * RT_CSTRIDE;
}
__host__ __device__ __forceinline__ int ac_at(int par, int shard)
{
    return C_SHARDED + ((2 * rtk::RK_COUNT + par) * RT_QSHARDS + shard) * RT_CSTRIDE;
}
__host__ __device__ __forceinline__ int hc_at(int par, int kind, int shard)
{
    return C_HEAVY + ((par * rtk::RK_COUNT + kind) * RT_HSHARDS + shard) * RT_CSTRIDE;
}

// Queue segments in k_trace's stream order. Each role's heavy class comes first, so the
// walks predicted long (their path's previous query of the kind took >= W.heavy_calls
// trips) start at the head of every wave's stream instead of setting its drain:
//   [closest kinds' heavy shards][closest kinds' shards][occlusion kinds' heavy][occlusion kinds']
// then zero-count padding to a multiple of 64 (shard_prefix).
#define RT_NCK 4  // closest kinds: CONT, LSH, BL, CAM
#define RT_SEG_CH (RT_NCK * RT_HSHARDS)
#define RT_SEG_AH (RT_SEG_CH + RT_NCK * RT_QSHARDS)
#define RT_SEG_A (RT_SEG_AH + (rtk::RK_COUNT - RT_NCK) * RT_HSHARDS)
#define RT_SEG_END (RT_SEG_A + (rtk::RK_COUNT - RT_NCK) * RT_QSHARDS)
#define RT_NSEG ((RT_SEG_END + 63) / 64 * 64)
struct SegId {
    int kind, shard;
    bool heavy;
};
__host__ __device__ __forceinline__ SegId seg_id(int j)
{
    SegId s;
    if (j < RT_SEG_CH) {
        s.heavy = true, s.kind = j / RT_HSHARDS, s.shard = j % RT_HSHARDS;
    } else if (j < RT_SEG_AH) {
        s.heavy = false, s.kind = (j - RT_SEG_CH) / RT_QSHARDS, s.shard = (j - RT_SEG_CH) % RT_QSHARDS;
    } else if (j < RT_SEG_A) {
        s.heavy = true, s.kind = RT_NCK + (j - RT_SEG_AH) / RT_HSHARDS, s.shard = (j - RT_SEG_AH) % RT_HSHARDS;
    } else {
        s.heavy = false, s.kind = RT_NCK + (j - RT_SEG_A) / RT_QSHARDS, s.shard = (j - RT_SEG_A) % RT_QSHARDS;
    }
    return s;
}
__host__ __device__ __forceinline__ int seg_counter(int par, int j)
{
    if (j >= RT_SEG_END) return C_ZERO;
    const SegId s = seg_id(j);
    return s.heavy ? hc_at(par, s.kind, s.shard) : qc_at(par, s.kind, s.shard);
}


// ------------------------------------------------------------ wave helpers
#ifndef RT_DEBUG_FB
#define RT_DEBUG_FB 0  // study builds: count k_trace's exact-walk hand-overs and the octet walks'
                       // parks of the timed renders, printed on stderr after each run_wave
#endif
#if RT_DEBUG_FB
__device__ unsigned long long rt_dbg_fb[8];  // k_trace closest fallbacks, octet parks, occlusion fallbacks, overflows, ties, chain fails, from rows, -
#define RT_DBG(i) atomicAdd(&rt_dbg_fb[i], 1ull)
#else
#define RT_DBG(i) ((void)0)
#endif
__device__ __forceinline__ int lane_id() { return __lane_id(); }

// Per-lane traversal stack in LDS: entry i of thread t at [i * 256 + t]
// (a wave at equal depth touches 64 consecutive words: no bank conflicts).
template <int N>
struct LdsStack {
    static constexpr int CAP = N;
    uint32_t* r;
    float* k;
    __device__ __forceinline__ uint32_t rec(int i) const { return r[i * 256]; }
    __device__ __forceinline__ float key(int i) const { return k[i * 256]; }
    __device__ __forceinline__ void set(int i, uint32_t rv, float kv)
    {
        r[i * 256] = rv;
        k[i * 256] = kv;
    }
    __device__ __forceinline__ void set_rec(int i, uint32_t rv) { r[i * 256] = rv; }
};

// Static wave-strided work assignment: wave w of the grid takes items
// [w*64, w*64+64), then strides by the grid's wave count. (A shared atomic
// ticket per 64 items serialized ~4k atomics on one address per launch:
// ~45 us even for an empty queue.)
__device__ __forceinline__ int wave_gid() { return (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); }
__device__ __forceinline__ int wave_count() { return (int)((gridDim.x * blockDim.x) >> 6); }

template <bool STATS>
__device__ __forceinline__ void flush_stats(const rtk::Stats& st, unsigned long long* out)
{
    if (STATS)
        for (int i = 0; i < RT_STAT_COUNT; i++)
            if (st.c[i]) atomicAdd(&out[i], st.c[i]);
}

// ------------------------------------------------------------------ kernels
// Queue record base of (kind, heavy class, shard): a normal shard holds seg_cap records, a
// heavy shard RT_QSHARDS / RT_HSHARDS seg_caps (it takes the input shards sh with sh % RT_HSHARDS = its index).
__host__ __device__ __forceinline__ size_t qbase(bool heavy, int shard, size_t seg_cap)
{
    return heavy ? ((size_t)RT_QSHARDS + (size_t)shard * (RT_QSHARDS / RT_HSHARDS)) * seg_cap : (size_t)shard * seg_cap;
}

// Appends what the wave's lanes emitted to the queues and the live list of
// parity pout, in the shard of the 64-item input chunk `base` (whole wave).
// Shards take contiguous runs of the n_in inputs' chunks, so a queue read in
// order follows its input order (pixel order, through the compactions).
template <class E>
__device__ __forceinline__ void append_emit(const rtk::WaveView& W, int pout, int base, int n_in, int p, const E& e)
{
    const int cps = ((n_in + 63) / 64 + RT_QSHARDS - 1) / RT_QSHARDS;  // chunks per shard
    const int sh = min(RT_QSHARDS - 1, (base >> 6) / cps);
    const size_t seg = (size_t)sh * W.seg_cap;
    const unsigned long long lt = (lane_id() == 0) ? 0ull : (~0ull >> (64 - lane_id()));
    if (W.r_heavy) {  // heavy class on: the rays of a path flagged heavy go to its kind's heavy shard
        const int hs = sh % RT_HSHARDS;
        unsigned long long b[2 * rtk::RK_COUNT + 1];
#pragma unroll
        for (int k = 0; k < rtk::RK_COUNT; k++) {
            const bool m = (e.mask >> k) & 1u;
            b[k] = __ballot(m && !e.heavy);
            b[rtk::RK_COUNT + k] = __ballot(m && e.heavy);
        }
        b[2 * rtk::RK_COUNT] = __ballot(e.active);
        int r[2 * rtk::RK_COUNT + 1];
        if (lane_id() == 0) {
#pragma unroll
            for (int k = 0; k <= 2 * rtk::RK_COUNT; k++) {
                const int c = k < rtk::RK_COUNT ? qc_at(pout, k, sh)
                              : k < 2 * rtk::RK_COUNT ? hc_at(pout, k - rtk::RK_COUNT, hs)
                                                      : ac_at(pout, sh);
                r[k] = b[k] ? atomicAdd(W.counters + c, __popcll(b[k])) : 0;
            }
        }
#pragma unroll
        for (int k = 0; k < rtk::RK_COUNT; k++) {
            const int ih = __shfl(r[rtk::RK_COUNT + k], 0) + __popcll(b[rtk::RK_COUNT + k] & lt);
            const int i = __shfl(r[k], 0) + __popcll(b[k] & lt);
            if ((e.mask >> k) & 1u) W.q[k][e.heavy ? qbase(true, hs, W.seg_cap) + ih : qbase(false, sh, W.seg_cap) + i] = e.rec(k, p);
        }
        const int a = __shfl(r[2 * rtk::RK_COUNT], 0) + __popcll(b[2 * rtk::RK_COUNT] & lt);
        if (e.active) W.act_out[seg + a] = p;
        return;
    }
    // the six reservations (five queues, the live list) issued back to back by lane 0
    // and waited for once, then the stores: one atomic round trip, not six in a row
    unsigned long long b[rtk::RK_COUNT + 1];
#pragma unroll
    for (int k = 0; k < rtk::RK_COUNT; k++) b[k] = __ballot((e.mask >> k) & 1u);
    b[rtk::RK_COUNT] = __ballot(e.active);
    int r[rtk::RK_COUNT + 1];
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k <= rtk::RK_COUNT; k++)
            r[k] = b[k] ? atomicAdd(W.counters + (k < rtk::RK_COUNT ? qc_at(pout, k, sh) : ac_at(pout, sh)),
                                    __popcll(b[k]))
                        : 0;
    }
#pragma unroll
    for (int k = 0; k < rtk::RK_COUNT; k++) {
        const int i = __shfl(r[k], 0) + __popcll(b[k] & lt);
        if ((e.mask >> k) & 1u) W.q[k][qbase(false, sh, W.seg_cap) + i] = e.rec(k, p);
    }
    const int a = __shfl(r[rtk::RK_COUNT], 0) + __popcll(b[rtk::RK_COUNT] & lt);
    if (e.active) W.act_out[seg + a] = p;
}


// Exclusive prefix sums of the sharded counters at cnt[at(j)], j < m (m a
// multiple of 64), into pre[0..m] (LDS); every thread of the block calls.
template <class AT>
__device__ __forceinline__ void shard_prefix(const int32_t* cnt, int m, AT at, int* pre)
{
    const int nw = (int)(blockDim.x >> 6), w = (int)(threadIdx.x >> 6);
    for (int g = w; g < m / 64; g += nw) {  // one wave per 64 counters: inclusive scan
        int v = cnt[at(g * 64 + lane_id())];
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o);
            if (lane_id() >= o) v += u;
        }
        pre[g * 64 + lane_id() + 1] = v;
    }
    __syncthreads();
    // chain the groups: entry (g, lane) adds the totals of groups < g (read before any write)
    int add[8];
    const int ng = m / 64;
    for (int g = w; g < ng && g < 8 * nw; g += nw) {
        int off = 0;
        for (int h = 0; h < g; h++) off += pre[h * 64 + 64];
        add[g / nw] = off;
    }
    __syncthreads();
    for (int g = w; g < ng && g < 8 * nw; g += nw) pre[g * 64 + lane_id() + 1] += add[g / nw];
    if (threadIdx.x == 0) pre[0] = 0;
    __syncthreads();
}

// Segment j of a prefix table pre[0..m] holding global index g (pre[j] <= g < pre[j+1]).
__device__ __forceinline__ int shard_find(const int* pre, int m, int g)
{
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The same search with M (a compile-time table size) as an 8-way search: each round reads 7
// entries at once (independent LDS reads, one round trip) and advances by the count at or below
// g (the table is non-decreasing), so 448 entries take 3 dependent round trips instead of 9 and
// 64 take 2 instead of 6. k_trace's refill (on ~4 of 5 wave trips, the whole wave waiting) and
// every k_step / k_tail chunk start search these tables.
#ifndef RT_FIND8
#define RT_FIND8 1
#endif
template <int M>
__device__ __forceinline__ int shard_find8(const int* pre, int g)
{
#if RT_FIND8
    constexpr int TOP = M > 512 ? 512 : M > 64 ? 64 : M > 8 ? 8 : 1;
    static_assert(M <= 4096, "three or four 8-way rounds");
    int lo = 0;
#pragma unroll
    for (int step = TOP; step >= 1; step >>= 3) {
        int c = 0;
#pragma unroll
        for (int k = 1; k < 8; k++) {
            const int j = lo + step * k;
            c += (j < M && pre[j] <= g) ? 1 : 0;
        }
        lo += step * c;
    }
    return lo;
#else
    return shard_find(pre, M, g);
#endif
}

// Where stream position g's queue record lives (segment table pre[0..RT_NSEG]) and its kind.
__device__ __forceinline__ const rtk::RayRec* queue_item_ptr(const rtk::WaveView& W, const int* pre, int g, int& kind)
{
    const int j = shard_find8<RT_NSEG>(pre, g);
    const SegId s = seg_id(j);
    kind = s.kind;
    rtk::RayRec* qk = W.q[0];
#pragma unroll
    for (int k2 = 1; k2 < rtk::RK_COUNT; k2++) qk = s.kind == k2 ? W.q[k2] : qk;
    return qk + qbase(s.heavy, s.shard, W.seg_cap) + (g - pre[j]);
}

// Queue item of stream position g (segment table pre[0..RT_NSEG], k_trace): the ray and its kind.
__device__ __forceinline__ rtk::RayRec queue_item_at(const rtk::WaveView& W, const int* pre, int g, int& kind)
{
    // (the queue base by selects: W.q[kind] with a lane-varying kind would be a load; heavy
    // shard h: after the kind's RT_QSHARDS segments, RT_QSHARDS / RT_HSHARDS seg_caps each)
    return *queue_item_ptr(W, pre, g, kind);
}

// k_trace's look-ahead (RT_TRACE_PREFETCH): right after a refill, the wave's next 16 stream
// positions are copied into its LDS buffer by direct-to-LDS loads (lane 2i + h: half h of
// record i, 16 B; the hardware puts lane L's 16 B at buf + 16 L), their kinds alongside; the next
// refill takes its records from there (a refill needs at most 16 positions, all from the
// cursor on, which the buffer starts at), so the refill no longer waits on the queue's memory.
#ifndef RT_TRACE_PREFETCH
#define RT_TRACE_PREFETCH 1
#endif
struct QPrefetch {
    float4_* buf;  // the wave's 64 x 16 B (records 0..15 in the first 512 B)
    int* kind;     // the wave's 16 kinds (-1: past the end of the stream)
};
__device__ __forceinline__ void queue_prefetch(const rtk::WaveView& W, const int* pre, const QPrefetch& pf, int first, int cursor,
                                               int wg, int wn, int total)
{
    const int lane = lane_id(), i = lane >> 1;
    const int j = cursor + i;
    const int idx = (wg + (j >> 4) * wn) * 16 + (j & 15);
    const bool ok = lane < 32 && idx < total;
    int kind = -1;
    if (ok) {
        const rtk::RayRec* rp = queue_item_ptr(W, pre, first + idx, kind);
        __builtin_amdgcn_global_load_lds((const void*)((const float4_*)rp + (lane & 1)),
                                         (__attribute__((address_space(3))) void*)pf.buf, 16, 0, 0);
    }
    if (lane < 32 && (lane & 1) == 0) pf.kind[i] = ok ? kind : -1;
}

// Path init: every slot seeds its RNG and emits its first camera ray (into Q[0], ACT[0]).
__global__ __launch_bounds__(256) void k_init(rtk::WaveView W)
{
    rtlibm::lds_tables_init();  // (a pixel of a 0-bounce render is tone-mapped here)
    const int p = blockIdx.x * blockDim.x + threadIdx.x;  // grid covers whole waves
    rtk::Emit e;
    e.mask = 0;
    e.active = false;
    e.heavy = false;
    if (p < W.n_slots) rtk::path_init(W, p, e);
    append_emit(W, 0, p & ~63, W.n_slots, p, e);
}

// k_init of a progressive pass after the first: every slot goes on from its pixel's paused
// state (rt_wave.h path_resume) and emits the camera ray of the pass's first sample.
__global__ __launch_bounds__(256) void k_resume(rtk::WaveView W)
{
    rtlibm::lds_tables_init();
    const int p = blockIdx.x * blockDim.x + threadIdx.x;  // grid covers whole waves
    rtk::Emit e;
    e.mask = 0;
    e.active = false;
    e.heavy = false;
    if (p < W.n_slots) rtk::path_resume(W, p, e);
    append_emit(W, 0, p & ~63, W.n_slots, p, e);
}

// A progression's image after `done` samples: one thread per pixel of the shard, base and
// paused state in, the tone-mapped pixel out (rt_wave.h resolve_pixel). Changes no state.
__global__ __launch_bounds__(256) void k_resolve(const float4_* __restrict__ base, const float4_* __restrict__ state,
                                                 float4_* __restrict__ out, int n, int done)
{
    rtlibm::lds_tables_init();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rtk::resolve_pixel(base[i], state[i], done);
}

// After a lane's last step: the tone-map of every pixel of the lane (rt_wave.h tonemap_pixel).
__global__ __launch_bounds__(256) void k_tonemap(rtk::WaveView W)
{
    rtlibm::lds_tables_init();
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < W.n_slots) rtk::tonemap_pixel(W, p);
}

// ------------------------------------------------------------- query kernel
// Every closest-hit and occlusion query of the iteration, plus the exact
// octree walks of the queries the previous iteration could not settle, in
// one launch: the blocks are split into four roles computed alike by every
// block from the counters.
//  * exact roles (blocks first, so their long dependent walks start early
//    and hide under the bulk): the previous launch's fallback lists and
//    parked walks, through the resumable octree walk (rt_traverse.h).
//    Persistent waves; idle lanes refill once RT_REFILL of them are idle; a
//    walk that has taken W.budget steps parks at its next node boundary and
//    continues in the next launch.
//  * fast roles (the rest, split in proportion to the two queues): one query
//    per lane through the search BVH (rt_fast.h), node-index stack in LDS. A
//    query whose answer needs the exact walk (or whose stack would overflow)
//    goes to the fallback list for the next launch, and its slot's r_park
//    count keeps k_step off the path until the walk has finished.
#ifndef RT_STEP_EMIT_LDS
#define RT_STEP_EMIT_LDS 1  // k_step's and k_tail's emitted rays wait in LDS (rt_wave.h EmitLds), not in VGPRs
#endif
#define RT_LDS_WORDS 16         // LDS words per lane of k_trace (16 KB per block of 256)
#define RT_LDS_CAP_FAST 16      // search-BVH stack: node + key in LDS ...
#define RT_SPILL_FAST RT_FAST_SPILL  // ... then in the lane's global spill area
#define RT_LDS_CAP_CLOSEST 8    // exact walks: key + record (windows are powers of two)
#define RT_LDS_CAP_ANY 16
#define RT_REFILL 16
#define RT_QSTACK 32            // quad walks (rt_quad.h): stack entries per quad (item + key, 64 quads per block)
#define RT_RSTACK 64            // row walks (rt_row.h): stack entries per row (item + key, 16 rows per block)
#ifndef RT_TRACE_REFILL
#define RT_TRACE_REFILL 4       // k_trace: idle quads of a wave that trigger a refill from its query stream
                                // (r02, cfg2: 4 / 8 -> 726 / 723 vs 678 Msamples/s with static 16-query chunks)
#endif
#ifndef RT_HEAVY_CALLS
#define RT_HEAVY_CALLS 6        // heavy class (seg_id): quad_visit calls of a walk that flag its path (0: off).
                                // cfg2 (r02): off / 3 / 6 / 10 / 16 -> 737 / 744 / 744-748 / 740 / 735 Msamples/s;
                                // 1-lane k_trace 124.1 -> 117.2 ms, drain slots 838 M -> 737 M
                                // (a dynamic, per-XCD-ticketed tail of the stream, 10-40 %: 684-691, rejected)
#endif
#ifndef RT_TRACE_OCC
#define RT_TRACE_OCC 6          // k_trace waves per SIMD (8 fits the quad walks in 64 VGPRs but measured
                                // 512 vs 539 Msamples/s: more trace waves crowd the other lanes k_step)
#endif

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

// Does this query skip the search-BVH walk for the exact octree walk? Its origin lies outside
// the near box (rt_fast.h far_origin), or the force_fallback stressor's ray hash selects it.
__device__ __forceinline__ bool forced_fallback(const rtk::WaveView& W, const float4_& o, const float4_& d)
{
    return (W.far_check && rtk::far_origin(W.S, rtk::v3of(o))) || rtk::forced_fallback(W.force_fb, o, d);
}

// Blocks [0, n0) take role 0, the rest role 1, in proportion to the work.
__device__ __forceinline__ int split_blocks(int nb, int w0, int w1)
{
    if (w0 + w1 == 0) return 0;
    int n0 = (int)((long)nb * w0 / ((long)w0 + w1));
    if (w0 > 0 && n0 == 0) n0 = 1;
    if (w1 > 0 && n0 == nb) n0 = nb - 1;
    return n0;
}

// A finished exact walk: its slot goes to DONE[par]; k_trace(i + 1) releases it.
__device__ __forceinline__ void walk_done(const rtk::WaveView& W, int par, uint32_t target)
{
    const int j = atomicAdd(W.counters + C_DONE0 + par, 1);
    W.done[par][j] = (int32_t)(target >> 3);
}

// (k_step's exact walks take 8 lanes per query, rt_octet.h; the one-lane-per-query walks they
// replaced were measured in profiles/r04m_exact_octets.json)
// Exact octree walks of k_step(i) (par = i & 1), one octet of lanes per query (rt_octet.h):
// the walks parked by k_step(i - 1) (PARK[par ^ 1], the first n_res tickets), then the
// fallbacks of k_trace(i) (FB[par]). ANY selects the occlusion walk.
template <bool ANY>
__device__ void exact_octets(const rtk::WaveView& W, int par, uint32_t* lds, int lane, int n_res, int total,
                             rtk::Stats* st)
{
    rtk::OctRing w = rtk::oct_ring(lds);
    const int sub = lane_id() & 7;
    uint32_t* spr = W.spill_r + (size_t)(lane & ~7) * RT_STACK_CAP;  // the leader lane's spill area
    float* spk = W.spill_k + (size_t)(lane & ~7) * RT_STACK_CAP;
    const rtk::RayRec* fb = ANY ? W.fb_a[par] : W.fb_c[par];
    int32_t* ticket = W.counters + (ANY ? C_TK_EXACT_A : C_TK_EXACT_C);
    int32_t* parked = W.counters + (ANY ? C_PARKA0 : C_PARKC0) + par;
    rtk::TravG T;
    bool has = false, drained = false;  // (octet-uniform)
    uint32_t target = 0;
    auto done = [&]() {
        if (sub == 0) {
            if (ANY)
                rtk::finish_any(W, target, T.hit);  // (false, or the brute-force answer)
            else
                rtk::finish_closest(W, target, T.o, T.d, T.best_t, T.best_k);
            walk_done(W, par, target);
        }
    };
    for (;;) {
        const unsigned long long bneed = __ballot(!has && sub == 0);
        const int nneed = __popcll(bneed);
        if (!drained && (nneed >= RT_REFILL / 8 || nneed == 8)) {
            int base = 0;
            if (lane_id() == 0) base = atomicAdd(ticket, nneed);
            base = __shfl(base, 0);
            if (base + nneed >= total) drained = true;
            if (!has) {
                const int idx = base + __popcll(bneed & ((1ull << rtk::oct_lane0()) - 1ull));
                if (idx < n_res) {
                    target = ANY ? rtk::octa_resume(W.S, &W.park_a[par ^ 1][idx], T, w, sub)
                                 : rtk::octc_resume(W.S, &W.park_c[par ^ 1][idx], T, w, sub);
                    has = true;
                } else if (idx < total) {
                    const rtk::RayRec r = fb[idx - n_res];
                    target = (rt_asuint(r.o.w) << 3) | rt_asuint(r.d.w);
                    if (st && sub == 0) st->c[RT_STAT_FALLBACK]++;
                    has = rtk::octg_setup(W.S, T, rtk::v3of(r.o), rtk::v3of(r.d), st, ANY, sub);
                    if (!has) done();
                }
            }
        }
        if (!__any(has)) {
            if (drained) break;
            continue;
        }
        if (has) {
            if (ANY)
                rtk::octa_node(W.S, T, w, spr, sub, st);
            else
                rtk::octc_node(W.S, T, w, spr, spk, sub, st);
            if (T.mode == rtk::TM_DONE) {
                done();
                has = false;
            } else if (T.steps >= W.budget && (ANY ? rtk::octa_parkable(T) : rtk::octc_parkable(T))) {
                int ps = 0;
                if (sub == 0) ps = atomicAdd(parked, 1);
                if (sub == 0) RT_DBG(1);
                ps = __shfl(ps, rtk::oct_lane0());
                if (ps < W.park_cap) {
                    if (ANY)
                        rtk::octa_park(T, w, target, &W.park_a[par][ps], sub);
                    else
                        rtk::octc_park(T, w, target, &W.park_c[par][ps], sub);
                    has = false;
                } else {
                    T.steps = 0;  // park pool full: keep going
                }
            }
        }
    }
}

// Path step of iteration i (par = i & 1): resolve, shade, next sample, for
// every live path not waiting on an exact walk; the first blocks instead run
// the exact octree walks of this iteration's fallbacks and of the walks parked
// last iteration (they need the registers this kernel has anyway; k_trace
// stays small enough for 8 waves per SIMD).
// PROG: the instantiation a progressive pass launches (rt_wave.h finish_pixel pauses the pixel).
template <bool STATS, bool PROG = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_STEP_OCC, 8))) void k_step(rtk::WaveView W, int par, unsigned long long* stats)
{
    // (the exact roles' stacks; in the path-step blocks, the emitted rays: rt_wave.h EmitLds)
    __shared__ uint32_t s_lds[(RT_STEP_EMIT_LDS ? 6 * rtk::RK_COUNT : RT_LDS_WORDS) * 256];
    static_assert(6 * rtk::RK_COUNT >= RT_LDS_WORDS, "the exact roles' stacks fit the emit columns");
    __shared__ int s_pre[RT_QSHARDS + 1];
    rtlibm::lds_tables_init();
    rtk::lds_shade_init(W.S);  // (the env-map row search and a small material table from LDS)
    int32_t* cnt = W.counters;
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // for k_trace(i + 1); DONE[par ^ 1] was released by k_trace(i)
        cnt[C_FBC0 + (par ^ 1)] = cnt[C_FBA0 + (par ^ 1)] = 0;
        cnt[C_DONE0 + (par ^ 1)] = 0;
        // (k_trace(i)'s hand-overs to the exact walk, summed for rt_device_exact_handovers: a
        // health figure, ~1e-6 of the queries; a search-BVH walk that went wrong shows here)
        const int nf = cnt[C_FBC0 + par] + cnt[C_FBA0 + par];
        if (W.handovers && nf > 0) atomicAdd(W.handovers, (unsigned long long)nf);
    }
    rtk::Stats st;
    if (STATS)
        for (int i = 0; i < RT_STAT_COUNT; i++) st.c[i] = 0;
    rtk::Stats* ps = STATS ? &st : nullptr;
    // exact roles: 32 walks per block to start with (8 octets per wave), at most half of the
    // spill lanes and a quarter of the grid each
    const int nrc = min(cnt[C_PARKC0 + (par ^ 1)], W.park_cap), nra = min(cnt[C_PARKA0 + (par ^ 1)], W.park_cap);
    const int ec = nrc + cnt[C_FBC0 + par], ea = nra + cnt[C_FBA0 + par];
    // (the host launches >= 3 blocks, so both exact roles and the path step each get one:
    // with gridDim 3, half = 1; above, the exact roles take at most half of the grid)
    const int half = min(W.spill_lanes / 512, max(1, (int)gridDim.x / 4));
    constexpr int WPB = 32;  // walks per block at once (octets)
    const int nbe_c = min(half, (ec + WPB - 1) / WPB), nbe_a = min(half, (ea + WPB - 1) / WPB);
    const int b = (int)blockIdx.x;
    if (b < nbe_c) {
        exact_octets<false>(W, par, s_lds, b * 256 + (int)threadIdx.x, nrc, ec, ps);
        flush_stats<STATS>(st, stats);
        return;
    }
    if (b < nbe_c + nbe_a) {
        exact_octets<true>(W, par, s_lds, (W.spill_lanes / 512 + b - nbe_c) * 256 + (int)threadIdx.x, nra, ea, ps);
        flush_stats<STATS>(st, stats);
        return;
    }
    shard_prefix(cnt, RT_QSHARDS, [&](int j) { return ac_at(par, j); }, s_pre);
    const int n = s_pre[RT_QSHARDS];
    if (STATS && W.iterq && b == nbe_c + nbe_a && threadIdx.x == 0 && W.iter < RT_MAX_TIMED_ITERS)
        W.iterq[2 * W.iter + 1] = n;
    const int nbs = (int)gridDim.x - (nbe_c + nbe_a);
    const int wg = (b - nbe_c - nbe_a) * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    const int wn = nbs * (int)(blockDim.x >> 6);
    for (int base = wg * 64; base < n; base += wn * 64) {
        const int idx = base + lane_id();
#if RT_STEP_EMIT_LDS
        rtk::EmitLds<256> e;
        e.s = reinterpret_cast<float*>(s_lds) + threadIdx.x;
#else
        rtk::Emit e;
#endif
        e.mask = 0;
        e.active = false;
        e.heavy = false;
        int p = -1;
        if (idx < n) {
            const int sh = shard_find8<RT_QSHARDS>(s_pre, idx);
            p = W.act_in[(size_t)sh * W.seg_cap + (idx - s_pre[sh])];
            rtk::path_step<PROG>(W, p, e, ps);
        }
        append_emit(W, par ^ 1, base, n, p, e);
    }
    flush_stats<STATS>(st, stats);
}

// The fast lane's hand-over (run_wave), between a lane's k_trace and k_step: the live paths of
// iteration par's list with at most W.fast_thr samples done and no parked query, up to
// W.fast_cap of them, move to W.fast_list (their wait counts become -1: k_step drops them from
// the lane's live list, rt_wave.h path_step; the fast lane's tail kernel clears the mark).
__global__ __launch_bounds__(256) void k_hand(rtk::WaveView W, int par)
{
    __shared__ int s_pre[RT_QSHARDS + 1];
    shard_prefix(W.counters, RT_QSHARDS, [&](int j) { return ac_at(par, j); }, s_pre);
    const int n = s_pre[RT_QSHARDS];
    for (int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x); idx < n; idx += (int)(gridDim.x * blockDim.x)) {
        const int sh = shard_find8<RT_QSHARDS>(s_pre, idx);
        const int p = W.act_in[(size_t)sh * W.seg_cap + (idx - s_pre[sh])];
        if ((int)rt_asuint(W.p_thr[p].w) > W.fast_thr || W.r_park[p] != 0) continue;
        const int j = atomicAdd(W.fast_ticket, 1);
        if (j >= W.fast_cap) continue;
        W.fast_list[j] = p;
        W.r_park[p] = -1;
    }
}

// Samples done by the live paths of iteration par's list (the fast lane's selection, run_wave).
__global__ __launch_bounds__(256) void k_hist(rtk::WaveView W, int par, int32_t* __restrict__ hist)
{
    __shared__ int s_pre[RT_QSHARDS + 1];
    shard_prefix(W.counters, RT_QSHARDS, [&](int j) { return ac_at(par, j); }, s_pre);
    const int n = s_pre[RT_QSHARDS];
    for (int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x); idx < n; idx += (int)(gridDim.x * blockDim.x)) {
        const int sh = shard_find8<RT_QSHARDS>(s_pre, idx);
        const int p = W.act_in[(size_t)sh * W.seg_cap + (idx - s_pre[sh])];
        atomicAdd(hist + min((int)rt_asuint(W.p_thr[p].w), W.spp), 1);
    }
}

// Stats renders with a walk log (rt_test_walk_log, include/rt_hip.h): one record per walk of at
// least W.wlog_min quad_visit calls. where: 0 k_trace quads, 1 a k_trace drain's rows, 2 k_tail.
__device__ __noinline__ void walk_log(const rtk::WaveView& W, rtk::V3 o, rtk::V3 d, uint32_t target, int calls, float t,
                                      int k, int where)
{
    if (W.wlog_every < 0 && t != -2.0f) return;  // (only the walks left to the exact walk)
    if (W.wlog_every > 1 && ((target * 2654435761u) ^ ((uint32_t)W.iter * 40503u)) % (uint32_t)W.wlog_every != 0u) return;
    const int i = atomicAdd(W.wlog_n, 1);
    if (i >= W.wlog_cap) return;
    float4_* r = W.wlog + 3 * (size_t)i;
    r[0] = float4_{o.x, o.y, o.z, rt_asfloat((target & 7u) | ((uint32_t)where << 8))};
    r[1] = float4_{d.x, d.y, d.z, rt_asfloat((uint32_t)calls)};
    r[2] = float4_{t, rt_asfloat((uint32_t)k), rt_asfloat((uint32_t)W.iter), rt_asfloat(target >> 3)};
}

// A row's stack held in its wave's quad stacks (k_trace's drain, trace_stream): row k of a
// wave uses the words of the wave's quads 4k .. 4k+3, entry e at depth e >> 2 of quad
// 4k + (e & 3), so converting the wave's walks to rows needs no other LDS.
struct RowInQuadStack {
    static constexpr int CAP = 4 * RT_QSTACK;
    uint32_t* r;  // the word of quad 4k, depth 0
    float* k;
    __device__ __forceinline__ uint32_t rec(int i) const { return r[(i >> 2) * 64 + (i & 3)]; }
    __device__ __forceinline__ float key(int i) const { return k[(i >> 2) * 64 + (i & 3)]; }
    __device__ __forceinline__ void set(int i, uint32_t rv, float kv)
    {
        r[(i >> 2) * 64 + (i & 3)] = rv;
        k[(i >> 2) * 64 + (i & 3)] = kv;
    }
    __device__ __forceinline__ void set_rec(int i, uint32_t rv) { r[(i >> 2) * 64 + (i & 3)] = rv; }
};

#if RT_DRAIN_STRONG_FENCE  // (study build: the hand-off's ordering made explicit)
#define RT_DRAIN_FENCE()                                       \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); \
        __builtin_amdgcn_s_waitcnt(0);                         \
        __builtin_amdgcn_wave_barrier();                       \
    } while (0)
#else
#define RT_DRAIN_FENCE()                                       \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                       \
    } while (0)
#endif
#ifndef RT_DRAIN_ROWS
#define RT_DRAIN_ROWS 3  // k_trace: once a wave's stream is out and at most this many quads still walk,
                         // their walks continue as rows (rt_row.h); 0 = off. cfg4 8-way shard, one
                         // MI355X (profiles/r04i_drain_probe.json, r04j_probe.json): off / 4 / 3 / 2 / 1 ->
                         // 370-373 / 362.6-362.9 / 359.9-361.4 / 360.5-363.6 / 366.5-367.3 ms, cfg2 148.0 /
                         // 145.3-145.9 / 145.1-145.4 / 145.6-146.0 / 147.1-147.6 ms
#endif

// k_trace's fast roles with per-quad refill (RT_TRACE_REFILL > 0): see k_trace.
// G = lanes per query: 4 (quads over the 4-wide BVH, rt_quad.h) or 16 (rows over the 16-wide
// BVH, rt_row.h). With quads, the drain (the wave's stream out, its last long walks running
// while the other quads idle) continues those walks as rows: same items, same stack entries
// (the 16-wide BVH is numbered like the 4-wide one), half the trips per remaining level.
// BRUTE: rt_quad.h (RT_BRUTE_OFF: the product's walks carry no original indices, QState.h.prim is dead).
template <bool ANY, bool STATS, bool PAIR, int G, int BRUTE, class QSTK>
__device__ __forceinline__ void trace_stream(const rtk::WaveView& W, const RtSceneView& S, QSTK& stk, const int* s_pre,
                                             int first, int total, int wg, int wn, int32_t* fbn, rtk::RayRec* fbl,
                                             rtk::Stats* ps, const QPrefetch& pf)
{
    static_assert(G == 4 || G == 16, "quads or rows");
    constexpr unsigned long long ALL_IDLE = G == 4 ? 0x1111111111111111ull : 0x0001000100010001ull;
    constexpr int REFILL = G == 4 ? RT_TRACE_REFILL : 1;  // idle groups that trigger a refill
    const int lane = lane_id(), qd = lane / G;
    int sub = lane & (G - 1);
    int cursor = 0;                     // the wave's next stream position (uniform)
    bool exhausted = wg * 16 >= total;  // (uniform)
    bool active = false;
    uint32_t target = 0;
    rtk::QState q;  // (its ray is the query's: a fallback record is rebuilt from q.o, q.d and target)
#if RT_TRACE_PREFETCH
    if (!exhausted) queue_prefetch(W, s_pre, pf, first, cursor, wg, wn, total);
#endif
    // a walk's end: its answer, or the exact walk's list; gs = lanes of the group walking it
    auto finish = [&](int res, int gs) {
        // a long walk: the path's next rays go to the heavy class (head of the next streams)
        // (q.calls counts quad_visit calls; a row call covers two 4-wide levels and counts 2)
        if (W.r_heavy && sub == 0 && q.calls >= W.heavy_calls) W.r_heavy[target >> 3] = 1;
        if (STATS && W.iterq && sub == 0 && W.iter < RT_MAX_TIMED_ITERS) {
            // (RT_ITER_LOG: the launch's longest walk in quad_visit calls per role, and
            // how many walks took more than 8)
            int32_t* q2 = W.iterq + 2 * RT_MAX_TIMED_ITERS + 4 * W.iter;
            atomicMax(q2 + (ANY ? 1 : 0), q.calls);
            if (q.calls > 8) atomicAdd(q2 + 2, 1);
        }
        float t = 0.0f;
        int k = 0;
        int why = res < 0 ? 3 : 0;  // (walk log: why the exact walk answers: 1 tie, 2 chain check, 3 stack overflow)
        // (rows: each quad of the row verifies alike; one counts)
        if (res > 0 && !ANY && !rtk::quad_closest_answer<BRUTE>(S, q, sub & 3, t, k, gs == 4 || sub == 0 ? ps : nullptr)) {
            res = -1;
            why = q.h.tie ? 1 : 2;
        }
        if (STATS && W.wlog && sub == 0 && q.calls >= W.wlog_min)
            walk_log(W, q.o, q.d, target, q.calls, res <= 0 ? -2.0f : ANY ? (float)(q.h.k == 1) : t, res <= 0 ? why : k,
                     gs == 4 ? 0 : 1);
        if (sub == 0) {
            if (res > 0) {
                if (ANY)
                    rtk::finish_any(W, target, q.h.k == 1);
                else
                    rtk::finish_closest(W, target, q.o, q.d, t, k);
            } else {  // the exact walk answers it (k_step(i)); the queue record again (o.w: slot)
                fbl[atomicAdd(fbn, 1)] = rtk::RayRec{rtk::f4(q.o, rt_asfloat(target >> 3)),
                                                     rtk::f4(q.d, rt_asfloat(target & 7u))};
                RT_DBG(ANY ? 2 : 0);
                RT_DBG(why == 3 ? 3 : why == 1 ? 4 : 5);
                if (gs == 16) RT_DBG(6);
                atomicAdd(&W.r_park[target >> 3], 1);
                if (STATS && W.iterq && W.iter < RT_MAX_TIMED_ITERS)
                    atomicAdd(W.iterq + 2 * RT_MAX_TIMED_ITERS + 4 * W.iter + 3, 1);  // (RT_ITER_LOG: fallbacks)
            }
        }
    };
    for (;;) {
        const unsigned long long bidle = __ballot(!active && sub == 0);
        if (!exhausted && (__popcll(bidle) >= REFILL || bidle == ALL_IDLE)) {
            if (!active) {
                const int j = cursor + __popcll(bidle & ((1ull << (qd * G)) - 1ull));  // this group's stream position
                const int idx = (wg + (j >> 4) * wn) * 16 + (j & 15);
                if (idx < total) {
#if RT_TRACE_PREFETCH
                    const int slot = j - cursor;  // (0..15: the buffer starts at the cursor)
                    // (the compiler does not order LDS reads after direct-to-LDS loads: wait for
                    // the vector-memory counter here, vmcnt(0), before reading the buffer)
                    __builtin_amdgcn_s_waitcnt(0x0F70);
                    rtk::RayRec r;
                    r.o = pf.buf[2 * slot];
                    r.d = pf.buf[2 * slot + 1];
                    const int kind = pf.kind[slot];
#else
                    int kind;
                    rtk::RayRec r = queue_item_at(W, s_pre, first + idx, kind);
#endif
                    target = (rt_asuint(r.o.w) << 3) | (uint32_t)kind;
                    if (forced_fallback(W, r.o, r.d)) {
                        if (sub == 0) {
                            r.d.w = rt_asfloat(target & 7u);
                            fbl[atomicAdd(fbn, 1)] = r;
                            atomicAdd(&W.r_park[target >> 3], 1);
                        }
                    } else if (rtk::qstate_begin<ANY>(q, rtk::v3of(r.o), rtk::v3of(r.d), sub, ps)) {
                        active = true;
                        q.calls = 0;
                    } else if (sub == 0) {  // (a NaN ray: no hit)
                        if (ANY)
                            rtk::finish_any(W, target, false);
                        else
                            rtk::finish_closest(W, target, q.o, q.d, -1.0f, -1);
                    }
                }
            }
            cursor += __popcll(bidle);
            exhausted = (wg + (cursor >> 4) * wn) * 16 >= total;
#if RT_TRACE_PREFETCH
            // (every lane has read its record: the buffer is free for the next 16 positions)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (!exhausted) queue_prefetch(W, s_pre, pf, first, cursor, wg, wn, total);
#endif
            if (STATS && lane == 0) ps->c[RT_STAT_REFILLS]++;
        }
        const unsigned long long bact = __ballot(active && sub == 0);
        if (!bact) {
            if (exhausted) break;
            continue;
        }
        if (G == 4 && W.drain_rows > 0 && exhausted && __popcll(bact) <= W.drain_rows) break;  // to rows (below)
        if (STATS) {  // SIMT slots of this trip: 16 quads, the active ones used
            if (active && sub == 0) ps->c[exhausted ? RT_STAT_DRAIN_VISITS : RT_STAT_QUAD_VISITS]++;
            if (lane == 0) ps->c[exhausted ? RT_STAT_DRAIN_SLOTS : RT_STAT_WAVE_SLOTS] += 64 / G;
        }
        if (active) {
            int res;
            if constexpr (G == 4)
                res = rtk::quad_visit<ANY, RT_VISIT_DESCEND, PAIR, BRUTE>(S, q, stk, sub, ps);
            else
                res = rtk::row_visit<ANY, RT_VISIT_DESCEND, BRUTE>(S, q, stk, sub, ps);
            q.calls += G == 4 ? 1 : 2;
            if (res != 0) {
                active = false;
                finish(res, G);
            }
        }
    }
    if constexpr (G == 4) {
        // The drain as rows: the k-th walking quad of the wave (lane order) continues on row k.
        const unsigned long long bact = __ballot(active && sub == 0);
        if (!bact) return;
        const int row = lane >> 4;
        unsigned long long m = bact;
        for (int i = 0; i < row; i++) m &= m - 1ull;
#ifndef RT_DRAIN_SRC_LANE
#define RT_DRAIN_SRC_LANE 0  // (study: which lane of the walking quad hands its state to the row)
#endif
        const int src = (m ? __ffsll((long long)m) - 1 : 0) + RT_DRAIN_SRC_LANE;  // the walking quad's lane
        const bool ract = m != 0;
        // its state (quad-uniform) to the row's lanes
        auto pf = [&](float v) { return __shfl(v, src); };
        auto pi = [&](int v) { return __shfl(v, src); };
        q.o = rtk::v3(pf(q.o.x), pf(q.o.y), pf(q.o.z));
        q.d = rtk::v3(pf(q.d.x), pf(q.d.y), pf(q.d.z));
        for (int i = 0; i < 3; i++) q.rb.inv[i] = pf(q.rb.inv[i]), q.rb.oi[i] = pf(q.rb.oi[i]);
        q.h.t = pf(q.h.t), q.h.t2 = pf(q.h.t2), q.h.k = pi(q.h.k), q.h.leaf = pi(q.h.leaf);
        if (BRUTE != RT_BRUTE_OFF) q.h.prim = pi(q.h.prim);  // (else no walk reads it)
        q.h.tie = pi(q.h.tie ? 1 : 0) != 0;  // (q.h.ovf: the one-lane walks' flag; these walks return -1 instead)
        q.sp = pi(q.sp), q.cur = pi(q.cur), q.calls = pi(q.calls);
        target = (uint32_t)pi((int)target);
        // its stack (<= RT_QSTACK entries), through registers: read everything, then write
        sub = lane & 15;
        const int wq = (int)(threadIdx.x >> 6) * 16;  // the wave's first quad in the block
        uint32_t* qr = stk.r - (threadIdx.x >> 2) + wq;  // word of the wave's quad 0, depth 0
        float* qk = stk.k - (threadIdx.x >> 2) + wq;
        const int sq = src >> 2;
        uint32_t r0 = 0, r1 = 0;
        float k0 = 0.0f, k1 = 0.0f;
        if (ract && sub < q.sp) r0 = qr[sub * 64 + sq], k0 = qk[sub * 64 + sq];
        if (ract && sub + 16 < q.sp) r1 = qr[(sub + 16) * 64 + sq], k1 = qk[(sub + 16) * 64 + sq];
        RT_DRAIN_FENCE();
        RowInQuadStack rs{qr + 4 * row, qk + 4 * row};
        if (ract && sub < q.sp) rs.set(sub, r0, k0);
        if (ract && sub + 16 < q.sp) rs.set(sub + 16, r1, k1);
        RT_DRAIN_FENCE();
        active = ract;
#if RT_DRAIN_RESTART == 1  // (study build: the row walk restarts at the root, the quad's stack dropped)
        q.sp = 0;
        if (q.cur != 0x7fffffff) q.cur = 0;
#elif RT_DRAIN_RESTART == 2  // (study build: a new walk of the same ray, nothing of the quad's kept)
        if (ract) rtk::qstate_begin<ANY>(q, q.o, q.d, sub, nullptr);
#elif RT_DRAIN_RESTART == 3  // (study build: the ray's box-test form recomputed from o and d)
        q.rb = rtk::rayb_setup(q.o, q.d);
#elif RT_DRAIN_RESTART == 4  // (study build: the walk's hit record reset; the walk goes on from its stack)
        q.h.t = __builtin_inff(), q.h.t2 = __builtin_inff(), q.h.k = ANY ? 0 : -1, q.h.leaf = -1;
        q.h.prim = 0x7fffffff, q.h.tie = false, q.h.ovf = false;
        q.sp = 0;
        if (q.cur != 0x7fffffff) q.cur = 0;
#endif
        while (__any(active)) {
            if (STATS) {
                if (active && sub == 0) ps->c[RT_STAT_DRAIN_VISITS]++;
                if (lane == 0) ps->c[RT_STAT_DRAIN_SLOTS] += 4;
            }
            if (active) {
                const int res = rtk::row_visit<ANY, RT_VISIT_DESCEND, BRUTE>(S, q, rs, sub, ps);
                q.calls += 2;
                if (res != 0) {
                    active = false;
                    finish(res, 16);
                }
            }
        }
    }
}

// BRUTE (rt_quad.h): RT_BRUTE_OFF and RT_BRUTE_ON are answers only for a scene of that kind; the
// kernel does not check it. A launch site either dispatches on W.S.brute (run_wave) or uses
// RT_BRUTE_SCENE, which reads it.
template <bool STATS, bool PAIR = true, int G = 4, int BRUTE = RT_BRUTE_SCENE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_TRACE_OCC, 8))) void k_trace(rtk::WaveView W, int par, unsigned long long* stats)
{
    __shared__ uint32_t s_lds[RT_LDS_WORDS * 256];
    __shared__ int s_pre[RT_NSEG + 1];
    __shared__ float4_ s_qbuf[RT_TRACE_PREFETCH ? 4 : 1][64];  // per wave: the next 16 stream records (queue_prefetch)
    __shared__ int s_qkind[RT_TRACE_PREFETCH ? 4 : 1][16];
    const QPrefetch pf{s_qbuf[RT_TRACE_PREFETCH ? threadIdx.x >> 6 : 0], s_qkind[RT_TRACE_PREFETCH ? threadIdx.x >> 6 : 0]};
    int32_t* cnt = W.counters;
    if (blockIdx.x == 0) {  // filled by k_step(i) next
        for (int j = threadIdx.x; j < (rtk::RK_COUNT + 1) * RT_QSHARDS; j += blockDim.x)
            cnt[j < rtk::RK_COUNT * RT_QSHARDS ? qc_at(par ^ 1, j / RT_QSHARDS, j % RT_QSHARDS)
                                                : ac_at(par ^ 1, j - rtk::RK_COUNT * RT_QSHARDS)] = 0;
        for (int j = threadIdx.x; j < rtk::RK_COUNT * RT_HSHARDS; j += blockDim.x)
            cnt[hc_at(par ^ 1, j / RT_HSHARDS, j % RT_HSHARDS)] = 0;
        if (threadIdx.x == 0) {
            cnt[C_PARKC0 + par] = cnt[C_PARKA0 + par] = 0;
            cnt[C_TK_EXACT_C] = cnt[C_TK_EXACT_A] = 0;
        }
    }
    // release the paths whose exact walks k_step(i - 1) finished
    {
        const int nd = cnt[C_DONE0 + (par ^ 1)];
        for (int j = (int)(blockIdx.x * blockDim.x + threadIdx.x); j < nd; j += (int)(gridDim.x * blockDim.x))
            atomicSub(&W.r_park[W.done[par ^ 1][j]], 1);
    }
    rtk::Stats st;
    if (STATS)
        for (int i = 0; i < RT_STAT_COUNT; i++) st.c[i] = 0;
    rtk::Stats* ps = STATS ? &st : nullptr;
    const int b = (int)blockIdx.x;

    const RtSceneView S = W.S;
    // fast roles: a quad of lanes per query (rt_quad.h), or a row of 16 (rt_row.h)
    // queue segments in stream order (seg_id: each role's heavy class first): prefix table in LDS
    shard_prefix(cnt, RT_NSEG, [&](int j) { return seg_counter(par, j); }, s_pre);
    // without occlusion walks (analytic spheres) every kind is a closest-hit query
    const int c0 = 0, a0 = s_pre[RT_SEG_AH];
    const int nc = (W.any_rays ? a0 : s_pre[RT_SEG_END]) - c0;
    const int na = W.any_rays ? s_pre[RT_SEG_END] - a0 : 0;
    if (STATS && W.iterq && b == 0 && threadIdx.x == 0 && W.iter < RT_MAX_TIMED_ITERS) W.iterq[2 * W.iter] = nc + na;
    const int fb0 = 0, nbf = (int)gridDim.x;
    const int nbc = split_blocks(nbf, nc, na);
    const bool closest = b - fb0 < nbc;
    const int rb = closest ? b - fb0 : b - fb0 - nbc;                       // block index within the role
    const int rnb = closest ? nbc : nbf - nbc;                              // blocks of the role
    const int wg = rb * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);  // wave index within the role
    const int wn = rnb * (int)(blockDim.x >> 6);
    const int total = closest ? nc : na;
    int32_t* fbn = cnt + (closest ? C_FBC0 : C_FBA0) + par;  // walked exactly by k_step(i)
    rtk::RayRec* fbl = closest ? W.fb_c[par] : W.fb_a[par];
    // The wave's queries are a stream (its 16-query chunks base = wg*16 + c*wn*16 in turn):
    // each quad walks one, one trip per loop (rt_quad.h quad_visit), and as soon as
    // RT_TRACE_REFILL quads are idle they all take the next queries, so a long walk holds
    // up its own quad, not the wave's next 15 queries.
    if constexpr (G == 4) {
        rtk::QuadStack<RT_QSTACK, 64> stk{s_lds + (threadIdx.x >> 2), (float*)s_lds + RT_QSTACK * 64 + (threadIdx.x >> 2)};
        if (closest)
            trace_stream<false, STATS, PAIR, 4, BRUTE>(W, S, stk, s_pre, c0, total, wg, wn, fbn, fbl, ps, pf);
        else
            trace_stream<true, STATS, PAIR, 4, BRUTE>(W, S, stk, s_pre, a0, total, wg, wn, fbn, fbl, ps, pf);
    } else {
        static_assert(2 * RT_RSTACK * 16 <= RT_LDS_WORDS * 256, "row stacks fit k_trace's LDS");
        rtk::QuadStack<RT_RSTACK, 16> stk{s_lds + (threadIdx.x >> 4), (float*)s_lds + RT_RSTACK * 16 + (threadIdx.x >> 4)};
        if (closest)
            trace_stream<false, STATS, PAIR, 16, BRUTE>(W, S, stk, s_pre, c0, total, wg, wn, fbn, fbl, ps, pf);
        else
            trace_stream<true, STATS, PAIR, 16, BRUTE>(W, S, stk, s_pre, a0, total, wg, wn, fbn, fbl, ps, pf);
    }
    flush_stats<STATS>(st, stats);
}

// ------------------------------------------------------------- tail kernel
// When few paths are left (the last pixels of a frame are the ones whose
// samples bounce the most), an iteration costs its slowest query plus its
// slowest step no matter how few paths it carries, and a pixel's 64 x
// (bounces + 1) steps are a chain: the frame end is set by that chain. The
// tail kernel takes the remaining paths in one launch and lets each wave run
// its own: up to W.tail_paths paths per wave (lanes 0..P-1), step them, trace
// the rays they emitted from an LDS list with quads, repeat; a wave whose path
// finishes takes the next one from the live list. No grid-wide step, no
// launches: each path runs at its own pace.
// Entry condition (run_wave): no query is parked or waiting for the exact
// walk, so every path is ready to step; a query the quad walk cannot answer
// is answered here by the exact walk, inline, by lane 0 of its quad.
#define RT_TAIL_MAXP 16  // paths per wave at most (RK_COUNT rays each per list)
#ifndef RT_TAIL_EMIT_LDS
#define RT_TAIL_EMIT_LDS RT_STEP_EMIT_LDS
#endif
#if RT_TAIL_EMIT_LDS
// k_tail: a path's emitted rays stay in the wave's LDS columns (EmitLds<RT_TAIL_MAXP>, lane j
// of the wave's paths in column j); the lists hold (j << 3 | kind) (l0: closest-hit kinds,
// l1: occlusion)
using TailEmit = rtk::EmitLds<RT_TAIL_MAXP>;
__device__ __forceinline__ void tail_lists(const TailEmit& e, int last_kind, uint8_t* l0, uint8_t* l1, int* nl)
{
    const int lane = lane_id();
    nl[0] = nl[1] = 0;
#pragma unroll
    for (int k = 0; k < rtk::RK_COUNT; k++) {
        const bool want = (e.mask >> k) & 1u;
        const unsigned long long b = __ballot(want);
        const int l = k <= last_kind ? 0 : 1;
        if (want) (l ? l1 : l0)[nl[l] + __popcll(b & ((1ull << lane) - 1ull))] = (uint8_t)((lane << 3) | k);
        nl[l] += __popcll(b);
    }
}
// k_tail's path step (lanes with my >= 0) and list append, out of line (its registers apart
// from the walk loop's; inlined, the tail loop spilled across every step: cfg2 811 -> 828
// Msamples/s, cfg4 8-way shard 436 -> 403 ms, r02): bit 0 the lane's path stays in
// flight, bits 1-10 / 11- the closest / occlusion list lengths.
__device__ __noinline__ int tail_step(const rtk::WaveView& W, int my, int last_kind, float* cols, uint8_t* l0, uint8_t* l1,
                                      rtk::Stats* ps)
{
    TailEmit e;
    e.s = cols + (lane_id() & (RT_TAIL_MAXP - 1));  // (lanes >= W.tail_paths never step)
    e.mask = 0;
    e.active = false;
    e.heavy = false;
    if (my >= 0) rtk::path_step<true>(W, my, e, ps);
    int nl[2];
    tail_lists(e, last_kind, l0, l1, nl);
    return (e.active ? 1 : 0) | (nl[0] << 1) | (nl[1] << 11);
}
#else
// k_tail: a path's emitted rays -> the wave's LDS lists (l0: closest-hit kinds, l1: occlusion)
__device__ __forceinline__ void tail_lists(const rtk::Emit& e, int slot, int last_kind, rtk::RayRec* l0, rtk::RayRec* l1,
                                           int* nl)
{
    const int lane = lane_id();
    nl[0] = nl[1] = 0;
#pragma unroll
    for (int k = 0; k < rtk::RK_COUNT; k++) {
        const bool want = (e.mask >> k) & 1u;
        const unsigned long long b = __ballot(want);
        const int l = k <= last_kind ? 0 : 1;
        if (want) {
            const int pos = nl[l] + __popcll(b & ((1ull << lane) - 1ull));
            (l ? l1 : l0)[pos] = e.rec(k, slot, rt_asfloat(((uint32_t)slot << 3) | (uint32_t)k));
        }
        nl[l] += __popcll(b);
    }
}
// (as above, the rays in registers and the lists of whole records)
__device__ __noinline__ int tail_step(const rtk::WaveView& W, int my, int last_kind, rtk::RayRec* l0, rtk::RayRec* l1,
                                      rtk::Stats* ps)
{
    rtk::Emit e;
    e.mask = 0;
    e.active = false;
    e.heavy = false;
    if (my >= 0) rtk::path_step<true>(W, my, e, ps);
    int nl[2];
    tail_lists(e, my, last_kind, l0, l1, nl);
    return (e.active ? 1 : 0) | (nl[0] << 1) | (nl[1] << 11);
}
#endif
// k_tail's inline exact walk (a query the quad walk cannot settle: ~1e-6 of them), kept
// out of line so that its registers do not add to the tail loop's: inlined, k_tail
// needed 468 VGPR spill slots at its 168-VGPR budget, out of line ~190.
template <class XS>
__device__ __noinline__ void tail_exact(const rtk::WaveView& W, int l, uint32_t target, rtk::V3 o, rtk::V3 d, XS& xs,
                                        rtk::Stats* ps)
{
    if (l == 0) {
        rtk::TravC T;
        if (rtk::travc_begin(W.S, T, o, d, ps))
            while (rtk::travc_step(W.S, T, xs, ps)) {
            }
        rtk::finish_closest(W, target, T.o, T.d, T.best_t, T.best_k);
    } else {
        rtk::TravA T;
        if (rtk::trava_begin(W.S, T, o, d, ps))
            while (rtk::trava_step(W.S, T, xs, ps)) {
            }
        rtk::finish_any(W, target, T.hit);  // (begin leaves the brute-force answer in T.hit)
    }
}
#ifndef RT_TAIL_DESCEND
#define RT_TAIL_DESCEND RT_VISIT_DESCEND  // inner-node trips per quad_visit call in k_tail
#endif
#ifndef RT_TAIL_OCC
#define RT_TAIL_OCC 3    // k_tail waves per SIMD (2: no spills but half the paths per launch; 3 measured faster)
#endif
// FAST: the fast lane's launch, one kernel over every lane's handed-over paths: blocks
// [fparts[l], fparts[l + 1]) step lane l's (fviews[l]: its fast list as shard 0 of its own
// counters, its own spill area).
template <bool STATS, bool PAIR, int G, bool FAST>
__device__ __forceinline__ void tail_body(const rtk::WaveView& W, int par, unsigned long long* stats, int blk)
{
#if RT_TAIL_EMIT_LDS
    __shared__ float s_em[4][6 * rtk::RK_COUNT * RT_TAIL_MAXP];        // per wave: its paths' rays (TailEmit columns)
    __shared__ uint8_t s_q[4][2][RT_TAIL_MAXP * rtk::RK_COUNT];        // per wave: closest list, occlusion list
    __shared__ int s_my[4][RT_TAIL_MAXP];                              // per wave: the slot of column j
#else
    __shared__ rtk::RayRec s_q[4][2][RT_TAIL_MAXP * rtk::RK_COUNT];  // per wave: closest list, occlusion list
#endif
    __shared__ uint32_t s_stk[2 * RT_QSTACK * 64];
    __shared__ int s_pre[RT_QSHARDS + 1];
    rtlibm::lds_tables_init();
    rtk::lds_shade_init(W.S);  // (the env-map row search and a small material table from LDS)
    int32_t* cnt = W.counters;
    shard_prefix(cnt, RT_QSHARDS, [&](int j) { return ac_at(par, j); }, s_pre);
    const int n = FAST ? min(s_pre[RT_QSHARDS], W.fast_cap) : s_pre[RT_QSHARDS];  // (fast lane: its list)
    const RtSceneView S = W.S;
    rtk::Stats st;
    if (STATS)
        for (int i = 0; i < RT_STAT_COUNT; i++) st.c[i] = 0;
    rtk::Stats* ps = STATS ? &st : nullptr;
    // G lanes per query: quads (4-wide BVH) or rows (16-wide BVH, rt_row.h), each with its LDS stack
    static_assert(G == 4 || G == 16, "quads or rows");
    constexpr int SCAP = G == 4 ? RT_QSTACK : RT_RSTACK, GPB = 256 / G;
    static_assert(2 * SCAP * GPB <= 2 * RT_QSTACK * 64, "group stacks fit k_tail's LDS");
    const int wv = (int)(threadIdx.x >> 6), lane = lane_id(), sub = lane & (G - 1), qd = (int)(threadIdx.x / G);
    using STK = rtk::QuadStack<SCAP, GPB>;
    STK stk{s_stk + qd, (float*)s_stk + SCAP * GPB + qd};
    const size_t gl = (size_t)blk * blockDim.x + threadIdx.x;
    rtk::SpillStack<STK> xs{stk, W.spill_r + gl * RT_STACK_CAP, W.spill_k + gl * RT_STACK_CAP};
    const int P = W.tail_paths;
    const int last_kind = W.any_rays ? rtk::RK_CAM : rtk::RK_BENV;
    int my = -1;
    bool drained = false;
    int rounds = 0;  // (RT_ITER_LOG: the longest pool loop of the launch)
    long long tk_step = 0, tk_walk = 0;  // (RT_ITER_LOG: 100 MHz ticks in path_step / in the walks)
    long long tk_solo = 0;               // (RT_ITER_LOG: ... in walk trips with one group walking)
    int trips = 0, solo_trips = 0;
    const bool probe = STATS && W.iterq && W.iter + 1 < RT_MAX_TIMED_ITERS;
    for (;;) {
        // refill the wave's pool from the live list
        const bool need = lane < P && my < 0;
        const unsigned long long bneed = __ballot(need);
        if (bneed && !drained) {
            const int nneed = __popcll(bneed);
            int base = 0;
            if (lane == 0) base = atomicAdd(cnt + C_TK_TAIL, nneed);
            base = __shfl(base, 0);
            if (base + nneed >= n) drained = true;
            const int idx = base + __popcll(bneed & ((1ull << lane) - 1ull));
            if (need && idx < n) {
                const int sh = shard_find8<RT_QSHARDS>(s_pre, idx);
                my = W.act_in[(size_t)sh * W.seg_cap + (idx - s_pre[sh])];
                if (FAST) W.r_park[my] = 0;  // (k_hand's mark)
            }
        }
        if (!__any(my >= 0)) break;
        rounds++;
        // step; the emitted rays -> the wave's LDS lists
        const long long t0 = probe ? wall_clock64() : 0;
        int nl[2];
        {
#if RT_TAIL_EMIT_LDS
            if (lane < RT_TAIL_MAXP) s_my[wv][lane] = my;
            const int r = tail_step(W, my, last_kind, s_em[wv], s_q[wv][0], s_q[wv][1], ps);
#else
            const int r = tail_step(W, my, last_kind, s_q[wv][0], s_q[wv][1], ps);
#endif
            if (!(r & 1)) my = -1;
            nl[0] = (r >> 1) & 0x3ff;
            nl[1] = r >> 11;
        }
        long long t1 = 0;
        if (probe) {
            t1 = wall_clock64();
            tk_step += __shfl(t1, 0) - __shfl(t0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the lists are read by other lanes
        __builtin_amdgcn_wave_barrier();
        // trace: both lists in one index space, streamed over the wave's 16 quads (an idle
        // quad takes the next query at once), each quad walking its own kind a few trips
        // per call (rt_quad.h quad_visit): a step waits for its slowest query, not for
        // the slowest of every 16-query pass
        const int nq = nl[0] + nl[1];
        int next = 0;  // the next query of the lists (uniform)
        bool act = false;
        int l = 0;
        uint32_t target = 0;
        rtk::QState q;
        for (;;) {
            bool exact = false;
            const unsigned long long bidle = __ballot(!act && sub == 0);
            if (next < nq) {
                const int qi = next + __popcll(bidle & ((1ull << (lane & ~(G - 1))) - 1ull));  // this group's query
                if (!act && qi < nq) {
                    l = qi < nl[0] ? 0 : 1;
#if RT_TAIL_EMIT_LDS
                    const int ent = s_q[wv][l][l ? qi - nl[0] : qi], j = ent >> 3, kind = ent & 7;
                    TailEmit ce;
                    ce.s = s_em[wv] + j;
                    rtk::RayRec r;
                    r.o = rtk::f4(ce.o(kind), 0.0f);
                    r.d = rtk::f4(ce.d(kind), 0.0f);
                    target = ((uint32_t)s_my[wv][j] << 3) | (uint32_t)kind;
#else
                    const rtk::RayRec r = s_q[wv][l][l ? qi - nl[0] : qi];
                    target = rt_asuint(r.d.w);
#endif
                    q.o = rtk::v3of(r.o);
                    q.d = rtk::v3of(r.d);
                    if (forced_fallback(W, r.o, r.d)) {
                        exact = true;
                    } else {
                        act = l ? rtk::qstate_begin<true>(q, q.o, q.d, sub, ps) : rtk::qstate_begin<false>(q, q.o, q.d, sub, ps);
                        if (STATS) q.calls = 0;
                        if (!act && sub == 0) {  // (a NaN ray: no hit)
                            if (l == 0)
                                rtk::finish_closest(W, target, q.o, q.d, -1.0f, -1);
                            else
                                rtk::finish_any(W, target, false);
                        }
                    }
                }
                next = min(nq, next + __popcll(bidle));
            }
            long long ts = 0;
            bool solo = false;
            if (probe) {
                ts = wall_clock64();
                solo = __popcll(__ballot(act && sub == 0)) == 1;
            }
            if (act) {
                int res;
                if constexpr (G == 4)
                    res = l ? rtk::quad_visit<true, RT_TAIL_DESCEND, PAIR>(S, q, stk, sub, ps)
                            : rtk::quad_visit<false, RT_TAIL_DESCEND>(S, q, stk, sub, ps);
                else
                    res = l ? rtk::row_visit<true, RT_TAIL_DESCEND>(S, q, stk, sub, ps)
                            : rtk::row_visit<false, RT_TAIL_DESCEND>(S, q, stk, sub, ps);
                if (STATS) q.calls += G == 4 ? 1 : 2;
                if (res != 0) {
                    act = false;
                    float t = 0.0f;
                    int k = 0;
                    const bool ok = res > 0 && (l == 1 || rtk::quad_closest_answer(S, q, sub & 3, t, k,
                                                                                    G == 4 || sub == 0 ? ps : nullptr));
                    if (STATS && W.wlog && sub == 0 && q.calls >= W.wlog_min)
                        walk_log(W, q.o, q.d, target, q.calls, !ok ? -2.0f : l ? (float)(q.h.k == 1) : t, k, 2);
                    if (ok && sub == 0) {
                        if (l == 0)
                            rtk::finish_closest(W, target, q.o, q.d, t, k);
                        else
                            rtk::finish_any(W, target, q.h.k == 1);
                    }
                    exact = !ok;
                }
            }
            if (exact && sub == 0) {  // the exact octree walk, to completion
                if (STATS) st.c[RT_STAT_FALLBACK]++;
                xs.f = stk;
                tail_exact(W, l, target, q.o, q.d, xs, ps);
            }
            if (probe) {
                const long long te = wall_clock64();
                trips++;
                if (solo) {
                    solo_trips++;
                    tk_solo += __shfl(te, 0) - __shfl(ts, 0);
                }
            }
            if (next >= nq && !__any(act)) break;
        }
        if (probe) {
            const long long t2 = wall_clock64();
            tk_walk += __shfl(t2, 0) - __shfl(t1, 0);
        }
    }
    if (STATS && W.iterq && lane == 0 && W.iter < RT_MAX_TIMED_ITERS) atomicMax(W.iterq + 2 * W.iter + 1, rounds);
    if (probe && lane == 0) {
        atomicAdd(W.iterq + 2 * W.iter + 2, (int)(tk_step >> 4));
        atomicAdd(W.iterq + 2 * W.iter + 3, (int)(tk_walk >> 4));
        int32_t* q2 = W.iterq + 2 * RT_MAX_TIMED_ITERS + 4 * (W.iter + 1);  // (the tail row's last columns)
        atomicAdd(q2, (int)(tk_solo >> 4));
        atomicAdd(q2 + 1, trips);
        atomicAdd(q2 + 2, solo_trips);
    }
    flush_stats<STATS>(st, stats);
    flush_stats<STATS>(st, stats + RT_STAT_COUNT);  // (the tail kernel's share, for per-kernel byte counts)
}
template <bool STATS, bool PAIR = true, int G = 4>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_TAIL_OCC, RT_TAIL_OCC))) void k_tail(
    rtk::WaveView W, int par, unsigned long long* stats)
{
    tail_body<STATS, PAIR, G, false>(W, par, stats, (int)blockIdx.x);
}
template <bool STATS, bool PAIR = true, int G = 4>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_TAIL_OCC, RT_TAIL_OCC))) void k_tail_fast(
    const rtk::WaveView* __restrict__ fviews, int4 fparts, unsigned long long* stats)
{
    const int b = (int)blockIdx.x;
    const int fl = (b >= fparts.y) + (b >= fparts.z) + (b >= fparts.w);
    const int b0 = fl == 0 ? 0 : fl == 1 ? fparts.y : fl == 2 ? fparts.z : fparts.w;
    tail_body<STATS, PAIR, G, true>(fviews[fl], 0, stats, b - b0);
}

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
        default: r = rtk::slab_div(x, 1.0 / (double)in2[i]); break;  // the slab quotient
    }
    out[i] = r;
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

// ------------------------------------------------------------- wave memory
}  // namespace

size_t rt_wave_counter_bytes() { return C_COUNT * sizeof(int32_t); }
size_t rt_wave_readback_bytes() { return RT_QSHARDS * RT_CSTRIDE * 4 + 64; }

namespace {
const int threads = 256;
const WaveKnobs knobs{RT_TRACE_OCC, RT_TAIL_OCC, RT_HEAVY_CALLS, RT_TAIL_ROWS, RT_DRAIN_ROWS, RT_TAIL_MAXP, RT_QSHARDS};

// One launch helper per kernel family: (SEQ, S, brute / rows) -> the instantiation.
// SEQ: counter renders with unpaired occlusion walks; S: counter renders; brute: USE_BVH 0
// scenes (the walks that keep the triangles' original indices); rows: k_tail walks by rows.
#define RT_LAUNCH(K) hipLaunchKernelGGL(K, g, dim3(threads), 0, s, W, par, stats)
void launch_k_trace(bool SEQ, bool S, bool brute, dim3 g, hipStream_t s, const rtk::WaveView& W, int par,
                    unsigned long long* stats)
{
    if (SEQ) RT_LAUNCH((k_trace<true, false>));
    else if (S) RT_LAUNCH((k_trace<true, true>));
    else if (brute) RT_LAUNCH((k_trace<false, true, 4, RT_BRUTE_ON>));
    else RT_LAUNCH((k_trace<false, true, 4, RT_BRUTE_OFF>));
}
void launch_k_tail_fast(bool SEQ, bool S, dim3 g, hipStream_t s, const rtk::WaveView* fv, int4 parts,
                        unsigned long long* stats)
{
    if (SEQ) hipLaunchKernelGGL((k_tail_fast<true, false, 4>), g, dim3(threads), 0, s, fv, parts, stats);
    else if (S) hipLaunchKernelGGL((k_tail_fast<true, true, 16>), g, dim3(threads), 0, s, fv, parts, stats);
    else hipLaunchKernelGGL((k_tail_fast<false, true, 16>), g, dim3(threads), 0, s, fv, parts, stats);
}
void launch_k_step(bool S, dim3 g, hipStream_t s, const rtk::WaveView& W, int par, unsigned long long* stats)
{
    if (W.prog && S) RT_LAUNCH((k_step<true, true>));  // (a progressive pass)
    else if (W.prog) RT_LAUNCH((k_step<false, true>));
    else if (S) RT_LAUNCH(k_step<true>);
    else RT_LAUNCH(k_step<false>);
}
void launch_k_tail(bool SEQ, bool S, bool rows, dim3 g, hipStream_t s, const rtk::WaveView& W, int par,
                   unsigned long long* stats)
{
    if (SEQ) RT_LAUNCH((k_tail<true, false, 4>));
    else if (S) RT_LAUNCH((rows ? k_tail<true, true, 16> : k_tail<true, true, 4>));
    else RT_LAUNCH((rows ? k_tail<false, true, 16> : k_tail<false, true, 4>));
}
#undef RT_LAUNCH
// The readback a lane waits for: none, the live count (read_live), or the fallback counts
// (the tail entry check of issue).
enum class Await { None, Live, Fallbacks };
// A lane's share of the fast lane, in order of life:
//   Waiting -> HistPending   process: the lane reached fast_iter; k_hist's histogram is on its way back
//   HistPending -> HandNext  fast_threshold: the histogram has landed, the threshold is known
//   HandNext -> Handed       launch_step: k_hand ran before this k_step
//   Waiting / HistPending -> NoShare   process: the lane is done or enters its tail first
// (NoShare from the start without a fast lane). fast_launch runs once no lane is before Handed.
enum class Fast { Waiting, HistPending, HandNext, Handed, NoShare };

// One wavefront run over a subset of the launch's pixels (a "lane"): its own
// path slots, queues, counters and stream. run_wave drives RT_LANES lanes on
// as many streams (row j of the launch -> lane j % lanes) so that one lane's
// k_step and the tails of its launches overlap another lane's k_trace.
struct WaveLane {
    rtk::WaveView W{};
    int32_t* lists[2] = {nullptr, nullptr};
    int32_t* cnt = nullptr;
    int32_t* h = nullptr;  // pinned readback: ACT shard counts, then 8 FB / PARK counters
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    int n = 0, it = 0, tail_iter = -1;
    long live = 0;  // live paths at the last readback (an upper bound: paths only finish)
    bool done = false, tail_next = false;
    Await await = Await::None;
    Fast fast = Fast::NoShare;
    int fast_thr = 0, fast_n = 0;  // ... samples-done threshold, paths at most
    Event (*tev)[RT_MAX_TIMED_ITERS] = nullptr;  // [3][RT_MAX_TIMED_ITERS]
};

// One call of run_wave: the plan, the lanes and the launches on their streams.
struct WaveRun {
    rt_context* c;
    Backend* b;
    int w, h, spp, bounces;
    const rtk::PixSrc& src;
    int n;
    float4_* fb;
    hipStream_t s;
    const WavePass* pass;  // a progressive pass: samples pass->first .. spp - 1, paused into pass->state (else null)
    bool linear;           // no tone-map pass after the last step (rt_render_linear)
    int dev_cus = 256;
    WavePlan P{};
    WaveLane L[RT_MAX_LANES];
    bool S = false, SEQ = false, wlog = false;
    unsigned long long* stats = nullptr;
    const char* iter_log = nullptr;  // per-iteration log of lane 0: counts (stats renders) / ms (timed)
    hipStream_t fstream = nullptr;
    bool fast_launched = false, fast_ran = false;
    long max_iters = 0;
    static constexpr size_t act_bytes = RT_QSHARDS * RT_CSTRIDE * 4;

    int begin();
    int init_lane(int l);
    int launch_trace(WaveLane& La);
    int fast_launch();
    int fast_threshold(WaveLane& La);
    int launch_step(WaveLane& La);
    int launch_tail(WaveLane& La, int par);
    int read_live(WaveLane& La);
    int issue(WaveLane& La);
    int process(WaveLane& La);
    int start_hist(WaveLane& La);
    int poll();
    int finish();
    int report();
    int lane_of(const WaveLane& La) const { return (int)(&La - L); }
    // grids sized by the last known live count: k_step one slot per thread; k_trace up to
    // five queries per path, a quad each, over two grid-fills, never fewer blocks than the
    // exact-walk roles can claim (dev_cus * 4) plus room for the fast roles
    // (k_step: at least 3 blocks, one per exact-walk role and one for the path step, so a
    // small live count with fallbacks or parked walks pending still steps its paths)
    int step_blocks_of(const WaveLane& La) const
    {
        return (int)std::max(3l, std::min((La.live + threads - 1) / threads, (long)dev_cus * RT_STEP_FILL));
    }
    int trace_blocks_of(const WaveLane& La) const
    {
        const long want = (20 * La.live + 2 * threads - 1) / (2 * threads);
        return (int)std::min((long)P.trace_blocks, std::max(want, (long)dev_cus * 4 + 64));
    }
};

int WaveRun::begin()
{
    // every render of a context reuses its lanes' slots and counters: the previous render
    // (whose tail kernel may still run, on another stream) must finish first
    if (b->done_recorded) HIPCHK(c, hipStreamWaitEvent(s, b->ev_done, 0));
    (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, b->device);
    const RtDiag& dg = c->diag;
    S = c->stats_enabled;
    SEQ = S && c->stats_seq;  // (counter renders with unpaired occlusion walks: rt_set_stats(ctx, 2))
    stats = (unsigned long long*)b->stats.p;
    if (S) HIPCHK(c, hipMemsetAsync(b->stats.p, 0, b->stats.bytes, s));
    iter_log = dg.iter_log.empty() ? nullptr : dg.iter_log.c_str();
    wlog = S && dg.wlog_cap > 0 && b->index == 0;
    if (wlog) {
        if (int r = ensure(c, b->wlog, 256 + (size_t)dg.wlog_cap * 48)) return r;
        HIPCHK(c, hipMemsetAsync(b->wlog.p, 0, 256, s));
    }
    if (!b->handovers.p) {
        if (int r = ensure(c, b->handovers, 8)) return r;
        HIPCHK(c, hipMemsetAsync(b->handovers.p, 0, 8, s));
    }
    if (S && iter_log) {
        if (int r = ensure(c, b->iterq, RT_MAX_TIMED_ITERS * 24)) return r;
        HIPCHK(c, hipMemsetAsync(b->iterq.p, 0, RT_MAX_TIMED_ITERS * 24, s));
    }
    const int rows = src.xy ? 0 : n / src.W;
    P = wave_plan(c->sched, knobs, WaveSource{src.xy != nullptr, src.W, src.off, src.stride}, n, rows, spp, dev_cus, SEQ,
                  b->lanes, b->budget);
    const int nl = P.lanes;
    if (P.fast_k > 0 && nl == RT_MAX_LANES && !b->fs) HIPCHK(c, hipStreamCreateWithFlags(&b->fs.h, hipStreamNonBlocking));
    fstream = P.fast_k > 0 ? (hipStream_t)(nl < RT_MAX_LANES ? b->ls[nl] : b->fs) : nullptr;
    if (nl > 1) {
        HIPCHK(c, hipEventRecord(b->ev_fork, s));
        for (int l = 1; l < nl; l++) HIPCHK(c, hipStreamWaitEvent(b->ls[l], b->ev_fork, 0));
    }
    for (int l = 0; l < nl; l++)
        if (int r = init_lane(l)) return r;
    if (dg.verbose)
        fprintf(stderr, "[rt] run_wave n=%d lanes=%d cus=%d trace_blocks=%d budget=%d\n", n, nl, dev_cus, P.trace_blocks,
                L[0].W.budget);
    // A sample takes at most bounces + 1 iterations without fallbacks; an
    // exact walk delays its path by at least one iteration. The bound only
    // guards against a runaway loop.
    max_iters = 64l * spp * ((long)bounces + 1) + 4096;
    for (int l = 0; l < nl; l++)
        if (int r = issue(L[l])) return r;
    return RT_OK;
}

// The lane's buffers carved, its view filled, its counters zeroed and k_init on its stream.
int WaveRun::init_lane(int l)
{
    WaveLane& La = L[l];
    const LanePlan& lp = P.lane[l];
    const RtDiag& dg = c->diag;
    rtk::PixSrc ls = src;
    if (src.xy) ls.xy = src.xy + 2 * (size_t)lp.first;
    ls.off = lp.off;
    ls.stride = lp.stride;
    La.n = lp.n;
    La.live = La.n;
    La.s = l == 0 ? s : (hipStream_t)b->ls[l];
    La.cnt = (int32_t*)b->counters[l].p;
    La.h = b->h_act[l];
    La.ev = b->ev_lane[l];
    La.tev = b->tev[l];
    rtk::WaveView& W = La.W;
    W.park_cap = 1 << 16;
    W.heavy_calls = P.heavy_calls;
    W.spec_cam = P.spec_cam;
    W.shards = RT_QSHARDS;
    W.seg_cap = lp.seg_cap;
    W.spill_lanes = dev_cus * 4 * threads;  // exact walks: up to dev_cus * 2 blocks per role
    W.fspill_lanes = 0;
    const size_t need = rtk::wave_carve(nullptr, (size_t)La.n, W);
    if (int r = ensure(c, b->wave[l], need)) return r;
    rtk::wave_carve((char*)b->wave[l].p, (size_t)La.n, W);
    W.S = b->view;
    rt_view_near(c, W.S);  // (rt_test_schedule may have changed it since the upload)
    W.cam = c->cam;
    W.src = ls;
    W.W = w;
    W.H = h;
    W.spp = spp;
    W.bounces = bounces;
    W.prog = pass ? pass->state + lp.first : nullptr;
    W.first = pass ? pass->first : 0;
    W.seed_spp = pass ? pass->seed_spp : spp;
    rtk::set_view_consts(W);
    W.n_slots = La.n;
    W.bl_rays = b->bl_rays;
    W.any_rays = b->any_rays;
    W.fb = fb + lp.first;
    W.fb_rs = lp.fb_rs;
    W.budget = P.budget;
    W.counters = La.cnt;
    W.tail_paths = P.tail_p;
    W.drain_rows = P.drain_rows;
    W.force_fb = c->sched.force_fallback;  // (test stressor, rt_test_schedule)
    W.fast_cap = 0;
    La.fast = P.fast_k > 0 ? Fast::Waiting : Fast::NoShare;
    La.fast_n = lp.fast_n;
    if (P.fast_k > 0) {  // the fast lane's buffers and events (first use)
        if (int r = ensure(c, b->fast[l], (size_t)(La.fast_n + 1) * 4)) return r;
        if (int r = ensure(c, b->fcnt[l], C_COUNT * sizeof(int32_t))) return r;
        if (int r = ensure(c, b->fhist[l], (RT_FAST_MAX_SPP + 1) * 4)) return r;
        if (int r = ensure(c, b->fspill[l], (size_t)((La.fast_n + 3) / 4) * threads * RT_STACK_CAP * 8)) return r;
        if (!b->h_hist[l]) HIPCHK(c, hipHostMalloc((void**)&b->h_hist[l].h, (RT_FAST_MAX_SPP + 1) * 4, hipHostMallocDefault));
        if (!b->fev[l]) HIPCHK(c, hipEventCreateWithFlags(&b->fev[l].h, hipEventDisableTiming));
        if (!b->hev[l]) HIPCHK(c, hipEventCreateWithFlags(&b->hev[l].h, hipEventDisableTiming));
        HIPCHK(c, hipMemsetAsync(b->fcnt[l].p, 0, C_COUNT * sizeof(int32_t), La.s));
    }
    W.iterq = (S && iter_log && l == 0) ? (int32_t*)b->iterq.p : nullptr;
    W.handovers = (unsigned long long*)b->handovers.p;
    if (wlog) {
        W.wlog_n = (int32_t*)b->wlog.p;
        W.wlog = (float4_*)((char*)b->wlog.p + 256);
        W.wlog_min = dg.wlog_min;
        W.wlog_cap = dg.wlog_cap;
        W.wlog_every = dg.wlog_every;
    }
    La.lists[0] = (int32_t*)W.act_in;
    La.lists[1] = W.act_out;
    HIPCHK(c, hipMemsetAsync(La.cnt, 0, C_COUNT * sizeof(int32_t), La.s));
    HIPCHK(c, hipMemsetAsync(W.r_park, 0, (size_t)La.n * 4, La.s));
    W.act_in = La.lists[1];
    W.act_out = La.lists[0];
    if (W.first > 0)
        hipLaunchKernelGGL(k_resume, dim3((La.n + threads - 1) / threads), dim3(threads), 0, La.s, W);
    else
        hipLaunchKernelGGL(k_init, dim3((La.n + threads - 1) / threads), dim3(threads), 0, La.s, W);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

int WaveRun::launch_trace(WaveLane& La)
{
    rtk::WaveView& W = La.W;
    const int par = La.it & 1;
    W.iter = La.it;
    W.act_in = La.lists[par];
    W.act_out = La.lists[par ^ 1];
    const bool T = b->timing && La.it < RT_MAX_TIMED_ITERS;
    if (T)
        for (int k = 0; k < 3; k++)
            if (!La.tev[k][La.it]) HIPCHK(c, hipEventCreate(&La.tev[k][La.it].h));
    if (T) HIPCHK(c, hipEventRecord(La.tev[0][La.it], La.s));
    launch_k_trace(SEQ, S, W.S.brute, dim3(trace_blocks_of(La)), La.s, W, par, stats);
    if (T) HIPCHK(c, hipEventRecord(La.tev[1][La.it], La.s));
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

// the fast lane's tail kernel, once every lane has handed its share over (or has none)
int WaveRun::fast_launch()
{
    const int nl = P.lanes;
    if (P.fast_k == 0 || fast_launched) return RT_OK;
    bool any = false;
    for (int l = 0; l < nl; l++) {
        if (L[l].fast != Fast::Handed && L[l].fast != Fast::NoShare) return RT_OK;  // (a lane still to hand over)
        any = any || L[l].fast == Fast::Handed;
    }
    fast_launched = true;
    if (!any) return RT_OK;
    if (!b->h_fviews)
        HIPCHK(c, hipHostMalloc((void**)&b->h_fviews.h, sizeof(rtk::WaveView) * RT_MAX_LANES, hipHostMallocDefault));
    if (!b->fev_done) HIPCHK(c, hipEventCreateWithFlags(&b->fev_done.h, hipEventDisableTiming));
    if (b->fev_done_recorded) HIPCHK(c, hipEventSynchronize(b->fev_done));  // (the last render's copy of the views)
    if (int r = ensure(c, b->fviews, sizeof(rtk::WaveView) * RT_MAX_LANES)) return r;
    int start[RT_MAX_LANES + 1] = {}, tot = 0;
    for (int l = 0; l < RT_MAX_LANES; l++) {
        start[l] = tot;
        if (l >= nl || L[l].fast != Fast::Handed) continue;
        rtk::WaveView FW = L[l].W;
        FW.act_in = (int32_t*)b->fast[l].p;
        FW.counters = (int32_t*)b->fcnt[l].p;
        FW.fast_cap = L[l].fast_n;
        FW.tail_paths = 1;  // (one path per wave, its queries on the wave's rows)
        const int blocks = (L[l].fast_n + 3) / 4;
        FW.spill_r = (uint32_t*)b->fspill[l].p;
        FW.spill_k = (float*)((uint32_t*)b->fspill[l].p + (size_t)blocks * threads * RT_STACK_CAP);
        FW.iterq = nullptr;
        FW.spec_cam = P.spec_cam ? P.tail_spec_cam : 0;
        b->h_fviews.h[l] = FW;
        tot += blocks;
        HIPCHK(c, hipStreamWaitEvent(fstream, b->fev[l], 0));
    }
    HIPCHK(c, hipMemcpyAsync(b->fviews.p, b->h_fviews, sizeof(rtk::WaveView) * RT_MAX_LANES, hipMemcpyHostToDevice,
                             fstream));
    if (b->timing) {
        for (Event& e : b->ftev)
            if (!e) HIPCHK(c, hipEventCreate(&e.h));
        HIPCHK(c, hipEventRecord(b->ftev[0], fstream));
    }
    launch_k_tail_fast(SEQ, S, dim3(tot), fstream, (const rtk::WaveView*)b->fviews.p,
                       make_int4(start[0], start[1], start[2], start[3]), stats);
    HIPCHK(c, hipGetLastError());
    if (b->timing) HIPCHK(c, hipEventRecord(b->ftev[1], fstream));
    HIPCHK(c, hipEventRecord(b->fev_done, fstream));
    b->fev_done_recorded = fast_ran = true;
    return RT_OK;
}

// the fast lane's threshold: the samples-done count of the lane's fast_n-th slowest live
// path, from the histogram k_hist read back (polled: the host thread serving every lane
// never blocks on it; the hand-over happens at the first k_step after it has landed)
int WaveRun::fast_threshold(WaveLane& La)
{
    const int l = lane_of(La);
    const hipError_t q = hipEventQuery(b->hev[l]);
    if (q == hipErrorNotReady) return RT_OK;
    HIPCHK(c, q);
    long acc = 0;
    int thr = spp;
    for (int k = 0; k <= spp; k++)
        if ((acc += b->h_hist[l].h[k]) >= La.fast_n) {
            thr = k;
            break;
        }
    La.fast_thr = thr;
    La.fast = Fast::HandNext;
    return RT_OK;
}

int WaveRun::launch_step(WaveLane& La)
{
    const int par = La.it & 1;
    const int l = lane_of(La);
    if (La.fast == Fast::HistPending)
        if (int r = fast_threshold(La)) return r;
    const bool hand = La.fast == Fast::HandNext;
    int32_t* fl = (int32_t*)b->fast[l].p;
    if (hand) {  // this step hands the lane's slowest paths to the fast lane
        HIPCHK(c, hipMemsetAsync(fl + La.fast_n, 0, 4, La.s));
        rtk::WaveView HW = La.W;
        HW.fast_list = fl;
        HW.fast_ticket = fl + La.fast_n;
        HW.fast_cap = La.fast_n;
        HW.fast_thr = La.fast_thr;
        hipLaunchKernelGGL(k_hand, dim3((unsigned)std::min(1024l, (La.live + threads - 1) / threads)), dim3(threads), 0,
                           La.s, HW, par);
        HIPCHK(c, hipGetLastError());
    }
    launch_k_step(S, dim3(step_blocks_of(La)), La.s, La.W, par, stats);
    if (hand) {  // (its list's length as shard 0 of the fast lane's counters)
        La.fast = Fast::Handed;
        HIPCHK(c, hipMemcpyAsync((int32_t*)b->fcnt[l].p + ac_at(0, 0), fl + La.fast_n, 4, hipMemcpyDeviceToDevice, La.s));
        HIPCHK(c, hipEventRecord(b->fev[l], La.s));
        if (int r = fast_launch()) return r;
    }
    if (b->timing && La.it < RT_MAX_TIMED_ITERS) HIPCHK(c, hipEventRecord(La.tev[2][La.it], La.s));
    HIPCHK(c, hipGetLastError());
    La.it++;
    return RT_OK;
}

// few paths left and none waits: the tail kernel finishes them all
int WaveRun::launch_tail(WaveLane& La, int par)
{
    HIPCHK(c, hipMemsetAsync(La.cnt + C_TK_TAIL, 0, 4, La.s));
    La.W.spec_cam = P.spec_cam ? P.tail_spec_cam : 0;  // (the lane's last launch)
    launch_k_tail(SEQ, S, P.tail_rows, dim3(P.tail_blocks), La.s, La.W, par, stats);
    if (b->timing && La.it < RT_MAX_TIMED_ITERS) HIPCHK(c, hipEventRecord(La.tev[2][La.it], La.s));
    HIPCHK(c, hipGetLastError());
    La.tail_iter = La.it;
    La.it++;
    La.done = true;
    return RT_OK;
}

int WaveRun::read_live(WaveLane& La)  // ACT counts of the next iteration
{
    HIPCHK(c, hipMemcpyAsync(La.h, La.cnt + ac_at(La.it & 1, 0), act_bytes, hipMemcpyDeviceToHost, La.s));
    HIPCHK(c, hipEventRecord(La.ev, La.s));
    La.await = Await::Live;
    return RT_OK;
}

// enqueue up to 8 iterations, then a readback
int WaveRun::issue(WaveLane& La)
{
    for (int k = 0; k < 8 && La.it < max_iters; k++) {
        if (int r = launch_trace(La)) return r;
        if (La.tail_next) {  // does any query wait for the exact walk?
            HIPCHK(c, hipMemcpyAsync(La.h + act_bytes / 4, La.cnt, 8 * 4, hipMemcpyDeviceToHost, La.s));
            HIPCHK(c, hipEventRecord(La.ev, La.s));
            La.await = Await::Fallbacks;
            return RT_OK;
        }
        if (int r = launch_step(La)) return r;
        if ((La.it & 7) == 0) break;
    }
    return read_live(La);
}

int WaveRun::process(WaveLane& La)
{
    HIPCHK(c, hipEventSynchronize(La.ev));
    const Await kind = La.await;
    La.await = Await::None;
    if (kind == Await::Fallbacks) {  // (a fallback pending: step, then the live count, checked again next iteration)
        const int par = La.it & 1;
        const int32_t* f = La.h + act_bytes / 4;
        if (f[C_FBC0 + par] == 0 && f[C_FBA0 + par] == 0 && f[C_PARKC0 + (par ^ 1)] == 0 &&
            f[C_PARKA0 + (par ^ 1)] == 0)  // (k_trace(i) released DONE[par ^ 1])
            return launch_tail(La, par);
        if (int r = launch_step(La)) return r;
        return read_live(La);
    }
    long live = 0;
    for (int j = 0; j < RT_QSHARDS; j++) live += La.h[j * RT_CSTRIDE];
    La.live = live;
    La.done = live == 0;
    La.tail_next = !La.done && live <= P.tail_max;
    const bool before_hand = La.fast == Fast::Waiting || La.fast == Fast::HistPending;
    if (before_hand && (La.done || La.tail_next)) {  // (no hand-over from this lane)
        if (La.fast == Fast::HistPending) HIPCHK(c, hipEventSynchronize(b->hev[lane_of(La)]));  // (its readback is done with h_hist)
        La.fast = Fast::NoShare;
        return fast_launch();
    }
    if (La.fast == Fast::Waiting && La.it >= P.fast_iter) return start_hist(La);
    return RT_OK;
}

// the samples-done histogram of the lane's live paths, read back asynchronously
// (fast_threshold picks it up from a later k_step launch)
int WaveRun::start_hist(WaveLane& La)
{
    const int l = lane_of(La);
    int32_t* hh = (int32_t*)b->fhist[l].p;
    HIPCHK(c, hipMemsetAsync(hh, 0, (size_t)(spp + 1) * 4, La.s));
    rtk::WaveView HW = La.W;
    HW.act_in = La.lists[La.it & 1];
    hipLaunchKernelGGL(k_hist, dim3((unsigned)std::min(1024l, (La.live + threads - 1) / threads)), dim3(threads), 0, La.s,
                       HW, La.it & 1, hh);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(b->h_hist[l], hh, (size_t)(spp + 1) * 4, hipMemcpyDeviceToHost, La.s));
    HIPCHK(c, hipEventRecord(b->hev[l], La.s));
    La.fast = Fast::HistPending;
    return RT_OK;
}

// The host serves whichever lane's readback has completed (hipEventQuery), so a lane whose
// batch is done is refilled at once instead of idling while the host blocks on another
// lane's event (blocking in lane order left lanes idle 17-34 ms of a 367-ms cfg4 8-way
// shard: profiles/r04e_tl.json; 379.5-380.2 -> 370.5-373.2 ms, cfg2 148.5-149.7 -> 148.0,
// profiles/r04i_drain_probe.json).
// (a thread that finds no lane done for a while sleeps between polls: in a multi-device
// render every device thread polls like this, and the caller's host work shares the cores)
int WaveRun::poll()
{
    auto idle_since = std::chrono::steady_clock::now();
    for (;;) {
        bool any = false, moved = false;
        for (int l = 0; l < P.lanes; l++) {
            WaveLane& La = L[l];
            if (La.await != Await::None) {
                any = true;
                const hipError_t q = hipEventQuery(La.ev);
                if (q == hipErrorNotReady) continue;
                HIPCHK(c, q);
                if (int r = process(La)) return r;
                moved = true;
            }
            if (!La.done && La.await == Await::None) {
                if (La.it >= max_iters) {
                    HIPCHK(c, hipStreamSynchronize(La.s));
                    return rt_fail(c, RT_ERR_STATE, "render: wavefront loop did not drain in " +
                                                            std::to_string(max_iters) + " iterations (step budget " +
                                                            std::to_string(b->budget) + ")");
                }
                if (int r = issue(La)) return r;
                any = moved = true;
            }
        }
        if (!any) break;
        if (moved) {
            idle_since = std::chrono::steady_clock::now();
        } else if (std::chrono::steady_clock::now() - idle_since > std::chrono::microseconds(200)) {
            std::this_thread::sleep_for(std::chrono::microseconds(10));
        } else {
            std::this_thread::yield();
        }
    }
    return RT_OK;
}

// each lane's pixels tone-mapped after its last step; the lanes joined back into s
int WaveRun::finish()
{
    const int nl = P.lanes;
    for (int l = 0; l < nl; l++) {
        if (fast_ran)
            HIPCHK(c, hipStreamWaitEvent(L[l].s, b->fev_done, 0));  // (and the fast lane's)
        if (pass) continue;  // (a progressive pass leaves the pixels paused: rt_progress_resolve tone-maps)
        if (linear) continue;  // (rt_render_linear: the framebuffer keeps finish_pixel's sum)
        hipLaunchKernelGGL(k_tonemap, dim3((L[l].n + threads - 1) / threads), dim3(threads), 0, L[l].s, L[l].W);
        HIPCHK(c, hipGetLastError());
    }
    b->last_iters = 0;
    for (int l = 0; l < nl; l++) {
        b->last_iters = std::max(b->last_iters, L[l].it);
        if (l > 0) {
            HIPCHK(c, hipEventRecord(b->ev_join[l], b->ls[l]));
            HIPCHK(c, hipStreamWaitEvent(s, b->ev_join[l], 0));
        }
    }
    b->tail_iter = L[0].tail_iter;
    HIPCHK(c, hipEventRecord(b->ev_done, s));
    b->done_recorded = true;
    return RT_OK;
}

// The run's diagnostics: walk log, iteration counts, per-kernel ms, timeline, RT_DEBUG_FB.
int WaveRun::report()
{
    const int nl = P.lanes;
    const RtDiag& dg = c->diag;
    if (wlog) {  // (diagnostics: device 0's records of this render replace the last render's)
        int32_t nw = 0;
        HIPCHK(c, hipMemcpyAsync(&nw, b->wlog.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        RtDiag& d = c->diag;
        d.wlog_total = nw;
        d.wlog.assign((size_t)std::min(nw, d.wlog_cap) * RT_WLOG_FLOATS, 0.0f);
        if (!d.wlog.empty())
            HIPCHK(c, hipMemcpy(d.wlog.data(), (char*)b->wlog.p + 256, d.wlog.size() * 4, hipMemcpyDeviceToHost));
    }
    if (S && iter_log) {
        std::vector<int32_t> hq((size_t)6 * RT_MAX_TIMED_ITERS);
        HIPCHK(c, hipMemcpyAsync(hq.data(), b->iterq.p, hq.size() * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (FILE* f = fopen((std::string(iter_log) + ".counts").c_str(), "w")) {
            const int32_t* h2 = hq.data() + 2 * RT_MAX_TIMED_ITERS;
            for (int i = 0; i <= L[0].it && i < RT_MAX_TIMED_ITERS; i++)
                fprintf(f, "%d %d %d %d %d %d %d\n", i, hq[2 * i], hq[2 * i + 1], h2[4 * i], h2[4 * i + 1], h2[4 * i + 2],
                        h2[4 * i + 3]);
            fclose(f);
        }
    }
    if (b->timing) {  // per-kernel-class time of this render (HIP events on the launch streams)
        HIPCHK(c, hipStreamSynchronize(s));
        FILE* lf = iter_log ? fopen((std::string(iter_log) + ".ms").c_str(), "w") : nullptr;
        for (int l = 0; l < nl; l++)
            for (int i = 0; i < L[l].it && i < RT_MAX_TIMED_ITERS; i++)
                for (int k = 0; k < 2; k++) {
                    float ms = 0;
                    HIPCHK(c, hipEventElapsedTime(&ms, L[l].tev[k][i], L[l].tev[k + 1][i]));
                    const int cls = (k == 1 && i == L[l].tail_iter) ? 2 : k;  // the tail kernel: class "other"
                    b->kms[cls] += ms;
                    b->klaunch[cls] += 1;
                    if (lf && l == 0) {
                        if (k == 0)
                            fprintf(lf, "%d %.4f", i, ms);
                        else
                            fprintf(lf, " %.4f\n", ms);
                    }
                }
        if (lf) fclose(lf);
        // RT_TIMELINE=file: every lane's launches on one clock (ms from lane 0's first
        // k_trace): lane, iteration, k_trace start, k_trace end = k_step start, k_step end,
        // 1 for the tail kernel (tools/timeline.py); the fast lane's kernel as lane `lanes`,
        // iteration 0, flag 2
        // (device index d > 0 of a multi-device context writes file.d: the device threads run concurrently)
        if (!dg.timeline.empty()) {
            const char* tl = dg.timeline.c_str();
            std::string rows;
            char line[128];
            for (int l = 0; l < nl; l++)
                for (int i = 0; i < L[l].it && i < RT_MAX_TIMED_ITERS; i++) {
                    float t[3];
                    for (int k = 0; k < 3; k++) HIPCHK(c, hipEventElapsedTime(&t[k], L[0].tev[0][0], L[l].tev[k][i]));
                    snprintf(line, sizeof line, "%d %d %.4f %.4f %.4f %d\n", l, i, t[0], t[1], t[2],
                             i == L[l].tail_iter ? 1 : 0);
                    rows += line;
                }
            if (fast_ran) {
                float t[2];
                for (int k = 0; k < 2; k++) HIPCHK(c, hipEventElapsedTime(&t[k], L[0].tev[0][0], b->ftev[k]));
                snprintf(line, sizeof line, "%d 0 %.4f %.4f %.4f 2\n", nl, t[0], t[1], t[1]);
                rows += line;
            }
            const std::string path = b->index > 0 ? std::string(tl) + "." + std::to_string(b->index) : std::string(tl);
            if (FILE* f = fopen(path.c_str(), "w")) {
                fwrite(rows.data(), 1, rows.size(), f);
                fclose(f);
            }
        }
    }
#if RT_DEBUG_FB
    {
        unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(c, hipStreamSynchronize(s));
        for (int l = 0; l < nl; l++) HIPCHK(c, hipStreamSynchronize(L[l].s));
        HIPCHK(c, hipMemcpyFromSymbol(v, HIP_SYMBOL(rt_dbg_fb), sizeof v));
        int its = 0;
        for (int l = 0; l < nl; l++) its = std::max(its, L[l].it);
        fprintf(stderr, "[rt dbg] n=%d iters=%d k_trace fallbacks closest=%llu any=%llu (overflow %llu tie %llu chain %llu; rows %llu) octet parks=%llu closest row drains=%llu\n",
                n, its, v[0], v[2], v[3], v[4], v[5], v[6], v[1], v[7]);
        const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(rt_dbg_fb), z, sizeof z));
    }
#endif
    return RT_OK;
}
}  // namespace

int run_wave(rt_context* c, Backend* b, int w, int h, int spp, int bounces, const rtk::PixSrc& src, int n, float4_* fb,
             hipStream_t s, const WavePass* pass, bool linear)
{
    if (n <= 0) return RT_OK;
    WaveRun R{c, b, w, h, spp, bounces, src, n, fb, s, pass, linear};
    if (int r = R.begin()) return r;
    if (int r = R.poll()) return r;
    if (int r = R.finish()) return r;
    return R.report();
}

int rt_wave_resolve(rt_context* c, const float4_* base, const float4_* state, float4_* out, int n, int done, hipStream_t s)
{
    hipLaunchKernelGGL(k_resolve, dim3((n + threads - 1) / threads), dim3(threads), 0, s, base, state, out, n, done);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

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
