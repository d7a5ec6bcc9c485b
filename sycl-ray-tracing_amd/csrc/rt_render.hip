// rt_render.hip — the wavefront render kernels of librt_hip.so (gfx950) and their launch
// helpers (rt_wave_kernels.h), nothing else: this unit changes only when a render kernel
// does. The host loop that launches them is rt_wave_run.hip; the counters and queue
// segments both sides index are rt_wave_layout.h; the kernels no render calls are rt_probe.hip.
//
// One iteration of a lane (rt_wave_run.hip run_wave) over its in-flight path slots:
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
// k_init / k_resume start a lane's paths, k_tonemap / k_resolve write its pixels, k_hist and
// k_hand select and move the fast lane's paths, k_tail_fast steps them.
#include <hip/hip_runtime.h>

#include "rt_backend_hip.h"
#include "rt_wave.h"
#include "rt_wave_kernels.h"
#include "rt_quad.h"
#include "rt_row.h"
#include "rt_octet.h"

namespace {

// ------------------------------------------------------------ wave helpers
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
    if (W.heavy_calls > 0) {  // heavy class on: the rays of a path flagged heavy go to its kind's heavy shard
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

// Segment j of a prefix table pre[0..M] holding global index g (pre[j] <= g < pre[j+1]), M a
// compile-time table size, as an 8-way search: each round reads 7
// entries at once (independent LDS reads, one round trip) and advances by the count at or below
// g (the table is non-decreasing), so 448 entries take 3 dependent round trips instead of 9 and
// 64 take 2 instead of 6. k_trace's refill (on ~4 of 5 wave trips, the whole wave waiting) and
// every k_step / k_tail chunk start search these tables. (Against the binary search it
// replaced: cfg2 127.5 -> 125.3 ms, profiles/r06_refill_prefetch_ab.json.)
template <int M>
__device__ __forceinline__ int shard_find8(const int* pre, int g)
{
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

// k_trace's look-ahead (against reading each record from the queue at its refill: cfg2 -1.1 %,
// the 8-way shard -2.4 %, profiles/r06_refill_prefetch_ab.json): right after a refill, the wave's next 16 stream
// positions are copied into its LDS buffer by direct-to-LDS loads (lane 2i + h: half h of
// record i, 16 B; the hardware puts lane L's 16 B at buf + 16 L), their kinds alongside; the next
// refill takes its records from there (a refill needs at most 16 positions, all from the
// cursor on, which the buffer starts at), so the refill no longer waits on the queue's memory.
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
#define RT_LDS_WORDS 16         // LDS words per lane of k_trace (16 KB per block of 256)
#define RT_REFILL 16
#ifndef RT_TRACE_REFILL
#define RT_TRACE_REFILL 4       // k_trace: idle quads of a wave that trigger a refill from its query stream
                                // (r02, cfg2: 4 / 8 -> 726 / 723 vs 678 Msamples/s with static 16-query chunks)
#endif

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
    // (k_step's and k_tail's emitted rays wait in LDS, not in VGPRs: k_step's spill slots 27 -> 0,
    // cfg2 -3.6 %, profiles/r06_emit_lds_ab.json)
    __shared__ uint32_t s_lds[6 * rtk::RK_COUNT * 256];
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
        rtk::EmitLds<256> e;
        e.s = reinterpret_cast<float*>(s_lds) + threadIdx.x;
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
    constexpr int REFILL = G == 4 ? RT_TRACE_REFILL : 1;  // idle groups that trigger a refill
    const int lane = lane_id(), qd = lane / G;
    int sub = lane & (G - 1);
    int cursor = 0;                     // the wave's next stream position (uniform)
    bool exhausted = wg * 16 >= total;  // (uniform)
    bool active = false;
    uint32_t target = 0;
    rtk::QState q;  // (its ray is the query's: a fallback record is rebuilt from q.o, q.d and target)
    if (!exhausted) queue_prefetch(W, s_pre, pf, first, cursor, wg, wn, total);
    // a walk's end: its answer, or the exact walk's list; gs = lanes of the group walking it
    auto finish = [&](int res, int gs) {
        // a long walk: the path's next rays go to the heavy class (head of the next streams)
        // (q.calls counts quad_visit calls; a row call covers two 4-wide levels and counts 2)
        if (W.heavy_calls > 0 && sub == 0 && q.calls >= W.heavy_calls) rtk::res_flag(W, (int)(target >> 3), rtk::RF_HEAVY) = 1;
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
    // The common trip is one ballot and one branch around the visit: `trig` is the number of idle groups
    // at which the wave has something else to do, and it changes only where `exhausted` does, at a refill.
    //   stream not exhausted: REFILL idle groups (all groups idle is at least that many) -> refill;
    //   stream exhausted: every group idle -> done, or, with quads, few enough walking (W.drain_rows) -> rows.
    // (a group is idle or walking: popcount(idle) + popcount(walking) = NGROUPS, so "at most drain_rows walking"
    // is "at least NGROUPS - drain_rows idle")
    constexpr int NGROUPS = 64 / G;
    static_assert(REFILL <= NGROUPS, "all groups idle triggers a refill");
    const int trig_done = NGROUPS - (G == 4 && W.drain_rows > 0 ? min(W.drain_rows, NGROUPS) : 0);
    int trig = exhausted ? trig_done : REFILL;  // (uniform)
    for (;;) {
        const unsigned long long bidle = __ballot(!active && sub == 0);
        if (__popcll(bidle) >= trig) {
            if (!exhausted) {
                if (!active) {
                    const int j = cursor + __popcll(bidle & ((1ull << (qd * G)) - 1ull));  // this group's stream position
                    const int idx = (wg + (j >> 4) * wn) * 16 + (j & 15);
                    if (idx < total) {
                        const int slot = j - cursor;  // (0..15: the buffer starts at the cursor)
                        // (the compiler does not order LDS reads after direct-to-LDS loads: wait for
                        // the vector-memory counter here, vmcnt(0), before reading the buffer)
                        __builtin_amdgcn_s_waitcnt(0x0F70);
                        rtk::RayRec r;
                        r.o = pf.buf[2 * slot];
                        r.d = pf.buf[2 * slot + 1];
                        const int kind = pf.kind[slot];
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
                // (every lane has read its record: the buffer is free for the next 16 positions)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (!exhausted) queue_prefetch(W, s_pre, pf, first, cursor, wg, wn, total);
                if (STATS && lane == 0) ps->c[RT_STAT_REFILLS]++;
                trig = exhausted ? trig_done : REFILL;
            }
            const unsigned long long bact = __ballot(active && sub == 0);
            if (!bact) {
                if (exhausted) break;
                continue;
            }
            if (G == 4 && W.drain_rows > 0 && exhausted && __popcll(bact) <= W.drain_rows) break;  // to rows (below)
        }
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
        if (q.cur != rtk::RT_CUR_NONE) q.cur = 0;
#elif RT_DRAIN_RESTART == 2  // (study build: a new walk of the same ray, nothing of the quad's kept)
        if (ract) rtk::qstate_begin<ANY>(q, q.o, q.d, sub, nullptr);
#elif RT_DRAIN_RESTART == 3  // (study build: the ray's box-test form recomputed from o and d)
        q.rb = rtk::rayb_setup(q.o, q.d);
#elif RT_DRAIN_RESTART == 4  // (study build: the walk's hit record reset; the walk goes on from its stack)
        q.h.t = __builtin_inff(), q.h.t2 = __builtin_inff(), q.h.k = ANY ? 0 : -1, q.h.leaf = -1;
        q.h.prim = 0x7fffffff, q.h.tie = false, q.h.ovf = false;
        q.sp = 0;
        if (q.cur != rtk::RT_CUR_NONE) q.cur = 0;
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
    __shared__ float4_ s_qbuf[4][64];  // per wave: the next 16 stream records (queue_prefetch)
    __shared__ int s_qkind[4][16];
    const QPrefetch pf{s_qbuf[threadIdx.x >> 6], s_qkind[threadIdx.x >> 6]};
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
// k_tail: a path's emitted rays stay in the wave's LDS columns (EmitLds<RT_TAIL_MAXP>, lane j
// of the wave's paths in column j); the lists hold (j << 3 | kind) (l0: closest-hit kinds,
// l1: occlusion). (With the rays in registers and lists of whole 32-B records k_tail had fewer
// spill slots, 28 / 20 against 34 / 24, and measured 0.8 % slower: profiles/r06_emit_lds_ab.json.)
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
// FAST: the fast lane's launch, one kernel over every lane's handed-over paths: blocks
// [fparts[l], fparts[l + 1]) step lane l's (fviews[l]: its fast list as shard 0 of its own
// counters, its own spill area).
template <bool STATS, bool PAIR, int G, bool FAST>
__device__ __forceinline__ void tail_body(const rtk::WaveView& W, int par, unsigned long long* stats, int blk)
{
    __shared__ float s_em[4][6 * rtk::RK_COUNT * RT_TAIL_MAXP];        // per wave: its paths' rays (TailEmit columns)
    __shared__ uint8_t s_q[4][2][RT_TAIL_MAXP * rtk::RK_COUNT];        // per wave: closest list, occlusion list
    __shared__ int s_my[4][RT_TAIL_MAXP];                              // per wave: the slot of column j
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
            if (lane < RT_TAIL_MAXP) s_my[wv][lane] = my;
            const int r = tail_step(W, my, last_kind, s_em[wv], s_q[wv][0], s_q[wv][1], ps);
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
                    const int ent = s_q[wv][l][l ? qi - nl[0] : qi], j = ent >> 3, kind = ent & 7;
                    TailEmit ce;
                    ce.s = s_em[wv] + j;
                    rtk::RayRec r;
                    r.o = rtk::f4(ce.o(kind), 0.0f);
                    r.d = rtk::f4(ce.d(kind), 0.0f);
                    target = ((uint32_t)s_my[wv][j] << 3) | (uint32_t)kind;
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

const int threads = rt_wave_threads;
}  // namespace

// ----------------------------------------------------------------- launches
// (rt_wave_kernels.h) One launch helper per kernel family: (SEQ, S, brute / rows) -> the instantiation.
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
void launch_k_init(dim3 g, hipStream_t s, const rtk::WaveView& W) { hipLaunchKernelGGL(k_init, g, dim3(threads), 0, s, W); }
void launch_k_resume(dim3 g, hipStream_t s, const rtk::WaveView& W) { hipLaunchKernelGGL(k_resume, g, dim3(threads), 0, s, W); }
void launch_k_tonemap(dim3 g, hipStream_t s, const rtk::WaveView& W) { hipLaunchKernelGGL(k_tonemap, g, dim3(threads), 0, s, W); }
void launch_k_hand(dim3 g, hipStream_t s, const rtk::WaveView& W, int par)
{
    hipLaunchKernelGGL(k_hand, g, dim3(threads), 0, s, W, par);
}
void launch_k_hist(dim3 g, hipStream_t s, const rtk::WaveView& W, int par, int32_t* hist)
{
    hipLaunchKernelGGL(k_hist, g, dim3(threads), 0, s, W, par, hist);
}
void launch_k_resolve(dim3 g, hipStream_t s, const float4_* base, const float4_* state, float4_* out, int n, int done)
{
    hipLaunchKernelGGL(k_resolve, g, dim3(threads), 0, s, base, state, out, n, done);
}
#if RT_DEBUG_FB
hipError_t rt_wave_dbg_fb_take(unsigned long long v[8])
{
    if (hipError_t e = hipMemcpyFromSymbol(v, HIP_SYMBOL(rt_dbg_fb), 8 * sizeof v[0])) return e;
    const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(rt_dbg_fb), z, sizeof z);
}
#endif

