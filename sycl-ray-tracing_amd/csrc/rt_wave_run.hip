// rt_wave_run.hip — the host side of a wavefront render: run_wave's lanes on their streams,
// the readbacks that steer them, the fast lane's hand-over, and the run's diagnostics.
// No device code: the kernels are rt_render.hip's, launched through rt_wave_kernels.h; the
// counters they share with this loop are laid out in rt_wave_layout.h.
//
// A render (run_wave) is a loop of iterations over the in-flight path slots (one slot per
// pixel of the launch), split into up to 3 independent lanes on their own streams: k_trace,
// then k_step, until few paths are left and k_tail finishes them. Queue sizes live in device
// memory; the host only launches and, every 8 iterations, reads the live-slot count.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>
#include <algorithm>

#include <chrono>
#include <thread>

#include "rt_backend_hip.h"
#include "rt_wave.h"
#include "rt_wave_kernels.h"

// ------------------------------------------------------------- wave memory
size_t rt_wave_counter_bytes() { return C_COUNT * sizeof(int32_t); }
size_t rt_wave_readback_bytes() { return RT_QSHARDS * RT_CSTRIDE * 4 + 64; }

namespace {
const int threads = rt_wave_threads;
const WaveKnobs knobs{RT_TRACE_OCC, RT_TAIL_OCC, RT_HEAVY_CALLS, RT_TAIL_ROWS, RT_DRAIN_ROWS, RT_TAIL_MAXP, RT_QSHARDS};

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
    if (int r = b->ev_done.wait(c, s)) return r;
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
    HIPCHK(c, hipMemsetAsync(W.r_flags, 0, (size_t)La.n * 4, La.s));
    W.act_in = La.lists[1];
    W.act_out = La.lists[0];
    if (W.first > 0)
        launch_k_resume(dim3((La.n + threads - 1) / threads), La.s, W);
    else
        launch_k_init(dim3((La.n + threads - 1) / threads), La.s, W);
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
    if (!b->fev_done.ev) HIPCHK(c, hipEventCreateWithFlags(&b->fev_done.ev.h, hipEventDisableTiming));
    if (int r = b->fev_done.sync(c)) return r;  // (the last render's copy of the views)
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
    if (int r = b->fev_done.record(c, fstream)) return r;
    fast_ran = true;
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
        launch_k_hand(dim3((unsigned)std::min(1024l, (La.live + threads - 1) / threads)), La.s, HW, par);
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
    launch_k_hist(dim3((unsigned)std::min(1024l, (La.live + threads - 1) / threads)), La.s, HW, La.it & 1, hh);
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
            if (int r = b->fev_done.wait(c, L[l].s)) return r;  // (and the fast lane's)
        if (pass) continue;  // (a progressive pass leaves the pixels paused: rt_progress_resolve tone-maps)
        if (linear) continue;  // (rt_render_linear: the framebuffer keeps finish_pixel's sum)
        launch_k_tonemap(dim3((L[l].n + threads - 1) / threads), L[l].s, L[l].W);
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
    return b->ev_done.record(c, s);
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
        HIPCHK(c, rt_wave_dbg_fb_take(v));
        int its = 0;
        for (int l = 0; l < nl; l++) its = std::max(its, L[l].it);
        fprintf(stderr, "[rt dbg] n=%d iters=%d k_trace fallbacks closest=%llu any=%llu (overflow %llu tie %llu chain %llu; rows %llu) octet parks=%llu closest row drains=%llu\n",
                n, its, v[0], v[2], v[3], v[4], v[5], v[6], v[1], v[7]);
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
    launch_k_resolve(dim3((n + threads - 1) / threads), s, base, state, out, n, done);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}
