// plan_check — rt_plan.h wave_plan against a table of plans worked out from the expressions
// run_wave evaluated inline before the plan function existed (each row: those expressions
// evaluated by hand for the case's inputs, never wave_plan's own output). Knobs as the
// product builds them: RT_TRACE_OCC 6, RT_TAIL_OCC 3, RT_HEAVY_CALLS 6, RT_TAIL_ROWS 1,
// RT_DRAIN_ROWS 3, RT_TAIL_MAXP 16, RT_QSHARDS 64. Exit status 0 iff every field agrees.
#include <cstdio>

#include "rt_plan.h"

struct LaneRow {
    int n, seg_cap, first, off, stride, fb_rs, fast_n;
};
struct Case {
    const char* name;
    // inputs
    RtSchedule sc;
    WaveSource src;
    int n, spp, cus;
    bool seq;
    int set_lanes, set_budget;
    // expected
    int lanes, fast_k;
    long fast_iter;
    int heavy_calls, spec_cam, tail_spec_cam, tail_rows, drain_rows, tail_p, tail_blocks, trace_blocks;
    double tail_enter;
    long tail_max;
    int budget;
    LaneRow lane[RT_MAX_LANES];
};

static RtSchedule sched(int lanes, int fast_k)
{
    RtSchedule s;
    s.lanes = lanes;
    s.fast_k = fast_k;
    return s;
}
static RtSchedule sched_seq()
{
    RtSchedule s;
    s.tail_paths = 5, s.step_budget = 77, s.fast_spp = 2.0;
    return s;
}
static RtSchedule sched_knobs()
{
    RtSchedule s;
    s.tail_rows = 0, s.tail_enter = 1.75, s.heavy_calls = 0, s.spec_cam = 2, s.tail_spec_cam = 1, s.drain_rows = 0;
    return s;
}

static int bad = 0;
template <class T>
static void eq(const char* cs, const char* field, int lane, T got, T want)
{
    if (got == want) return;
    bad++;
    std::printf("%s: %s", cs, field);
    if (lane >= 0) std::printf("[%d]", lane);
    std::printf(" = %g, expected %g\n", (double)got, (double)want);
}

int main()
{
    const WaveKnobs K{6, 3, 6, 1, 3, 16, 64};
    const Case cases[] = {
        // auto lanes with the default fast lane: 3 lanes, the fourth queue the fast lane's
        {"640x480 defaults", RtSchedule(), {false, 640, 0, 1}, 307200, 2, 256, false, 0, 1024,
         3, 768, 4, 6, 1, 0, 1, 3, 1, 768, 1536, 2.0, 2048, 1024,
         {{102400, 1600, 0, 0, 3, 3, 256}, {102400, 1600, 640, 1, 3, 3, 256}, {102400, 1600, 1280, 2, 3, 3, 256}}},
        // fast_k = 0 with 4 lanes asked for: the 4-lane tail entry
        {"640x480 lanes 4, no fast lane", sched(4, 0), {false, 640, 0, 1}, 307200, 2, 256, false, 0, 1024,
         4, 0, 4, 6, 1, 0, 1, 3, 1, 768, 1536, 1.4, 1075, 1024,
         {{76800, 1216, 0, 0, 4, 4, 0}, {76800, 1216, 640, 1, 4, 4, 0}, {76800, 1216, 1280, 2, 4, 4, 0},
          {76800, 1216, 1920, 3, 4, 4, 0}}},
        // fast_k = 0, auto: 4 lanes up to RT_LANES4_MAX slots, 3 above
        {"1280x720 auto, no fast lane", sched(0, 0), {false, 1280, 0, 1}, 921600, 2, 256, false, 0, 1024,
         4, 0, 4, 6, 1, 0, 1, 3, 1, 768, 1536, 1.4, 1075, 1024,
         {{230400, 3648, 0, 0, 4, 4, 0}, {230400, 3648, 1280, 1, 4, 4, 0}, {230400, 3648, 2560, 2, 4, 4, 0},
          {230400, 3648, 3840, 3, 4, 4, 0}}},
        {"1920x1080 auto, no fast lane", sched(0, 0), {false, 1920, 0, 1}, 2073600, 2, 256, false, 0, 1024,
         3, 0, 4, 6, 1, 0, 1, 3, 1, 768, 1536, 2.0, 2048, 1024,
         {{691200, 10816, 0, 0, 3, 3, 0}, {691200, 10816, 1920, 1, 3, 3, 0}, {691200, 10816, 3840, 2, 3, 3, 0}}},
        // n below 2 x 65536: one lane, which keeps the whole fast-lane share
        {"400x250 defaults", RtSchedule(), {false, 400, 0, 1}, 100000, 4, 256, false, 0, 1024,
         1, 768, 9, 6, 1, 0, 1, 3, 1, 768, 1536, 2.0, 6144, 1024,
         {{100000, 1600, 0, 0, 1, 1, 768}}},
        // a pixel list, 4 lanes asked for and n shrinks them to 3: runs of the list
        {"pixel list 200001, lanes 4", sched(4, -1), {true, 640, 0, 1}, 200001, 8, 256, false, 0, 1024,
         3, 768, 18, 6, 1, 0, 1, 3, 1, 768, 1536, 2.0, 2048, 1024,
         {{66667, 1088, 0, 0, 1, 1, 256}, {66667, 1088, 66667, 0, 1, 1, 256}, {66667, 1088, 133334, 0, 1, 1, 256}}},
        // SEQ (counter renders): no row walks; a shard of rows 1, 9, 17, ... of a 1080p frame
        {"SEQ shard 1920x135", sched_seq(), {false, 1920, 1, 8}, 259200, 64, 256, true, 0, 512,
         3, 768, 128, 6, 1, 0, 0, 0, 5, 768, 1536, 2.0, 10240, 77,
         {{86400, 1408, 0, 1, 24, 3, 256}, {86400, 1408, 1920, 9, 24, 3, 256}, {86400, 1408, 3840, 17, 24, 3, 256}}},
        // the backend's 3 lanes shrunk by 2 rows; spp above RT_FAST_MAX_SPP: no fast lane; 304 CUs
        {"2 rows of 100000, backend lanes 3", sched_knobs(), {false, 100000, 3, 2}, 200000, 5000, 304, false, 3, 1024,
         2, 0, 11250, 0, 2, 1, 0, 0, 2, 912, 1824, 1.75, 6384, 1024,
         {{100000, 1600, 0, 3, 4, 2, 0}, {100000, 1600, 100000, 5, 4, 2, 0}}},
    };
    for (const Case& C : cases) {
        const int rows = C.src.pixel_list ? 0 : C.n / C.src.w;
        const WavePlan P = wave_plan(C.sc, K, C.src, C.n, rows, C.spp, C.cus, C.seq, C.set_lanes, C.set_budget);
        eq(C.name, "lanes", -1, P.lanes, C.lanes);
        eq(C.name, "fast_k", -1, P.fast_k, C.fast_k);
        eq(C.name, "fast_iter", -1, P.fast_iter, C.fast_iter);
        eq(C.name, "heavy_calls", -1, P.heavy_calls, C.heavy_calls);
        eq(C.name, "spec_cam", -1, P.spec_cam, C.spec_cam);
        eq(C.name, "tail_spec_cam", -1, P.tail_spec_cam, C.tail_spec_cam);
        eq(C.name, "tail_rows", -1, P.tail_rows, C.tail_rows);
        eq(C.name, "drain_rows", -1, P.drain_rows, C.drain_rows);
        eq(C.name, "tail_p", -1, P.tail_p, C.tail_p);
        eq(C.name, "tail_blocks", -1, P.tail_blocks, C.tail_blocks);
        eq(C.name, "trace_blocks", -1, P.trace_blocks, C.trace_blocks);
        eq(C.name, "tail_enter", -1, P.tail_enter, C.tail_enter);
        eq(C.name, "tail_max", -1, P.tail_max, C.tail_max);
        eq(C.name, "budget", -1, P.budget, C.budget);
        for (int l = 0; l < C.lanes && l < P.lanes; l++) {
            const LanePlan& g = P.lane[l];
            const LaneRow& w = C.lane[l];
            eq(C.name, "n", l, g.n, w.n);
            eq(C.name, "seg_cap", l, g.seg_cap, w.seg_cap);
            eq(C.name, "first", l, g.first, w.first);
            eq(C.name, "off", l, g.off, w.off);
            eq(C.name, "stride", l, g.stride, w.stride);
            eq(C.name, "fb_rs", l, g.fb_rs, w.fb_rs);
            eq(C.name, "fast_n", l, g.fast_n, w.fast_n);
        }
    }
    std::printf("plan_check: %d cases, %d mismatches\n", (int)(sizeof cases / sizeof cases[0]), bad);
    return bad == 0 ? 0 : 1;
}
