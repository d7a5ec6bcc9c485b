// rt_plan.h — what a wavefront render (rt_wave_run.hip run_wave) decides before its first
// launch: the lane count, the tail and fast-lane figures and each lane's share of the
// launch. Host only and free of HIP calls, so tests/native/plan_check.cpp runs it as it is.
#pragma once

#include <algorithm>

#include "rt_context.h"

#define RT_MAX_LANES 4  // wavefront lanes (streams) per render (run_wave)
#define RT_FAST_K 768         // fast lane: paths handed over (run_wave)
#define RT_FAST_SPP 2.25      // ... from iteration RT_FAST_SPP x spp on
#define RT_FAST_MAX_SPP 4096  // ... in renders of at most this many samples per pixel
#define RT_LANES4_MAX 1572864  // auto lanes: 4 at most this many slots per launch, else 3

// The kernels' build-time knobs the plan depends on (rt_wave_run.hip fills them from rt_wave_layout.h's macros).
struct WaveKnobs {
    int trace_occ, tail_occ;  // RT_TRACE_OCC, RT_TAIL_OCC
    int heavy_calls;          // RT_HEAVY_CALLS
    int tail_rows, drain_rows, tail_maxp;  // RT_TAIL_ROWS, RT_DRAIN_ROWS, RT_TAIL_MAXP
    int qshards;              // RT_QSHARDS
};

// The launch's pixels: rows of src_w pixels (row j at image row off + j * stride), or a pixel list.
struct WaveSource {
    bool pixel_list;
    int w, off, stride;
};

struct LanePlan {
    int n;          // path slots
    int seg_cap;    // entries per queue shard (append_emit: chunks per shard)
    int first;      // its first pixel in the launch's list / framebuffer (pixel lists: a run; rows: row l)
    int off, stride;  // rows: its first image row and the stride between its rows
    int fb_rs;      // framebuffer rows from one of its rows to the next
    int fast_n;     // fast lane: the paths it hands over at most
};

struct WavePlan {
    int lanes;
    int fast_k;
    long fast_iter;
    int heavy_calls, spec_cam, tail_spec_cam, tail_rows, drain_rows, tail_p;
    int tail_blocks, trace_blocks;
    double tail_enter;
    long tail_max;
    int budget;
    LanePlan lane[RT_MAX_LANES];
};

// set_lanes / set_budget: the backend's own settings (rt_device_set_lanes, RT_STEP_BUDGET).
inline WavePlan wave_plan(const RtSchedule& sc, const WaveKnobs& K, const WaveSource& src, int n, int rows, int spp,
                          int dev_cus, bool SEQ, int set_lanes, int set_budget)
{
    WavePlan P{};
    // k_trace: wave-strided over 2 grid-fills; RT_TRACE_OCC blocks resident per CU (quad
    // walks: 6 waves/SIMD measured best, 423 vs 374 Msamples/s at 4 and 350 at 8)
    // k_trace grid-fills (RT_TRACE_FILLS): with per-wave query streams one fill is best, a wave's
    // stream is longer and its end (the last long walk) costs less; cfg2: 0.75 / 1 / 1.25 / 1.5 / 2 / 3
    // -> 739 / 730-740 / 731 / 724 / 708-710 / 692 Msamples/s
    P.trace_blocks = dev_cus * K.trace_occ;
    // lanes: rows interleave (row j of the launch -> lane j % lanes); pixel lists split in runs
    const int lanes_set = sc.lanes > 0 ? std::min(RT_MAX_LANES, sc.lanes) : set_lanes;
    P.fast_k = spp <= RT_FAST_MAX_SPP ? std::max(0, std::min(1 << 16, sc.fast_k >= 0 ? sc.fast_k : RT_FAST_K)) : 0;
    // (auto: 3 lanes with the fast lane, the fourth hardware queue its stream)
    int nl = lanes_set > 0 ? lanes_set : n <= RT_LANES4_MAX && P.fast_k == 0 ? 4 : 3;
    while (nl > 1 && (n < nl * 65536 || (!src.pixel_list && rows < nl))) nl--;
    P.lanes = nl;
    P.heavy_calls = sc.heavy_calls >= 0 ? sc.heavy_calls : K.heavy_calls;
    // the next sample's camera ray traced ahead (rt_wave.h next_camera): 1; 0 off; 2 only where
    // the pixel's previous sample ended (cfg2 -1.5 ms, the cfg4 8-way shard unchanged, r04)
    P.spec_cam = sc.spec_cam >= 0 ? sc.spec_cam : 1;
    // The camera ray traced ahead costs a walk whenever the sample goes on. In k_tail a round
    // waits for its path's slowest query, often that camera walk: there it is off (cfg4 8-way
    // shard 352.3-354.6 -> 343.5 ms, cfg2 142.5-143.6 -> 141.3-141.6, profiles/r04q_cam.json).
    P.tail_spec_cam = sc.tail_spec_cam >= 0 ? sc.tail_spec_cam : 0;  // the tail kernel's mode (as spec_cam)
    // k_tail paths per wave: a round waits for the slowest walk of the wave's ~3 P queries, so
    // fewer paths per wave move each chain faster. With the entry held at the same live count
    // (r03, P x RT_TAIL_ENTER = 3.5): P = 5 / 3 / 2 / 1 -> cfg2 886-893 / 892-896 / 897-901 /
    // 887-890 Msamples/s, cfg4 8-way shard (slowest rank) 401 / - / 390 / 405 ms
    // row walks (rt_row.h, 16 lanes per query over the 16-wide BVH) where walks are latency-bound:
    // the tail kernel (tail_rows: its rounds wait for their slowest walk). cfg4 8-way shard, one
    // MI355X (profiles/r04c_row_probe.json, r04d_tail_probe.json): quads 380-382 ms; tail rows
    // 367-370; rows for whole k_trace launches below 32 K / 131 K paths 415 / 420-428 ms (removed).
    // (counter renders with unpaired occlusion walks, SEQ: every walk a quad walk, so that the box
    // tests counted are the ones a one-node-per-trip walk makes; a row trip tests 16)
    P.tail_rows = SEQ ? 0 : sc.tail_rows >= 0 ? (sc.tail_rows != 0) : K.tail_rows;
    P.drain_rows = SEQ ? 0 : sc.drain_rows >= 0 ? sc.drain_rows : K.drain_rows;  // k_trace: a drain's walks continue as rows
    // (rows: one path per wave, its ~4 queries on the wave's 4 rows: shard 367 ms vs 2 / 3 paths
    // 373-378 / 373-375 at the same entry live count)
    P.tail_p = sc.tail_paths >= 0 ? std::min(K.tail_maxp, sc.tail_paths) : P.tail_rows ? 1 : 2;
    P.tail_blocks = dev_cus * K.tail_occ;  // one grid-fill of k_tail
    // a lane enters the tail kernel at 2x one grid-fill's pool (the waves refill from the live
    // list): with 2 paths per wave, RT_TAIL_ENTER = 1.4 / 1.75 / 2.2 / 2.8 -> cfg2 888-897 /
    // 891-898 / 893-897 / 874-879 Msamples/s (5 paths at 0.7: 888-892), cfg4 8-way shard
    // 393.5 / 389.6 / 393.1 / - ms (profiles/r03_tail_paths_ab.json)
    // (4 lanes, the auto count of launches of <= 1.5 M slots: 1.4 — cfg4 8-way shard, 4 rounds on
    // one MI355X: 2.0 / 1.5 / 1.25 / 1.0 -> 384-391 / 380-384 / 379-383 / 382-390 ms,
    // profiles/r03_tail_enter4.json)
    P.tail_enter = sc.tail_enter >= 0.0 ? sc.tail_enter : nl == 4 ? 1.4 : 2.0;
    // Fast lane: from iteration fast_spp x spp on, each lane's share of the fast_k live paths
    // with the fewest samples done (the pixels with the longest chains, tools/fastlane_model.py)
    // leaves the wavefront at the lane's next k_step; when every lane has handed its share over,
    // one tail kernel steps them all on a stream of their own (an idle lane's: 3 lanes + the fast
    // lane are the 4 hardware queues), at a tail round's pace beside the wavefront. cfg4 8-way
    // shard (rank 1) / cfg2, one MI355X, 3 rounds (profiles/r05_fast_lane.json): 4 lanes, none
    // 319.7-323.9 / 134.9-135.4 ms; 3 lanes + fast lane 768 paths at 2.0 / 2.25 x spp
    // 311.5-316.1 / 134.7-136.4 and 312.2-316.9 / 133.7-134.0; 1024 paths 308.1-317.6; 1536 and
    // more slower (r04's fast lane beside 4 lanes, a fifth stream: slower, r04x).
    P.fast_iter = (long)((sc.fast_spp >= 0.0 ? sc.fast_spp : RT_FAST_SPP) * spp);
    P.tail_max = (long)(P.tail_enter * P.tail_blocks * 4 * P.tail_p / nl);
    P.budget = sc.step_budget > 0 ? sc.step_budget : set_budget;
    for (int l = 0; l < nl; l++) {
        LanePlan& La = P.lane[l];
        La.off = src.off, La.stride = src.stride, La.fb_rs = 1;
        if (nl == 1) {
            La.n = n;
        } else if (src.pixel_list) {
            const int b0 = (int)((long)n * l / nl), b1 = (int)((long)n * (l + 1) / nl);
            La.n = b1 - b0;
            La.first = b0;
        } else {
            La.n = ((rows - l + nl - 1) / nl) * src.w;
            La.off = src.off + l * src.stride;
            La.stride = nl * src.stride;
            La.first = l * src.w;
            La.fb_rs = nl;
        }
        La.seg_cap = 64 * (((La.n + 63) / 64 + K.qshards - 1) / K.qshards);  // (append_emit: chunks per shard)
        La.fast_n = (int)((long)P.fast_k * (l + 1) / nl - (long)P.fast_k * l / nl);
    }
    return P;
}
