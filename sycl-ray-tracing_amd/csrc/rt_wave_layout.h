// rt_wave_layout.h — what the render kernels (rt_render.hip) and the wavefront driver
// (rt_wave_run.hip) must agree on: the counters[] layout, the queue segments in k_trace's
// stream order, and the build-time knobs the driver sizes grids and plans by (WaveKnobs).
#pragma once

#include <hip/hip_runtime.h>

#include "rt_wave.h"

#ifndef RT_DEBUG_FB
#define RT_DEBUG_FB 0  // study builds: count k_trace's exact-walk hand-overs and the octet walks'
                       // parks of the timed renders, printed on stderr after each run_wave
#endif

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
#ifndef RT_DRAIN_ROWS
#define RT_DRAIN_ROWS 3  // k_trace: once a wave's stream is out and at most this many quads still walk,
                         // their walks continue as rows (rt_row.h); 0 = off. cfg4 8-way shard, one
                         // MI355X (profiles/r04i_drain_probe.json, r04j_probe.json): off / 4 / 3 / 2 / 1 ->
                         // 370-373 / 362.6-362.9 / 359.9-361.4 / 360.5-363.6 / 366.5-367.3 ms, cfg2 148.0 /
                         // 145.3-145.9 / 145.1-145.4 / 145.6-146.0 / 147.1-147.6 ms
#endif
#define RT_TAIL_MAXP 16  // k_tail: paths per wave at most (RK_COUNT rays each per list)
#ifndef RT_TAIL_OCC
#define RT_TAIL_OCC 3    // k_tail waves per SIMD (2: no spills but half the paths per launch; 3 measured faster)
#endif
#define RT_QSTACK 32            // quad walks (rt_quad.h): stack entries per quad (item + key, 64 quads per block)
#define RT_RSTACK 64            // row walks (rt_row.h): stack entries per row (item + key, 16 rows per block)

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
