// rt_wave_kernels.h — the launches of rt_render.hip's kernels, all the wavefront driver
// (rt_wave_run.hip) sees of them. Each enqueues on stream s and checks nothing: the caller
// reads hipGetLastError.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_wave_layout.h"

constexpr int rt_wave_threads = 256;  // threads per block of every render kernel

// One launch helper per kernel family: (SEQ, S, brute / rows) -> the instantiation.
// SEQ: counter renders with unpaired occlusion walks; S: counter renders; brute: USE_BVH 0
// scenes (the walks that keep the triangles' original indices); rows: k_tail walks by rows.
void launch_k_trace(bool SEQ, bool S, bool brute, dim3 g, hipStream_t s, const rtk::WaveView& W, int par,
                    unsigned long long* stats);
void launch_k_tail_fast(bool SEQ, bool S, dim3 g, hipStream_t s, const rtk::WaveView* fv, int4 parts,
                        unsigned long long* stats);
void launch_k_step(bool S, dim3 g, hipStream_t s, const rtk::WaveView& W, int par, unsigned long long* stats);
void launch_k_tail(bool SEQ, bool S, bool rows, dim3 g, hipStream_t s, const rtk::WaveView& W, int par,
                   unsigned long long* stats);
// The kernels with one instantiation.
void launch_k_init(dim3 g, hipStream_t s, const rtk::WaveView& W);
void launch_k_resume(dim3 g, hipStream_t s, const rtk::WaveView& W);
void launch_k_tonemap(dim3 g, hipStream_t s, const rtk::WaveView& W);
void launch_k_hand(dim3 g, hipStream_t s, const rtk::WaveView& W, int par);
void launch_k_hist(dim3 g, hipStream_t s, const rtk::WaveView& W, int par, int32_t* hist);
void launch_k_resolve(dim3 g, hipStream_t s, const float4_* base, const float4_* state, float4_* out, int n, int done);
#if RT_DEBUG_FB
// study builds: the kernels' rt_dbg_fb counters into v, then zeroed
hipError_t rt_wave_dbg_fb_take(unsigned long long v[8]);
#endif
