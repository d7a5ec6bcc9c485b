// rt_motion.hip — gfx950 kernels and launches of the motion stages (rt_motion.h). Its own translation
// unit, so that the render kernels of rt_render.hip and the kernels of the other stages compile
// exactly as they do without it.
//
//   k_motion_vectors  k_temporal's shape: 64 x 4 pixels per block, a wave per row, one pixel per thread;
//                     one 16-B guide load (global_load_dwordx4) and one 8-B store (global_store_dwordx2).
//   k_motion_tilemax  one block of 256 threads per 16 x 16 motion tile. Each thread takes rule 1 from its
//                     pixel's motion (one 8-B load) and forms the key of rule 2; the key's maximum is taken
//                     over the wave by six xor-shuffles, then over the four waves through 32 B of LDS, and
//                     the thread whose index the key names writes the tile's record {hx, hy, l, 0} as one
//                     16-B store into a buffer the context keeps (Backend::motion_tiles, grown as bloom's pyramid is).
//   k_mblur_lds       one block of 256 threads per motion tile, so the line's direction, n and every tap's
//                     offset are uniform over the block. Rule 3 is folded in: nine 16-B reads of the tile
//                     records at uniform addresses. A tile with L < 0.5 is a copy: no LDS, no barrier.
//                     Otherwise the block stages the bounding box of the tile swept along +-(Nx, Ny),
//                     (16 + 2 max|ox|) x (16 + 2 max|oy|) entries (48 x 16 for a horizontal streak of 16, 40 x 38
//                     at worst near the diagonal), not a square halo of max_radius: per entry a 16-B colour
//                     load, a 16-B guide load and an 8-B motion load at a position clamped to the frame
//                     (mb_ld16 / mb_ld8: whole records, all three issued before anything tests a part), rule 1
//                     computed on the way in, the entries outside the image or with a bad colour marked as
//                     mb_skipped so that the rule's own arithmetic gives them the weight +0. Two arrays, one
//                     index: {r, g, b, l_q} as 16-B records (ds_read_b128) and {t'_q, k_q} as 8-B records
//                     (ds_read_b64). Each lane i <= 2 n of a wave holds tap i - n's LDS offset and distance;
//                     a tap's two are v_readlane's into scalar registers, so the tap loop holds two LDS
//                     reads at the lane's own index plus a scalar and the rule's arithmetic, no global load.
//                     The 16 lanes of a tile row read 16 consecutive records, the wave's four rows a pitch
//                     apart. The LDS is dynamic, sized by the call's max_radius (mb_lds_entries: the largest
//                     box any direction of that length gives, 1520 entries = 36480 B at 16); a box that would
//                     not fit (none does, by that bound) takes the direct path for its tile. No thread
//                     leaves between the first barrier and the last.
//   k_mblur_direct    the rule as written (mb_pixel, what the CPU build runs) with every tap from global
//                     memory, the same block shape and the same folded rule 3. The yardstick for the tile.
// Which kernel a call takes: rt_backend_motion_blur.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "rt_backend_hip.h"
#include "rt_motion.h"

namespace {

#define MV_TW 64  // k_motion_vectors: block width (one wave per row) ...
#define MV_TH 4   // ... and height
#define MB_T rtk::MB_TILE
#define MB_THREADS (MB_T * MB_T)

struct alignas(8) MbTK {
    float t, k;
};

// One record as one load: a vector value, read whole before anything tests a part of it (rt_dof.hip dof_ld16).
typedef float mb_v4 __attribute__((ext_vector_type(4)));
typedef float mb_v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4_ mb_ld16(const float4_* __restrict__ p)
{
    const mb_v4 v = *(const mb_v4*)p;
    return float4_{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ rtk::MbVec mb_ld8(const rtk::MbVec* __restrict__ p)
{
    const mb_v2 v = *(const mb_v2*)p;
    return rtk::MbVec{v.x, v.y};
}
__device__ __forceinline__ float mb_uniform(float v) { return rt_asfloat((uint32_t)__builtin_amdgcn_readfirstlane((int)rt_asuint(v))); }
__device__ __forceinline__ float mb_lane(float v, int i) { return rt_asfloat((uint32_t)__builtin_amdgcn_readlane((int)rt_asuint(v), i)); }

__global__ __launch_bounds__(256) void k_motion_vectors(rtk::MotionVecArgs A, rtk::MbVec* __restrict__ out)
{
    const int x = blockIdx.x * MV_TW + (threadIdx.x & (MV_TW - 1));
    const int y = blockIdx.y * MV_TH + (threadIdx.x / MV_TW);
    if (x >= A.cur.W || y >= A.cur.H) return;
    const size_t p = (size_t)y * A.cur.W + x;
    const rtk::MbVec m = rtk::mv_pixel(A, x, y, mb_ld16(A.nd + p));
    *(mb_v2*)(out + p) = mb_v2{m.x, m.y};
}

__global__ __launch_bounds__(MB_THREADS) void k_motion_tilemax(rtk::MotionArgs A, float4_* __restrict__ tiles)
{
    __shared__ unsigned long long s_key[MB_THREADS / 64];
    const int tx = threadIdx.x & (MB_T - 1), ty = threadIdx.x / MB_T;
    const int x = blockIdx.x * MB_T + tx, y = blockIdx.y * MB_T + ty;
    const bool live = x < A.w && y < A.h;
    const size_t p = (size_t)rt_mini(y, A.h - 1) * A.w + rt_mini(x, A.w - 1);
    const float4_ r = rtk::mb_reach(A, mb_ld8(A.motion + p));
    unsigned long long key = live ? rtk::mb_key(r.z, (int)threadIdx.x) : 0ull;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    unsigned long long best = s_key[0];
#pragma unroll
    for (int i = 1; i < MB_THREADS / 64; i++) best = s_key[i] > best ? s_key[i] : best;
    // (pixel (0, 0) of a tile is inside the image, so best is a live pixel's key)
    if (rtk::mb_key_index(best) == (int)threadIdx.x) tiles[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
}

// MbDirect (rt_motion.h) with the three records read whole, unconditionally, at a position clamped to the
// frame; a tap outside it is then skipped as the rule says.
struct MbGlobal {
    const rtk::MotionArgs& A;
    __device__ __forceinline__ rtk::MbRec rec(int x, int y) const
    {
        const size_t q = (size_t)rt_mini(rt_maxi(y, 0), A.h - 1) * A.w + rt_mini(rt_maxi(x, 0), A.w - 1);
        const float4_ c = mb_ld16(A.in + q), g = mb_ld16(A.nd + q);
        const rtk::MbVec m = mb_ld8(A.motion + q);
        const rtk::MbRec r = rtk::mb_record(A, c, g.w, m);
        return (x < 0 || x >= A.w || y < 0 || y >= A.h) ? rtk::mb_skipped() : r;
    }
};

// The tile's {Nx, Ny, L} (rule 3), in scalar registers.
__device__ __forceinline__ float4_ mb_tile_line(const float4_* __restrict__ tiles)
{
    const float4_ N = rtk::mb_neighbour_max(tiles, (int)gridDim.x, (int)gridDim.y, (int)blockIdx.x, (int)blockIdx.y);
    return float4_{mb_uniform(N.x), mb_uniform(N.y), mb_uniform(N.z), 0.0f};
}

// One pixel by the rule as written (k_mblur_direct; k_mblur_lds for a box beyond its LDS).
__device__ __forceinline__ void mb_direct_pixel(const rtk::MotionArgs& A, const float4_& N, int x, int y, float4_* __restrict__ out,
                                                float* __restrict__ reach_out)
{
    if (x >= A.w || y >= A.h) return;
    const size_t p = (size_t)y * A.w + x;
    const float4_ c = mb_ld16(A.in + p), g = mb_ld16(A.nd + p);
    const float l = rtk::mb_reach(A, mb_ld8(A.motion + p)).z;
    const MbGlobal F{A};
    out[p] = rtk::mb_pixel(A, x, y, c, g.w, l, N, F);
    if (reach_out) reach_out[p] = l;
}

__global__ __launch_bounds__(MB_THREADS) void k_mblur_direct(rtk::MotionArgs A, const float4_* __restrict__ tiles,
                                                             float4_* __restrict__ out, float* __restrict__ reach_out)
{
    const float4_ N = mb_tile_line(tiles);
    const int x = blockIdx.x * MB_T + (threadIdx.x & (MB_T - 1)), y = blockIdx.y * MB_T + threadIdx.x / MB_T;
    mb_direct_pixel(A, N, x, y, out, reach_out);
}

__global__ __launch_bounds__(MB_THREADS) void k_mblur_lds(rtk::MotionArgs A, const float4_* __restrict__ tiles, int cap,
                                                          float4_* __restrict__ out, float* __restrict__ reach_out)
{
    extern __shared__ float4_ s_mb[];  // fw * fh colour records, then fw * fh {t', k} records
    const float4_ N = mb_tile_line(tiles);
    const int tx = threadIdx.x & (MB_T - 1), ty = threadIdx.x / MB_T;
    const int X0 = blockIdx.x * MB_T, Y0 = blockIdx.y * MB_T;
    const int x = X0 + tx, y = Y0 + ty;
    const bool live = x < A.w && y < A.h;
    const size_t p = (size_t)rt_mini(y, A.h - 1) * A.w + rt_mini(x, A.w - 1);
    if (!(N.z >= 0.5f)) {  // (uniform) a still tile among still tiles: the copy
        if (!live) return;
        out[p] = mb_ld16(A.in + p);
        if (reach_out) reach_out[p] = rtk::mb_reach(A, mb_ld8(A.motion + p)).z;
        return;
    }
    const rtk::MbLine ln = rtk::mb_line(N);
    const int n = ln.n;
    // |ox_j| and |oy_j| are largest at an end of the line ((float)j * dx is monotonic in j, and so is its floor)
    const int mx = rt_maxi(rtk::mb_absi(rtk::mb_off(-n, ln.dx)), rtk::mb_absi(rtk::mb_off(n, ln.dx)));
    const int my = rt_maxi(rtk::mb_absi(rtk::mb_off(-n, ln.dy)), rtk::mb_absi(rtk::mb_off(n, ln.dy)));
    const int fw = MB_T + 2 * mx, fh = MB_T + 2 * my, fn = fw * fh;
    if (fn > cap) {  // (uniform; never taken while mb_lds_entries bounds the box)
        mb_direct_pixel(A, N, x, y, out, reach_out);
        return;
    }
    float4_* s_cl = s_mb;
    MbTK* s_tk = (MbTK*)(s_mb + fn);
    for (int i = threadIdx.x; i < fn; i += MB_THREADS) {
        const int ly = i / fw, lx = i - ly * fw;
        const int gx = X0 - mx + lx, gy = Y0 - my + ly;
        const bool inside = gx >= 0 && gx < A.w && gy >= 0 && gy < A.h;
        const size_t q = (size_t)rt_mini(rt_maxi(gy, 0), A.h - 1) * A.w + rt_mini(rt_maxi(gx, 0), A.w - 1);
        const float4_ c = mb_ld16(A.in + q), g = mb_ld16(A.nd + q);
        const rtk::MbVec m = mb_ld8(A.motion + q);
        const rtk::MbRec in_rec = rtk::mb_record(A, c, g.w, m);
        const rtk::MbRec rec = inside ? in_rec : rtk::mb_skipped();
        s_cl[i] = rec.cl;
        s_tk[i] = MbTK{rec.t, rec.k};
    }
    // Tap i - n of the line in lane i of every wave: its offset in the footprint and its distance.
    const int lane = threadIdx.x & 63;
    const int j = rt_mini(lane, 2 * n) - n;
    const int tap_off = rtk::mb_off(j, ln.dy) * fw + rtk::mb_off(j, ln.dx);
    const float tap_d = (float)rtk::mb_absi(j) * ln.ds;
    __syncthreads();

    const int ci = (ty + my) * fw + tx + mx;
    const float4_ pc = s_cl[ci];
    const MbTK pt = s_tk[ci];
    // (a centre with a bad colour, or outside the image, holds l = -1: its sums are never used)
    const rtk::MbCentre P{pc.w, pt.t, pt.k, 1.0f / (A.depth_soft * pt.t)};
    rtk::MbSum s{0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i <= 2 * n; i++) {
        if (i == n) {
            rtk::mb_centre_tap(s, P, pc);
            continue;
        }
        const int q = ci + __builtin_amdgcn_readlane(tap_off, i);
        const float4_ qc = s_cl[q];
        const MbTK qt = s_tk[q];
        rtk::mb_tap(s, P, qc, qt.t, qt.k, mb_lane(tap_d, i));
    }
    if (!live) return;
    const float4_ c = mb_ld16(A.in + p);  // (alpha, and a bad centre's own bits)
    if (pc.w >= 0.0f) {
        out[p] = rtk::mb_resolve(s, c);
        if (reach_out) reach_out[p] = pc.w;
    } else {
        out[p] = c;
        if (reach_out) reach_out[p] = rtk::mb_reach(A, mb_ld8(A.motion + p)).z;
    }
}

// The largest footprint, in entries, a line of reach R can ask for: |ox| <= |Nx| + 0.5 and |Nx|^2 + |Ny|^2 <= R^2
// (rule 1 clamps l to R), with a little room for the roundings of s, dx and j * dx.
int mb_lds_entries(int R)
{
    int best = 0;
    for (int mx = 0; mx <= R; mx++)
        for (int my = 0; my <= R; my++) {
            const double ax = mx > 0 ? mx - 0.5 : 0.0, ay = my > 0 ? my - 0.5 : 0.0;
            if (ax * ax + ay * ay <= 1.001 * R * R) best = std::max(best, (MB_T + 2 * mx) * (MB_T + 2 * my));
        }
    return best;
}
size_t mb_lds_bytes(int R) { return (size_t)mb_lds_entries(R) * (sizeof(float4_) + sizeof(MbTK)); }

size_t mb_tile_bytes(int w, int h) { return (size_t)rtk::mb_tiles_x(w) * rtk::mb_tiles_y(h) * sizeof(float4_); }

int mb_launch_tilemax(rt_context* c, const rtk::MotionArgs& A, float4_* tiles, hipStream_t s)
{
    const dim3 grid(rtk::mb_tiles_x(A.w), rtk::mb_tiles_y(A.h));
    hipLaunchKernelGGL(k_motion_tilemax, grid, dim3(MB_THREADS), 0, s, A, tiles);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

int mb_launch_blur(rt_context* c, const rtk::MotionArgs& A, bool lds, const float4_* tiles, float4_* d_out, float* d_reach,
                   hipStream_t s)
{
    const dim3 grid(rtk::mb_tiles_x(A.w), rtk::mb_tiles_y(A.h));
    if (lds)
        hipLaunchKernelGGL(k_mblur_lds, grid, dim3(MB_THREADS), mb_lds_bytes(A.R), s, A, tiles, mb_lds_entries(A.R), d_out, d_reach);
    else hipLaunchKernelGGL(k_mblur_direct, grid, dim3(MB_THREADS), 0, s, A, tiles, d_out, d_reach);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

int mv_launch(rt_context* c, const rtk::MotionVecArgs& A, rtk::MbVec* d_out, hipStream_t s)
{
    const dim3 grid((A.cur.W + MV_TW - 1) / MV_TW, (A.cur.H + MV_TH - 1) / MV_TH);
    hipLaunchKernelGGL(k_motion_vectors, grid, dim3(256), 0, s, A, d_out);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

}  // namespace

int rt_backend_motion_vectors(rt_context* c, rtk::MotionVecArgs A, void* motion_out, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const size_t n = (size_t)A.cur.W * A.cur.H;
    if (int r = st.staging(b->motion_io, n * sizeof(float4_) + st.pad(n * sizeof(rtk::MbVec)))) return r;
    A.nd = (const float4_*)st.in(A.nd, n * sizeof(float4_));
    rtk::MbVec* d_out = (rtk::MbVec*)st.out(motion_out, n * sizeof(rtk::MbVec));
    if (int r = st.begin()) return r;
    if (int r = mv_launch(c, A, d_out, st.s)) return r;
    return st.end();
}

int rt_backend_motion_blur(rt_context* c, rtk::MotionArgs A, void* rgba_out, void* reach_out, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const size_t n = (size_t)A.w * A.h, bytes = n * sizeof(float4_);
    // The tile records live in a buffer of their own that only grows. A device-form call that has to grow it frees
    // the old one first, which waits for the device: no earlier call still reads it.
    if (int r = ensure(c, b->motion_tiles, mb_tile_bytes(A.w, A.h))) return r;
    if (int r = st.staging(b->motion_io, 3 * bytes + st.pad(n * sizeof(rtk::MbVec)) + st.pad(n * sizeof(float)))) return r;
    A.in = (const float4_*)st.in(A.in, bytes);
    A.nd = (const float4_*)st.in(A.nd, bytes);
    A.motion = (const rtk::MbVec*)st.in(A.motion, n * sizeof(rtk::MbVec));
    float4_* d_out = (float4_*)st.out(rgba_out, bytes);
    float* d_reach = (float*)st.out(reach_out, n * sizeof(float));  // (may be null)
    float4_* tiles = (float4_*)b->motion_tiles.p;
    if (int r = st.begin()) return r;
    if (int r = mb_launch_tilemax(c, A, tiles, st.s)) return r;
    // Which gather kernel the call takes (motion_variant, rt_use_lds): the faster of the two as measured on the MI355X
    // (profiles/motion_bench.json), the tile at every radius.
    const bool lds = rt_use_lds(c->sched.variant[RT_VAR_MOTION], true);
    if (int r = mb_launch_blur(c, A, lds, tiles, d_out, d_reach, st.s)) return r;
    return st.end();
}

// MEASUREMENT HOOK, like rt_device_dof_kernel_ms of rt_dof.hip: exported by the gfx950 library only, not part of
// include/rt_hip.h, never called by the product paths.
// GPU time of the stage's kernels on one footing (tools/motion_bench.py): for each of reps rounds each kernel runs
// alone on the default stream between two events recorded immediately before and after it. The arguments are
// validated by one rt_motion_blur_device call first (and one rt_motion_vectors_device call when d_vec_out is given:
// the context then needs a camera). Round r runs the blur kernel (r + first) & 1 before the other.
// out_ms[k * reps + r]: k = 0 k_mblur_direct, 1 k_mblur_lds, 2 k_motion_tilemax, 3 k_motion_vectors (0 without d_vec_out).
extern "C" int rt_device_motion_kernel_ms(rt_context* c, int w, int h, const void* d_in, const void* d_nd, const void* d_motion,
                                          const rt_motion_params* params, void* d_out, void* d_reach, const float* prev_view,
                                          float prev_fov_dist, void* d_vec_out, int reps, int first, double* out_ms)
{
    TimedRounds T;
    if (int r = T.enter(c, "rt_device_motion_kernel_ms", reps, out_ms)) return r;
    if (int r = rt_motion_blur_device(c, w, h, d_in, d_nd, d_motion, params, d_out, d_reach, nullptr)) return r;
    if (d_vec_out)
        if (int r = rt_motion_vectors_device(c, w, h, d_nd, prev_view, prev_fov_dist, d_vec_out, nullptr)) return r;
    rt_motion_params p;
    if (params) p = *params;
    else rt_motion_default_params(&p);
    const rtk::MotionArgs A{w, h, p.max_radius, 0.5f * p.shutter, p.depth_soft, (const float4_*)d_in, (const float4_*)d_nd,
                            (const rtk::MbVec*)d_motion};
    rtk::MotionVecArgs V;
    if (d_vec_out)
        if (int r = rt_motion_vec_args(c, w, h, d_nd, prev_view, prev_fov_dist, V)) return r;
    float4_* tiles = (float4_*)rt_backend_dev0(c)->motion_tiles.p;
    auto blur = [&](bool lds) {
        return [&, lds] { return mb_launch_blur(c, A, lds, tiles, (float4_*)d_out, (float*)d_reach, nullptr); };
    };
    return T.run(first, {TimedKernel::fixed(2, [&] { return mb_launch_tilemax(c, A, tiles, nullptr); }),
                         TimedKernel::turns(0, blur(false)),
                         TimedKernel::turns(1, blur(true)),
                         d_vec_out ? TimedKernel::fixed(3, [&] { return mv_launch(c, V, (rtk::MbVec*)d_vec_out, nullptr); })
                                   : TimedKernel::absent(3)});
}
