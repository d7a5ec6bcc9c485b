// rt_dof.hip — gfx950 kernels and launch of the depth-of-field stage (rt_dof.h). Its own translation
// unit, so that the render kernels of rt_render.hip and the kernels of the other stages compile
// exactly as they do without it.
//
// One launch per call, one thread per output pixel. The 13 x 13 table of tap distances rides in the
// kernel's arguments (DofArgs::D): a tap's offset is uniform over the block, so its entry is a scalar.
//   k_dof_lds     a block of 512 threads makes a 32 x 16 tile. It first stages the tile's footprint,
//                 the tile plus a halo of max_radius on every side, (32 + 2R) x (16 + 2R) pixels:
//                 16-B global loads of the colour and of the guide record along the rows (dof_ld16: two
//                 global_load_dwordx4 per entry, both issued before anything tests their parts), coordinates
//                 clamped to the frame so that every load is inside it, the entries outside the image
//                 marked as rule 2 skips them (dof_skipped: r = -inf, so a = -inf). The radius and
//                 k(r), one division each, are computed once per staged pixel on the way in: no radius
//                 image exists in memory. Two arrays, one index: {r, g, b, r_q} as 16-B records
//                 (ds_read_b128) and {t_q, k(r_q)} as 8-B records (ds_read_b64). At a tap the 32
//                 lanes of a row read 32 consecutive records: ds_read_b128 serves lanes in four
//                 groups of 16 over 64 banks of 4 B, and the lanes of a group (0-3, 12-15, 20-27 or
//                 4-11, 16-19, 28-31 of a half-wave) hold 16 records whose 16-B slots are distinct
//                 modulo 16: no conflict whatever the pitch; ds_read_b64 serves a half-wave at once,
//                 32 consecutive 8-B records, the 64 banks once each. The LDS is dynamic, sized by the
//                 call's radius: 24 B per staged pixel, 53760 B at radius 12 (2240 pixels, 4.4 staged
//                 per output pixel; a 32 x 8 tile would stage 7), three blocks to a CU's 160 KiB;
//                 16128 B at radius 4.
//                 While staging, the block takes the largest r_q of the whole footprint, not of its
//                 own pixels: a neighbour's blur reaches into a tile that is itself in focus. The tap
//                 loops then run over -B .. B with B = ceil(that maximum), uniform over the block, and
//                 pass over a tap whose distance D is not below max r_q + 0.5: every such tap has
//                 re <= r_q, (re + 0.5) <= (max r_q + 0.5) <= D, a <= 0, and rule 2 skips it. A skipped
//                 tap adds nothing (rt_dof.h), so the shorter loop gives the rule's bits. D grows along
//                 a row of the table, so the taps kept in a row of the window are -X .. X: the table's
//                 row is loaded once across the wave's lanes, X is a ballot's population count, and a
//                 tap's D is a v_readlane. The tap loop takes four taps a round, their four ds_read_b128
//                 and four ds_read_b64 issued ahead of the first tap's arithmetic, the taps in the
//                 rule's order, then the one to three left over; it holds no other load and no branch
//                 but its own. A region in focus costs one tap per pixel. No thread returns
//                 before the last barrier; a thread outside the image computes from staged entries and
//                 does not store.
//   k_dof_direct  no LDS: the rule's whole window (dof_pixel, what the CPU build runs), every tap two
//                 16-B global loads (global_load_dwordx4) at a position clamped to the frame, read whole
//                 whether the tap is inside or not, and the radius and k(r) computed again, two
//                 divisions per tap; a tap outside the frame is then skipped. The yardstick for the
//                 tile; 64 x 4 pixels per block, a wave per row, as k_firefly_direct.
// Which kernel a call takes: rt_backend_dof.
#include <hip/hip_runtime.h>

#include <string>

#include "rt_backend_hip.h"
#include "rt_dof.h"

namespace {

#define DOF_TW 32  // k_dof_lds: tile width in pixels (half a wave per row) ...
#define DOF_TH 16  // ... and height; DOF_TW * DOF_TH threads
#define DOF_PW 64  // k_dof_direct: block width (one wave per row) ...
#define DOF_PH 4   // ... and height

struct alignas(8) DofTK {
    float t, k;
};

// One record as one 16-B load: a vector value, read whole before anything tests a part of it. (Read as
// the struct's four floats, the loads are sunk into the tests of dn_finite3 and dof_far and come out as
// dword pieces, each behind a wait of its own.)
typedef float dof_v4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4_ dof_ld16(const float4_* __restrict__ p)
{
    const dof_v4 v = *(const dof_v4*)p;
    return float4_{v.x, v.y, v.z, v.w};
}

// DofDirect (rt_dof.h) with both records read by dof_ld16, unconditionally, at a position clamped to the
// frame; a tap outside it is then skipped as the rule says.
struct DofGlobal {
    const rtk::DofArgs& A;
    __device__ __forceinline__ rtk::DofRec rec(int x, int y) const
    {
        const size_t q = (size_t)rt_mini(rt_maxi(y, 0), A.h - 1) * A.w + rt_mini(rt_maxi(x, 0), A.w - 1);
        const float4_ c = dof_ld16(A.in + q), g = dof_ld16(A.nd + q);
        const rtk::DofRec r = rtk::dof_record(A, c, g.w);
        return (x < 0 || x >= A.w || y < 0 || y >= A.h) ? rtk::dof_skipped() : r;
    }
};

__global__ __launch_bounds__(256) void k_dof_direct(rtk::DofArgs A, float4_* __restrict__ out, float* __restrict__ coc_out)
{
    const int x = blockIdx.x * DOF_PW + (threadIdx.x & (DOF_PW - 1));
    const int y = blockIdx.y * DOF_PH + (threadIdx.x / DOF_PW);
    if (x >= A.w || y >= A.h) return;
    const size_t p = (size_t)y * A.w + x;
    const DofGlobal F{A};
    float r;
    out[p] = rtk::dof_pixel(A, x, y, dof_ld16(A.in + p), dof_ld16(A.nd + p).w, F, &r);
    if (coc_out) coc_out[p] = r;
}

// Lane i's value of v, i uniform: a v_readlane into a scalar register.
__device__ __forceinline__ float dof_lane(float v, int i)
{
    return rt_asfloat((uint32_t)__builtin_amdgcn_readlane((int)rt_asuint(v), i));
}

__global__ __launch_bounds__(DOF_TW* DOF_TH) void k_dof_lds(rtk::DofArgs A, float4_* __restrict__ out,
                                                             float* __restrict__ coc_out)
{
    extern __shared__ float4_ s_dof[];  // fw * fh colour records, then fw * fh {t, k} records
    __shared__ int s_rmax;              // the footprint's largest radius, as the bits of a float >= 0
    const int R = A.R;
    const int fw = DOF_TW + 2 * R, fh = DOF_TH + 2 * R, fn = fw * fh;
    float4_* s_cr = s_dof;
    DofTK* s_tk = (DofTK*)(s_dof + fn);
    const int X0 = blockIdx.x * DOF_TW, Y0 = blockIdx.y * DOF_TH;
    if (threadIdx.x == 0) s_rmax = 0;
    __syncthreads();
    float rmax = 0.0f;
    for (int i = threadIdx.x; i < fn; i += DOF_TW * DOF_TH) {
        const int ly = i / fw, lx = i - ly * fw;
        const int gx = X0 - R + lx, gy = Y0 - R + ly;
        const bool inside = gx >= 0 && gx < A.w && gy >= 0 && gy < A.h;
        const size_t q = (size_t)rt_mini(rt_maxi(gy, 0), A.h - 1) * A.w + rt_mini(rt_maxi(gx, 0), A.w - 1);
        const float4_ c = dof_ld16(A.in + q), g = dof_ld16(A.nd + q);
        const rtk::DofRec in_rec = rtk::dof_record(A, c, g.w);
        const rtk::DofRec rec = inside ? in_rec : rtk::dof_skipped();
        s_cr[i] = rec.cr;
        s_tk[i] = DofTK{rec.t, rec.k};
        rmax = rt_max(rmax, rec.cr.w);  // (a skipped entry's -inf never wins)
    }
    atomicMax(&s_rmax, (int)rt_asuint(rmax));  // (floats >= 0 order as their bits do)
    __syncthreads();
    const float fmax = rt_asfloat((uint32_t)__builtin_amdgcn_readfirstlane(s_rmax));
    int B = (int)fmax;  // (0 <= fmax <= R)
    if ((float)B < fmax) B++;
    const float reach = fmax + 0.5f;

    const int tx = threadIdx.x & (DOF_TW - 1), ty = threadIdx.x / DOF_TW;
    const int x = X0 + tx, y = Y0 + ty;
    const int ci = (ty + R) * fw + tx + R;
    const float4_ pc = s_cr[ci];
    const DofTK pt = s_tk[ci];
    // (a centre with a bad colour, or outside the image, holds r = -inf: its sums are never used)
    const rtk::DofCentre P{pc.w, pt.t, pt.k};
    rtk::DofSum s{0.0f, 0.0f, 0.0f, 0.0f};
    const int lane = threadIdx.x & 63;
    for (int dy = -B; dy <= B; dy++) {
        // The table's row for |dy| across the wave's lanes, entry |dx| in lane |dx|: a tap's D is then a
        // v_readlane into a scalar register, not a load. D grows with |dx|, so the taps the test above keeps
        // are -X .. X, X + 1 the number of entries below `reach` among the first B + 1.
        const float dv = A.D[rtk::dof_absi(dy) * rtk::DOF_TAB + rt_mini(lane, rtk::DOF_MAX_RADIUS)];
        const unsigned long long keep = __ballot(lane <= B && dv < reach);
        if (!keep) continue;  // (uniform, like X)
        const int X = __popcll(keep) - 1;
        const int row = ci + dy * fw;
        // Four taps a round, their eight LDS reads issued before the first tap's arithmetic, the taps
        // themselves in the rule's order; then the one to three taps left over (2 X + 1 is odd).
        int dx = -X;
        for (; dx + 3 <= X; dx += 4) {
            float4_ qc[4];
            DofTK qt[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                // (the index through an empty asm: from one base register the compiler pairs the 8-B reads into
                // ds_read2_b64, which the LDS serves at a quarter of ds_read_b64's rate)
                int i = row + dx + j;
                asm volatile("" : "+v"(i));
                qc[j] = s_cr[row + dx + j], qt[j] = s_tk[i];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) rtk::dof_tap(s, P, qc[j], qt[j].t, qt[j].k, dof_lane(dv, rtk::dof_absi(dx + j)));
        }
        for (; dx <= X; dx++) {
            const float4_ qc = s_cr[row + dx];
            const DofTK qt = s_tk[row + dx];
            rtk::dof_tap(s, P, qc, qt.t, qt.k, dof_lane(dv, rtk::dof_absi(dx)));
        }
    }
    if (x >= A.w || y >= A.h) return;
    const size_t p = (size_t)y * A.w + x;
    const float4_ c = dof_ld16(A.in + p);  // (alpha, and a bad centre's own bits)
    if (pc.w >= 0.0f) {
        out[p] = rtk::dof_resolve(s, c);
        if (coc_out) coc_out[p] = pc.w;
    } else {
        out[p] = c;
        if (coc_out) coc_out[p] = rtk::dof_radius(A, dof_ld16(A.nd + p).w);
    }
}

size_t dof_lds_bytes(int R) { return (size_t)(DOF_TW + 2 * R) * (DOF_TH + 2 * R) * (sizeof(float4_) + sizeof(DofTK)); }

int dof_launch(rt_context* c, const rtk::DofArgs& A, bool lds, float4_* d_out, float* d_coc, hipStream_t s)
{
    if (lds) {
        const dim3 grid((A.w + DOF_TW - 1) / DOF_TW, (A.h + DOF_TH - 1) / DOF_TH);
        hipLaunchKernelGGL(k_dof_lds, grid, dim3(DOF_TW * DOF_TH), dof_lds_bytes(A.R), s, A, d_out, d_coc);
    } else {
        const dim3 grid((A.w + DOF_PW - 1) / DOF_PW, (A.h + DOF_PH - 1) / DOF_PH);
        hipLaunchKernelGGL(k_dof_direct, grid, dim3(256), 0, s, A, d_out, d_coc);
    }
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

}  // namespace

int rt_backend_dof(rt_context* c, rtk::DofArgs A, void* rgba_out, void* coc_out, bool device, void* stream)
{
    Backend* b = rt_backend_dev0(c);
    StagedCall st;
    if (int r = st.enter(c, b, device, stream, nullptr)) return r;
    const size_t n = (size_t)A.w * A.h, bytes = n * sizeof(float4_);
    if (int r = st.staging(b->dof_io, 3 * bytes + st.pad(n * sizeof(float)))) return r;
    A.in = (const float4_*)st.in(A.in, bytes);
    A.nd = (const float4_*)st.in(A.nd, bytes);
    float4_* d_out = (float4_*)st.out(rgba_out, bytes);
    float* d_coc = (float*)st.out(coc_out, n * sizeof(float));  // (may be null)
    if (int r = st.begin()) return r;
    // Which kernel the call takes (dof_variant, rt_use_lds): the faster of the two as measured on the MI355X
    // (profiles/dof_bench.json), LDS / direct ms at 1920x1080 on a frame defocused everywhere: 0.10 /
    // 0.30 at radius 4, 0.25 / 0.99 at 8, 0.55 / 2.1 at 12; in focus everywhere 0.04 / 0.32, 0.05 / 1.0, 0.07 / 2.1;
    // the same ratios at 3840x2160. The tile wins at every radius, so the dispatch does not look at it.
    const bool lds = rt_use_lds(c->sched.variant[RT_VAR_DOF], true);
    if (int r = dof_launch(c, A, lds, d_out, d_coc, st.s)) return r;
    return st.end();
}

// MEASUREMENT HOOK, like rt_device_upscale_kernel_ms of rt_upscale.hip: exported by the gfx950 library
// only, not part of include/rt_hip.h, never called by the product paths.
// GPU time of the two kernels on one footing (tools/dof_bench.py): for each of reps rounds each kernel
// runs alone on the default stream between two events recorded immediately before and after it. The
// arguments are validated by one rt_dof_device call first. Round r runs kernel (r + first) & 1 before the
// other. out_ms[k * reps + r]: k = 0 k_dof_direct, 1 k_dof_lds.
extern "C" int rt_device_dof_kernel_ms(rt_context* c, int w, int h, const void* d_in, const void* d_nd, const rt_dof_params* params,
                                       void* d_out, void* d_coc, int reps, int first, double* out_ms)
{
    TimedRounds T;
    if (int r = T.enter(c, "rt_device_dof_kernel_ms", reps, out_ms)) return r;
    if (int r = rt_dof_device(c, w, h, d_in, d_nd, params, d_out, d_coc, nullptr)) return r;
    rt_dof_params p;
    if (params) p = *params;
    else rt_dof_default_params(&p);
    rtk::DofArgs A{w, h, p.max_radius, p.focus, p.coc_inf, (const float4_*)d_in, (const float4_*)d_nd, {}};
    rtk::dof_build_table(A.D);
    auto kernel = [&](bool lds) { return [&, lds] { return dof_launch(c, A, lds, (float4_*)d_out, (float*)d_coc, nullptr); }; };
    return T.run(first, {TimedKernel::turns(0, kernel(false)), TimedKernel::turns(1, kernel(true))});
}
