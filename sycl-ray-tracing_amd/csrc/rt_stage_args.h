// rt_stage_args.h — the argument rules the frame stages share (rt_capi_stages.cpp): a stage's
// *_ready function lists its buffers once and applies the rules in the order it always has, with
// its own rules (parameter ranges, "both or neither") as plain lines in between. Host code only.
#pragma once

#include <cstdint>
#include <string>

#include "rt_context.h"

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// *params, or what the stage's rt_*_default_params fills in.
template <class P>
P params_or_defaults(const P* params, void (*defaults)(P*))
{
    P p;
    if (params) p = *params;
    else defaults(&p);
    return p;
}

struct StageBuf {
    const void* p;
    size_t bytes;
    bool out;        // the call writes it (else it reads it)
    bool required;   // NULL is an error (else NULL means "not given" and every rule skips it)
    unsigned align;  // what the device form asks of the pointer: 16 (a float4 per element) or 4
};
constexpr bool SA_IN = false, SA_OUT = true, SA_OPT = false, SA_REQ = true;

struct StageArgs {
    rt_context* c;
    std::string f;  // the call's name: the prefix of every message
    bool device;    // the device form
    StageBuf buf[10];  // (entries past the stage's own stay NULL)

    int fail(const char* msg, int code = RT_ERR_ARG) const { return rt_fail(c, code, f + msg); }

    bool missing() const  // a required buffer is NULL
    {
        for (const StageBuf& b : buf)
            if (b.required && !b.p) return true;
        return false;
    }

    // rt_denoise's frame limits: w*h <= 134217727 and, with rows, h <= 4 * 65535 (the kernels that tile the
    // frame 4 rows per block: 65535 blocks in y at most)
    int frame_limits(int w, int h, bool rows) const
    {
        if ((double)w * (double)h > 134217727.0) return fail(": too many pixels");
        if (rows && h > 4 * 65535) return fail(": height above 262140 rows");
        return RT_OK;
    }

    // o against the inputs, or (later_outputs) against the outputs listed after it
    bool hits(const StageBuf& o, bool later_outputs) const
    {
        for (const StageBuf* k = later_outputs ? &o + 1 : buf; k < buf + sizeof(buf) / sizeof(buf[0]); k++)
            if (k->p && k->out == later_outputs && ranges_overlap(o.p, o.bytes, k->p, k->bytes)) return true;
        return false;
    }
    // No output's bytes overlap an input's or another output's. Each output in turn, against the inputs and then
    // the outputs after it; inputs_first (rt_upscale): every output against the inputs before any pair of outputs.
    int overlap(bool inputs_first = false) const
    {
        for (const StageBuf& o : buf) {
            if (!o.out || !o.p) continue;
            if (hits(o, false)) return fail(": an output overlaps an input");
            if (!inputs_first && hits(o, true)) return fail(": two outputs overlap");
        }
        for (const StageBuf& o : buf)
            if (inputs_first && o.out && o.p && hits(o, true)) return fail(": two outputs overlap");
        return RT_OK;
    }

    // The device form's pointers are aligned (the kernels move a float4 with one 16-byte access).
    int aligned(const char* msg = ": the float4 buffers must be 16-byte aligned, the float buffers 4-byte aligned") const
    {
        for (const StageBuf& b : buf)
            if (device && b.p && (uintptr_t)b.p % b.align != 0) return fail(msg);
        return RT_OK;
    }
};
