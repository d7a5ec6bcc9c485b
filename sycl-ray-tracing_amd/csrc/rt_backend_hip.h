// rt_backend_hip.h — what the gfx950 backend (rt_render.hip) shares with the translation
// units of the post stage (rt_denoise.hip) and of the ray queries (rt_query.hip): the root
// device's ordinal, scene view and timing events, and a slot for each unit's own buffers.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_context.h"

struct RtRootDev {
    int device;               // HIP ordinal of the context's root device
    const RtSceneView* view;  // its scene view (valid after rt_backend_upload)
    hipEvent_t ev0, ev1;      // the events rt_last_kernel_ms / rt_device_last_kernel_ms read
    void** post;              // the post stage's state, created on first use; rt_post_free releases it
    void** query;             // the ray queries' workspace, likewise; rt_query_free releases it
};

int rt_backend_root(rt_context* c, RtRootDev* out);  // rt_render.hip
void rt_post_free(void* post);                       // rt_denoise.hip (the device is current)
void rt_query_free(void* query);                     // rt_query.hip (the device is current)
