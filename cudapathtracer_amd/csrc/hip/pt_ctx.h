// pt_ctx.h -- the render context (pt_ctx) as a record: the scene's scalars, its arrays on the device and the buffers
// the entry points grow inside it.  pt_render_host.h creates, fills and destroys it (pt_create / pt_destroy); a
// translation unit with kernels of its own over the scene's device arrays (pt_lightmap.hip: tris_orig) includes this
// file and reads them where they are.  Host only; nothing here emits code.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../host/host_internal.h"
#include "../host/render_plan.h"
#include "pt_records.h"
#include "pt_scene_pack.h"

struct pt_ctx : pt::SceneInfo {            // (the scene's scalars: pt_scene_pack.h)
    int device = 0;
    int num_cus = 256;
    pt::RenderKnobs knobs;                 // the PT_* knobs as they were at pt_create
    // the packed scene's arrays on the device (pt::PackedScene has the same names)
    ptd::DNode* nodes = nullptr;
    ptd::RNode* rnodes = nullptr;
    ptd::DTri* tris_leaf = nullptr;
    ptd::DTri* tris_orig = nullptr;
    ptd::DShade* shade = nullptr;
    ptd::DMat* mats = nullptr;
    ptd::DLight* lights = nullptr;
    uint32_t* jump = nullptr;
    float4* shade_m = nullptr;        // merged shading records (Args::shade_m), or none
    ptd::DNode4* nodes4 = nullptr;
    ptd::DTri* acc_tris = nullptr;
    uint32_t* rparent = nullptr;
    float4* hrec = nullptr;
    float* tone_thr = nullptr;        // output step: the host libm's 255 code boundaries (+ t[0] = 0)
    float4* spheres = nullptr;        // sphere primitives (center, radius)
    ptd::DTri* emis = nullptr;        // last-bounce light probe: records of the emissive triangles
    uint32_t* tri_counts = nullptr;   // PT_FLAG_COUNT: per-triangle test counts (num_tris entries, >= 1)
    uint32_t* jump_bytes = nullptr;   // byte-position jump matrices (built on the first wavefront render)
    hipEvent_t jump_ready = nullptr;  // recorded behind their build
    float* scratch_out = nullptr;     // pt_render: the image on the device
    size_t scratch_floats = 0;
    void* pinned = nullptr;                    // pt_render: pinned staging buffer of the image copy-out
    size_t pinned_bytes = 0;
    // renders in flight (pt_render_device_async / pt_render_wait): a FIFO of kFlights slots, each with
    // its events and a pinned host copy of the render's counters
    struct Flight {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;   // the whole render
        hipEvent_t ek0 = nullptr, ek1 = nullptr;   // the integration kernel alone
        hipEvent_t done = nullptr;                 // after the counters' copy
        unsigned long long* hcnt = nullptr;        // pinned: the counters, copied behind the render
        bool kernel_events = false, count = false;
        uint64_t units = 0, split = 0;
        int32_t spp = 0, bounces = 0;
    };
    static constexpr int kFlights = 2;
    Flight fl[kFlights];
    // A render's device scratch, one set per in-flight slot, so that two queued renders (e.g. frames on
    // two streams) never share a buffer; set 0 also serves the batched trace entry points.
    struct Bufs {
        uint32_t* spill = nullptr;            // per-lane stack spill columns, then the shading records
        size_t spill_words = 0;
        uint32_t* pix_states = nullptr;       // init_pixel_states output (kUnitWords per work unit)
        size_t pix_states_words = 0;
        double* lbuf = nullptr;               // per-sample radiance of split pixels
        size_t lbuf_words = 0;
        uint32_t* pmemo = nullptr;            // per-pixel-slot primary hit shared by a split pixel's chunks
        size_t pmemo_words = 0;
        unsigned long long* counters = nullptr;
        uint32_t* pixel_counter = nullptr;    // the unit queues
        uint32_t* tile_counter = nullptr;
        uint32_t* seed_states = nullptr;      // per-render seed_table output
        uint64_t seed_cached = 0;             // the seed seed_states was built for
        bool seed_valid = false;
    };
    Bufs rb[kFlights];
    int fl_head = 0, fl_n = 0;                 // oldest in-flight slot, number in flight
    pt::DenoiseScratch denoise;       // pt_denoise*'s device scratch (pt_denoise.hip), grown on demand
    pt::SessionScratch session;       // pt_session_save / _load's staging (pt_session.cpp), grown on demand
    uint8_t* query_stage = nullptr;   // pt_occluded's device staging (rays, bounds, answers), grown on demand
    size_t query_stage_bytes = 0;
    uint32_t* ray_classes = nullptr;  // classify_rays' four words (pt_render_rays*, pt_rays_classify_device)
    size_t ray_classes_words = 0;
    float* rays_stage = nullptr;      // pt_render_rays' device staging of the host ray buffer, grown on demand
    size_t rays_stage_floats = 0;
};
