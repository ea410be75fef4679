// pt_scene_pack.h -- a scene as the kernels read it (pt_scene_pack.cpp): every device record of pt_create as
// host vectors, ready to upload.  Host only.
#pragma once

#include <chrono>
#include <vector>

#include "../host/host_internal.h"
#include "../host/render_plan.h"
#include "pt_records.h"

namespace pt {

// What a render context keeps of its scene besides the device arrays.
struct SceneInfo {
    uint32_t num_tris = 0;
    int32_t depth = 0;                // of the reference BVH
    float root[6] = {};               // its root box
    float scene_extent = 1.0f;
    bool scene_fast = false;          // all scene coordinates admit the Markstein quotient
    uint32_t node_mask = 0;           // low bits of a packed stack entry holding a reference node index
    uint32_t num_lights = 0;
    float total_light_area = 0;
    uint32_t num_spheres = 0;
    uint32_t sphere_mat_base = 0;
    uint32_t top_nodes = 0;           // nodes of this scene's BVH4 that are LDS-staged (<= wf_top)
    uint32_t n4 = 0;                  // nodes of this scene's BVH4
    float acc_root[6] = {};
    int32_t acc4_depth = 0;
    uint32_t node4_mask = 0;
    uint32_t num_emis = 0;            // (0 = probe off: spheres present, too many emitters, PT_NO_LIGHT_PROBE)
    bool tone_ok = false;
    uint64_t scene_digest = 0;        // FNV-1a of the scene arrays (a checkpoint file names its scene by it)
    uint32_t scene_spheres = 0;       // ... and the sphere count of that scene
};

struct PackedScene : SceneInfo {
    RenderKnobs knobs;                      // the caller's, with this scene's defaults of wf_threshold and
                                            // wf_root_first (a tree held whole in LDS) where they were not set
    std::vector<ptd::DNode> nodes;          // reference BVH, both children per record
    std::vector<ptd::RNode> rnodes;         // ... as the reference has it
    std::vector<uint32_t> rparent;          // ... parent of each node
    std::vector<ptd::DTri> tris_leaf;       // DFS leaf order (culled walk)
    std::vector<ptd::DTri> tris_orig;       // original order (reference walk)
    std::vector<ptd::DShade> shade;
    std::vector<float4> shade_m;            // merged shading records, or empty
    std::vector<ptd::DMat> mats;            // scene materials, then one per sphere
    std::vector<ptd::DLight> lights;        // num_lights + 1: the last is "nothing picked" (primitive 0)
    std::vector<float4> spheres;
    std::vector<ptd::DNode4> nodes4;        // render-path BVH4: the LDS-staged top first
    std::vector<ptd::DTri> acc_tris;        // its triangle records by slot, permuted for tri_hit_pk
    std::vector<float4> hrec;               // per slot: winner check + shading words (Args::hrec)
    std::vector<ptd::DTri> emis;            // last-bounce light probe: the emissive triangles
    std::vector<uint32_t> jump;             // byte-sliced XORWOW jump tables
    std::vector<float> tone;                // output step: the host libm's 255 code boundaries
};

// PT_TIMING=1: host-side phase times of pt_create on stderr (tools/debug/ingest_timing.py reads them)
struct PhaseTimer {
    bool on;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char* what);
};

// What check_scene learns of a valid scene's reference BVH and pack_scene needs again.
struct SceneCheck {
    std::vector<uint32_t> leaf_rank, leaf_order;   // the triangles in left-first DFS order, and the inverse
};

// Validates the scene's indices, lights, spheres and BVH (pt.h, pt_scene: a tree over the triangles with finite,
// nested, bounding boxes, no deeper than bvh_depth says), in one walk of the tree.  Host only, no device needed:
// pt_create runs it before it looks for one.  The scene's null / count checks are pt_create's, before it.
int check_scene(const pt_scene& sc, SceneCheck* out);

// Fills every record of a scene that passed check_scene (checked = its result; null: runs check_scene itself).
int pack_scene(const pt_scene& sc, const RenderKnobs& knobs, PhaseTimer* timer, PackedScene* out, const SceneCheck* checked = nullptr);

}  // namespace pt
