// render_plan.h -- what a render decides on the host before anything is launched (render_plan.cpp): the PT_*
// knobs, the shard's tile grid, the parameter checks and the wavefront kernel's work-unit split.  Plain
// C++17, no HIP: it runs (and is tested) on a machine without a GPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>

#include "pt/pt.h"

namespace pt {

constexpr uint32_t kTile = 8;   // 8x8 = 64 pixels = one wave

// The tuning knobs of a render context, read from the environment once, at pt_create.
struct RenderKnobs {
    uint32_t wf_threshold = 56;     // measured best at 5 waves/SIMD (C3: 24..64 swept)
    uint32_t wf_queues = 8;         // unit counters (PT_WF_QUEUES=1: one; 8: the 1/8 shard +5.8%, C3 +1.2%)
    uint32_t wf_root_first = 4;     // a new ray's first visits (root + up to 3 staged nodes) in the shading pass
                                    // (PT_WF_ROOT_FIRST; C3 1/2/3/4/6: 5331/5417/5461/5509/5406)
    uint32_t wf_waves_per_cu = 16;
    int wf_min_waves = 5;           // register budget of the wavefront kernel (PT_WF_MIN_WAVES: 4/5/6)
    int wf_chunks = 0;              // sample chunks per pixel, 0 = automatic (PT_WF_CHUNKS)
    int wf_tail_chunks = 6;         // chunks of each tail pixel (PT_WF_TAIL_CHUNKS; 1 = no tail split)
    double wf_tail_px = 1.5;        // tail pixels per resident lane (PT_WF_TAIL_PX; round 2 re-sweep after the
                                    // shading-pass fetch merges: C3 0.75 -> 1.5 +4.7%, the 1/2 shard +8%)
    int64_t wf_tail_npix = -1;      // explicit number of tail pixel slots (PT_WF_TAIL_NPIX), -1 = by wf_tail_px
    int wf_mid_chunks = -1;         // split shards: chunks of all but the last pixels (PT_WF_MID_CHUNKS;
                                    // -1 = automatic, 0 or 1 = one split for all)
    double wf_fine_px = 0.5;        // ... the last pixels per resident lane (PT_WF_FINE_PX)
    double wf_whole_px = 0.5;       // split shards with >= wf_whole_min pixels per lane: whole pixels per lane
    double wf_whole_min = 1.25;     // first (PT_WF_WHOLE_PX, PT_WF_WHOLE_MIN)
    int wf_fine_chunks = 0;         // ... and their chunks (PT_WF_FINE_CHUNKS; 0 = the automatic count)
    double wf_fin_px = 0.2;         // final grade: the last pixels per resident lane (PT_WF_FIN_PX) ...
    int wf_fin_chunks = 64;         // ... in this many chunks (PT_WF_FIN_CHUNKS; <= the fine count = off)
                                    // (measured: 1/8 and 1/4 shards +3%, full frame and 1/2 neutral)
    uint32_t wf_iters = 2;          // (PT_WF_ITERS)
    uint32_t wf_top = 0;            // BVH4 nodes staged in each block's LDS (PT_WF_TOP; 0 = none)
    bool wf_lds_tree = true;        // (PT_WF_LDS_TREE)
    bool head_wf = true;            // integrator 1 on the wavefront kernel (PT_HEAD_WF=0: the tile kernel)
    int head_min_waves = 5;         // its register budget (PT_HEAD_MIN_WAVES: 4 = 128 VGPRs, 5 = 96)
    bool use_jump_bytes = true;     // PT_JUMP_BYTES=0: per-bit jumps only
    bool tile_fast4 = true;         // PT_TILE_FAST4=0: the tile kernel walks the reference BVH (culled)
    bool no_light_probe = false;    // PT_NO_LIGHT_PROBE
    bool no_shade_m = false;        // PT_NO_SHADE_M
    // set explicitly (a tree the LDS top holds whole changes only the defaults, pack_scene)
    bool wf_threshold_set = false, wf_root_first_set = false;
};
// The knobs as the environment has them now, with their clamps.  queues: the unit counters PT_WF_QUEUES > 1
// stands for; top_nodes_max: the default and the upper bound of PT_WF_TOP.
RenderKnobs read_render_knobs(uint32_t queues, uint32_t top_nodes_max);

// The padded tile grid of a render and this shard's part of it: tile t (row-major) belongs to shard
// t % shard_count; a tile is tile_w x tile_h work slots in 8x8 blocks.  The field names are Args's (unit_pixel
// in pt_render.hip maps a slot to its pixel from either).
struct TileGrid {
    int32_t w, h, shard_index, shard_count;
    uint32_t tiles_x, tile_w, tile_h;
    uint32_t tile_bx, tile_blocks;   // 8x8 blocks per tile row / per tile
    uint32_t ntiles, ntiles_shard;
    uint32_t npix;                   // work slots of this shard: ntiles_shard * tile_w * tile_h
    uint64_t grid_slots;             // slots of the whole grid; the kernels' unit indices are 32 bits wide:
    bool fits() const { return grid_slots <= 0xffffffffull; }
};
// (p's size, shard and tile fields must already be in range: validate_render's first checks)
TileGrid tile_grid(const pt_params& p);

// What a render's parameters and camera must satisfy whatever the context (pt_render_device_async,
// pt_accum_create and pt_render_features share it).
int validate_render(const pt_params* p, const pt_camera* cam);
// The render-path BVH's box margin assumes ray origins within ~2^6 of the scene extent.
bool near_camera(const pt_camera* cam, float scene_extent);
// Whether a render of (p, cam) takes the wavefront kernels (else render_tiles).
bool takes_wavefront(const pt_params* p, const pt_camera* cam, float scene_extent, bool head_wf);

// The wavefront kernel's launch and its work units (Args has the same names): whole-pixel units first, then
// the `ntail` last pixel slots split into sample chunks in up to three grades (mid, fine, final).
struct UnitPlan {
    uint32_t wpc;          // waves per CU the launch is sized for
    uint32_t top_nodes;    // BVH4 nodes staged in LDS: the scene's, capped by what every block of a CU can hold
    uint32_t blocks;
    uint32_t npix, nwhole, ntail, nmid, chunks_mid, chunks, nfin, chunks_fin, nunits;
};
struct PlanInput {
    int num_cus;
    uint32_t npix;
    int32_t spp;
    bool head, count;
    uint32_t top_nodes;        // of the scene (PackedScene::top_nodes)
    size_t lds_fixed;          // LDS bytes of a block besides the staged nodes
    uint32_t top_node_bytes;   // LDS bytes of a staged node
};
// lbuf_budget: bytes the split pixels' per-sample radiance may take, asked only when pixels are split and
// PT_LBUF_BUDGET_MB (read here, at every render) does not say; its error, if any, is plan_units's.
// npix == 0 (an empty shard) gives the empty plan: nunits = blocks = 0, every chunk count 1, the budget not asked.
int plan_units(const PlanInput& in, const RenderKnobs& k, const std::function<int(uint64_t*)>& lbuf_budget, UnitPlan* out);

// Which instance of the wavefront kernels a render launches: the template arguments of render_unidir_wf /
// render_head_wf (count, min_waves, lds_walk) or their accumulating twins (accum; always 5 waves, never counting).
struct WavefrontVariant {
    bool head, count;
    int min_waves;
    bool lds_walk, accum;
    constexpr uint32_t code() const   // one word per instance, for a switch
    {
        return (uint32_t)head | (uint32_t)count << 1 | (uint32_t)lds_walk << 2 | (uint32_t)accum << 3 | (uint32_t)min_waves << 4;
    }
};
// The instance for a render's integrator (head: 1), PT_FLAG_COUNT, an accumulating pass (never with count), a
// tree held whole in LDS, and the PT_WF_MIN_WAVES / PT_HEAD_MIN_WAVES knobs.  Not every combination has an
// instance of its own: integrator 1 counts at 5 waves and has no LDS walk; integrator 0 counts at 5 waves for
// PT_WF_MIN_WAVES=6, and walks the LDS tree at 5 waves only.  (Internal linkage: the library exports nothing for it.)
static constexpr WavefrontVariant wavefront_variant(bool head, bool count, bool accum, bool lds_tree, int wf_min_waves,
                                                    int head_min_waves)
{
    if (head) {
        if (accum) return {true, false, 5, false, true};
        if (count) return {true, true, 5, false, false};
        return {true, false, head_min_waves == 4 ? 4 : 5, false, false};
    }
    if (accum) return {false, false, 5, lds_tree, true};
    if (count) return wf_min_waves == 4 ? WavefrontVariant{false, true, 4, false, false}
                                        : WavefrontVariant{false, true, 5, lds_tree, false};
    if (wf_min_waves == 6) return {false, false, 6, false, false};
    if (wf_min_waves == 5) return {false, false, 5, lds_tree, false};
    return {false, false, 4, false, false};
}

}  // namespace pt
