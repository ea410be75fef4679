// render_plan.cpp -- the host decisions of a render (render_plan.h): knobs, tile grid, checks, unit split.
#include "render_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "host_internal.h"

namespace pt {

RenderKnobs read_render_knobs(uint32_t queues, uint32_t top_nodes_max)
{
    RenderKnobs k;
    k.wf_queues = queues;
    k.wf_top = top_nodes_max;
    if (const char* e = getenv("PT_WF_THRESHOLD")) { k.wf_threshold = (uint32_t)atoi(e); k.wf_threshold_set = true; }
    if (const char* e = getenv("PT_WF_ROOT_FIRST")) { k.wf_root_first = (uint32_t)atoi(e); k.wf_root_first_set = true; }
    if (const char* e = getenv("PT_WF_QUEUES")) k.wf_queues = (atoi(e) > 1) ? queues : 1u;
    if (const char* e = getenv("PT_JUMP_BYTES")) k.use_jump_bytes = atoi(e) != 0;
    if (const char* e = getenv("PT_TILE_FAST4")) k.tile_fast4 = atoi(e) != 0;
    if (const char* e = getenv("PT_HEAD_WF")) k.head_wf = atoi(e) != 0;
    if (const char* e = getenv("PT_HEAD_MIN_WAVES")) k.head_min_waves = (atoi(e) == 5) ? 5 : 4;
    if (const char* e = getenv("PT_WF_MIN_WAVES")) {
        const int v = atoi(e);
        k.wf_min_waves = (v == 4 || v == 6) ? v : 5;
    }
    k.wf_waves_per_cu = 4u * (uint32_t)k.wf_min_waves;
    if (const char* e = getenv("PT_WF_WAVES_PER_CU")) k.wf_waves_per_cu = (uint32_t)atoi(e);
    if (const char* e = getenv("PT_WF_CHUNKS")) k.wf_chunks = atoi(e);
    if (const char* e = getenv("PT_WF_TAIL_CHUNKS")) k.wf_tail_chunks = atoi(e);
    if (const char* e = getenv("PT_WF_TAIL_PX")) k.wf_tail_px = std::max(0.0, atof(e));
    if (const char* e = getenv("PT_WF_TAIL_NPIX")) k.wf_tail_npix = atoll(e);
    if (const char* e = getenv("PT_WF_MID_CHUNKS")) k.wf_mid_chunks = atoi(e);
    if (const char* e = getenv("PT_WF_FINE_PX")) k.wf_fine_px = std::max(0.0, atof(e));
    if (const char* e = getenv("PT_WF_FINE_CHUNKS")) k.wf_fine_chunks = atoi(e);
    if (const char* e = getenv("PT_WF_WHOLE_PX")) k.wf_whole_px = std::max(0.0, atof(e));
    if (const char* e = getenv("PT_WF_WHOLE_MIN")) k.wf_whole_min = std::max(0.0, atof(e));
    if (const char* e = getenv("PT_WF_FIN_PX")) k.wf_fin_px = std::max(0.0, atof(e));
    if (const char* e = getenv("PT_WF_FIN_CHUNKS")) k.wf_fin_chunks = atoi(e);
    if (const char* e = getenv("PT_WF_ITERS")) k.wf_iters = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("PT_WF_TOP")) k.wf_top = std::min<uint32_t>((uint32_t)std::max(0, atoi(e)), top_nodes_max);
    if (const char* e = getenv("PT_WF_LDS_TREE")) k.wf_lds_tree = atoi(e) != 0;
    k.no_light_probe = getenv("PT_NO_LIGHT_PROBE") != nullptr;
    k.no_shade_m = getenv("PT_NO_SHADE_M") != nullptr;
    return k;
}

TileGrid tile_grid(const pt_params& p)
{
    TileGrid g;
    g.w = p.width; g.h = p.height; g.shard_index = p.shard_index; g.shard_count = p.shard_count;
    g.tile_w = p.tile_w ? (uint32_t)p.tile_w : kTile;
    g.tile_h = p.tile_h ? (uint32_t)p.tile_h : kTile;
    g.tiles_x = ((uint32_t)p.width + g.tile_w - 1) / g.tile_w;
    g.ntiles = g.tiles_x * (((uint32_t)p.height + g.tile_h - 1) / g.tile_h);
    g.tile_bx = g.tile_w / kTile;
    g.tile_blocks = g.tile_bx * (g.tile_h / kTile);
    const uint32_t si = (uint32_t)p.shard_index, sn = (uint32_t)p.shard_count;
    g.ntiles_shard = (g.ntiles > si) ? (g.ntiles - si + sn - 1) / sn : 0u;
    g.npix = g.ntiles_shard * g.tile_w * g.tile_h;
    g.grid_slots = (uint64_t)g.ntiles * g.tile_w * g.tile_h;
    return g;
}

int validate_render(const pt_params* p, const pt_camera* cam)
{
    if (p->width <= 0 || p->height <= 0 || p->width > 65535 || p->height > 65535)
        return fail(PT_E_INVALID, "pt_render: image size %dx%d out of range (1..65535)", p->width, p->height);
    if (p->spp < 0) return fail(PT_E_INVALID, "pt_render: spp < 0");
    if (int rc = validate_jitter_flags("pt_render", p->flags)) return rc;
    if (p->integrator != PT_INTEGRATOR_UNIDIR && p->integrator != PT_INTEGRATOR_HEAD)
        return fail(PT_E_INVALID, "pt_render: unknown integrator %d", p->integrator);
    if (p->integrator == PT_INTEGRATOR_UNIDIR && (p->bounces < 1 || p->bounces > 64))
        return fail(PT_E_INVALID, "pt_render: bounces %d out of range (1..64)", p->bounces);
    if (p->shard_count < 1 || p->shard_index < 0 || p->shard_index >= p->shard_count)
        return fail(PT_E_INVALID, "pt_render: shard %d of %d", p->shard_index, p->shard_count);
    if (cam->pxl_width <= 0 || cam->pxl_height <= 0) return fail(PT_E_INVALID, "pt_render: camera pixel size must be > 0");
    if (p->pixel_order != PT_ORDER_SCANLINE && p->pixel_order != PT_ORDER_MORTON)
        return fail(PT_E_INVALID, "pt_render: unknown pixel order %d", p->pixel_order);
    if (p->pixel_order == PT_ORDER_MORTON && !morton_size_ok(p->width, p->height))
        return fail(PT_E_INVALID, "pt_render: Morton pixel order needs a square power-of-two image, not %dx%d "
                    "(the reference's imgBuff indexing, kernel.cu:543,771)", p->width, p->height);
    for (const int32_t v : {p->tile_w, p->tile_h})
        if (v != 0 && (v < 8 || v > 256 || v % 8 != 0))
            return fail(PT_E_INVALID, "pt_render: tile size %dx%d (0 = 8, else multiples of 8 up to 256)", p->tile_w, p->tile_h);
    // the padded tile grid (tiles x tile_w x tile_h slots) must fit the kernels' 32-bit unit indices
    const TileGrid g = tile_grid(*p);
    if (!g.fits())
        return fail(PT_E_INVALID, "pt_render: %dx%d in %ux%u tiles pads to %llu pixel slots (limit 2^32-1)", p->width, p->height,
                    g.tile_w, g.tile_h, (unsigned long long)g.grid_slots);
    return PT_OK;
}

bool near_camera(const pt_camera* cam, float scene_extent)
{
    const float cam_ext = std::fmax(std::fabs(cam->pos.x), std::fmax(std::fabs(cam->pos.y), std::fabs(cam->pos.z)));
    return cam_ext <= 64.0f * scene_extent;
}

bool takes_wavefront(const pt_params* p, const pt_camera* cam, float scene_extent, bool head_wf)
{
    // integrator 1 takes the wavefront kernel too (PT_HEAD_WF=0: the tile kernel, for comparisons)
    const bool head = p->integrator == PT_INTEGRATOR_HEAD;
    return (p->integrator == PT_INTEGRATOR_UNIDIR || (head && head_wf)) && !(p->flags & PT_FLAG_REFERENCE_TRAVERSAL) &&
           !(p->flags & PT_FLAG_REFERENCE_BVH) && near_camera(cam, scene_extent) &&
           p->width < 65536 && p->height < 65536;   // (16-bit pixel coordinates per unit)
}

int plan_units(const PlanInput& in, const RenderKnobs& k, const std::function<int(uint64_t*)>& lbuf_budget, UnitPlan* out)
{
    const uint32_t wpc = (in.head && !in.count) ? 4u * (uint32_t)k.head_min_waves : k.wf_waves_per_cu;
    uint32_t top_nodes = in.top_nodes;
    {   // as many top nodes as leave every block of a CU its LDS (granted in 1280-B granules): integrator 1's
        // staged light normals cost it one node at 5 blocks per CU (97 -> 96), which kept it at 4 blocks
        const uint32_t bpc = std::max(1u, wpc / 4u);
        const size_t per_block = (size_t)(163840u / bpc) / 1280u * 1280u;
        const uint32_t cap = per_block > in.lds_fixed ? (uint32_t)((per_block - in.lds_fixed) / in.top_node_bytes) : 1u;
        if (top_nodes > 0) top_nodes = std::max(1u, std::min(top_nodes, cap));   // (0: no triangles, no BVH4)
    }
    if (in.npix == 0) {   // an empty shard (more shards than tiles): no unit, no block, nothing to budget
        *out = UnitPlan{};
        out->wpc = wpc;
        out->top_nodes = top_nodes;
        out->chunks = out->chunks_mid = out->chunks_fin = 1;
        return PT_OK;
    }
    uint32_t blocks = (uint32_t)in.num_cus * (wpc / 4 ? wpc / 4 : 1);
    // Work units: a pixel's samples run in sequence, so a unit lasts one pixel's time and the
    // kernel's end waits for the last units started.  Whole pixels first; the last `ntail`
    // pixel slots are split into sample chunks, so the final units are short.
    // A shard with too few pixels to keep every resident lane busy is split entirely.
    const uint32_t npix = in.npix;
    const uint32_t paths_per_block = 256u;
    const uint64_t lanes = (uint64_t)blocks * paths_per_block;   // concurrently running paths
    uint32_t chunks = 1, ntail = 0, nmid = 0, chunks_mid = 1;
    if (k.wf_tail_npix >= 0) {   // (tests: an explicit tail)
        chunks = (uint32_t)(k.wf_chunks > 0 ? k.wf_chunks : k.wf_tail_chunks);
        ntail = (uint32_t)std::min<int64_t>(npix, k.wf_tail_npix);
    } else if (k.wf_chunks > 0) {
        chunks = (uint32_t)k.wf_chunks;
        ntail = npix;
    } else if (2 * (uint64_t)npix < 5 * lanes) {
        // ~16 fine units per lane, at most 8 chunks per pixel (round 2, after the shading pass got
        // cheaper: the 1/8 C3 shard +5..6% with 8 chunks instead of 21 and 4 mid chunks instead of
        // 6, profiles/r02_s4_units; the 1/4 shard alike with 8 or 11)
        chunks = (uint32_t)std::min<uint64_t>((16 * lanes + npix - 1) / npix, 8);
        // longer units first, the finer split for the last wf_fine_px pixels per lane
        // (measured on C3 shards: 1/4 shard 3 mid chunks, 1/8 shard 6: +3..4% over one split)
        const uint32_t nfine = (uint32_t)std::min<uint64_t>(npix, (uint64_t)(k.wf_fine_px * (double)lanes));
        // whole pixels first for wf_whole_px of the lanes when the shard has at least wf_whole_min pixels
        // per lane (a lane's whole pixel is then well within its share of the samples); the rest split
        // (round 5, profiles/r05_whole: the 1/4 shard with 0.3 / 0.5 / 0.7 / 0.9 whole pixels per lane
        // against none: C3 +3.4 / +5.0 / -0.6 / -12%, C4 +3.5 / +5.8 / +1.4%)
        uint32_t nwhole = 0;
        if ((double)npix >= k.wf_whole_min * (double)lanes)
            nwhole = (uint32_t)std::min<uint64_t>(npix - nfine, (uint64_t)(k.wf_whole_px * (double)lanes));
        ntail = npix - nwhole;
        int mc = k.wf_mid_chunks;
        if (mc < 0 && nfine < ntail)   // automatic: ~2.5 mid units per lane, at most 3 chunks
            // (round 5, sample-major split radiance: 3 against 4 at the 1/8 shard, C3 +0.9%, C4 +0.8%,
            // profiles/r05_mid)
            mc = std::min(3, (int)std::ceil(2.5 * (double)lanes / (double)(ntail - nfine)));
        if (mc > 1 && nfine < ntail) {
            nmid = ntail - nfine;
            chunks_mid = (uint32_t)std::min(mc, in.spp);
            if (k.wf_fine_chunks > 0) chunks = (uint32_t)k.wf_fine_chunks;
        }
    } else if (k.wf_tail_chunks > 1) {
        // (measured on C3: +6% with 0.5..1 tail pixel per lane in 4..8 chunks, 0.75 x 6 in round 1;
        // 1.5 x 6 since the shading pass's fetches were merged)
        chunks = (uint32_t)k.wf_tail_chunks;
        ntail = (uint32_t)std::min<uint64_t>(npix, (uint64_t)(k.wf_tail_px * (double)lanes));
    }
    // (measured on C3 shards: whole pixels down to ~3 per lane; below that ~16 units per lane:
    // 1/8 shard 20 chunks, 1/4 shard 10)
    if (chunks > (uint32_t)in.spp) chunks = (uint32_t)in.spp;
    // Split pixels keep their per-sample radiance (lbuf: 24 B per sample), so the split is
    // capped at a memory budget (PT_LBUF_BUDGET_MB; default a quarter of the device memory
    // free now, plus what lbuf already holds): beyond it the first tail slots become whole-pixel
    // units instead (the split only shortens the kernel's tail; results are identical).
    if (ntail > 0 && chunks > 1) {
        uint64_t budget;
        if (const char* e = getenv("PT_LBUF_BUDGET_MB")) {
            budget = (uint64_t)(std::max(0.0, atof(e)) * (double)(1ull << 20));   // (fractional MB kept)
        } else if (int rc = lbuf_budget(&budget)) {
            return rc;
        }
        const uint64_t cap = budget / ((uint64_t)in.spp * 3 * sizeof(double));
        if (ntail > cap) {
            const uint32_t drop = ntail - (uint32_t)cap;   // taken from the front: mid grade first
            nmid = nmid > drop ? nmid - drop : 0;
            ntail = (uint32_t)cap;
        }
    }
    // final grade: the queue's last units shorter still (the kernel ends when the units started
    // last are done), carved from the end of the fine grade
    uint32_t nfin = 0, chunks_fin = 1;
    if (ntail > nmid && k.wf_fin_px > 0.0 && k.wf_fin_chunks > (int)chunks) {
        nfin = (uint32_t)std::min<uint64_t>(ntail - nmid, (uint64_t)(k.wf_fin_px * (double)lanes));
        chunks_fin = (uint32_t)std::min(k.wf_fin_chunks, in.spp);
    }
    if ((uint64_t)npix + (uint64_t)ntail * (std::max(std::max(chunks, chunks_mid), chunks_fin) - 1) > 0xffffffffull)
        chunks = 1;
    if (chunks <= 1 || ntail == 0) { chunks = 1; ntail = 0; nmid = 0; }
    if (nmid == 0) chunks_mid = 1;
    if (ntail == 0 || chunks_fin <= chunks) { nfin = 0; chunks_fin = 1; }
    out->wpc = wpc;
    out->top_nodes = top_nodes;
    out->npix = npix;
    out->chunks = chunks;
    out->ntail = ntail;
    out->nmid = nmid;
    out->chunks_mid = chunks_mid;
    out->nfin = nfin;
    out->chunks_fin = chunks_fin;
    out->nwhole = npix - ntail;
    out->nunits = out->nwhole + nmid * chunks_mid + (ntail - nmid - nfin) * chunks + nfin * chunks_fin;
    const uint32_t need = (out->nunits + paths_per_block - 1) / paths_per_block;
    out->blocks = blocks > need ? need : blocks;
    return PT_OK;
}

}  // namespace pt
