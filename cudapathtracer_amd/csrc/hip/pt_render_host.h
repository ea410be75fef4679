// pt_render_host.h -- the host half of the render translation unit; included once, as the last line of
// pt_render.hip, after every kernel.  The render context (pt_create / pt_destroy of pt_ctx.h's record), a render enqueued in a
// flight slot (render_enqueue, pt_render_wait) and the trace, features and tone-map entry points of
// include/pt/pt.h.  It stays in the kernels' translation unit because Args and the kernels live in that file's
// anonymous namespace; it is a file of its own so that host edits leave the kernel source untouched.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "pt_ctx.h"
#include "pt_hip_util.h"

void pt::sincos_det(float theta, float* s, float* c) { det_sincos(theta, s, c); }

int pt::ctx_device(const pt_ctx* c) { return c->device; }

// Per-lane HBM words the walks may need: the BVH4 ring's overflow (at most 3 pushes per level)
// and trace_slow's full stack on the reference BVH.
static size_t stack_words_per_lane(const pt_ctx* c)
{
    size_t per_lane = (size_t)(3 * c->acc4_depth + 4);
    if (per_lane < (size_t)(2 * (c->depth + 2))) per_lane = (size_t)(2 * (c->depth + 2));
    return per_lane;
}

static bool alloc_bufs(pt_ctx::Bufs& B)
{
    if (B.counters && B.tile_counter && B.pixel_counter) return true;
    // (all three or none: a partial failure is released, so the next call allocates again)
    for (void** q : {reinterpret_cast<void**>(&B.counters), reinterpret_cast<void**>(&B.tile_counter),
                     reinterpret_cast<void**>(&B.pixel_counter)})
        if (*q) { (void)hipFree(*q); *q = nullptr; }
    if (hipMalloc(reinterpret_cast<void**>(&B.counters), kCounterWords * sizeof(unsigned long long)) == hipSuccess &&
        hipMalloc(reinterpret_cast<void**>(&B.tile_counter), 16) == hipSuccess &&
        hipMalloc(reinterpret_cast<void**>(&B.pixel_counter), kQueueStride * (kQueues + 1) * 4) == hipSuccess)
        return true;
    for (void** q : {reinterpret_cast<void**>(&B.counters), reinterpret_cast<void**>(&B.tile_counter),
                     reinterpret_cast<void**>(&B.pixel_counter)})
        if (*q) { (void)hipFree(*q); *q = nullptr; }
    return false;
}

extern "C" {

static bool create_flights(pt_ctx* c)
{
    for (pt_ctx::Flight& f : c->fl) {
        if (hipEventCreate(&f.ev0) != hipSuccess || hipEventCreate(&f.ev1) != hipSuccess ||
            hipEventCreate(&f.ek0) != hipSuccess || hipEventCreate(&f.ek1) != hipSuccess ||
            hipEventCreateWithFlags(&f.done, hipEventDisableTiming) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void**>(&f.hcnt), kCounterWords * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
            return false;
    }
    return true;
}

// The packed scene's arrays on the device, and the per-triangle counters.
static int upload_scene(pt_ctx* c, const pt::PackedScene& P)
{
    int rc = PT_OK;
    if ((rc = pt::upload(&c->nodes, P.nodes)) || (rc = pt::upload(&c->rnodes, P.rnodes)) || (rc = pt::upload(&c->tris_leaf, P.tris_leaf)) ||
        (rc = pt::upload(&c->tris_orig, P.tris_orig)) || (rc = pt::upload(&c->shade, P.shade)) ||
        (!P.shade_m.empty() && (rc = pt::upload(&c->shade_m, P.shade_m))) || (rc = pt::upload(&c->mats, P.mats)) ||
        (rc = pt::upload(&c->lights, P.lights)) || (rc = pt::upload(&c->jump, P.jump)) || (rc = pt::upload(&c->tone_thr, P.tone)) ||
        (rc = pt::upload(&c->spheres, P.spheres)) || (rc = pt::upload(&c->nodes4, P.nodes4)) || (rc = pt::upload(&c->acc_tris, P.acc_tris)) ||
        (rc = pt::upload(&c->rparent, P.rparent)) || (rc = pt::upload(&c->hrec, P.hrec)) ||
        (rc = pt::upload(&c->tri_counts, std::vector<uint32_t>(std::max<uint32_t>(P.num_tris, 1u), 0u))) ||
        (rc = pt::upload(&c->emis, P.emis)))
        return rc;
    return PT_OK;
}

pt_ctx* pt_create(const pt_scene* sc, int device, int* err)
{
    // PT_TIMING=1: host-side phase times on stderr (ingest-speed measurements)
    pt::PhaseTimer timer{getenv("PT_TIMING") != nullptr};
    auto bail = [&](int code) -> pt_ctx* { if (err) *err = code; return nullptr; };
    // the arguments
    if (!sc || (sc->num_tris == 0 && sc->num_spheres == 0) || (sc->num_tris > 0 && (!sc->verts || !sc->tris || !sc->bvh)) ||
        (sc->num_mats > 0 && !sc->mats) ||
        (sc->num_spheres > 0 && !sc->spheres) || (sc->num_lights > 0 && !sc->lights))
        return bail(pt::fail(PT_E_INVALID, "pt_create: incomplete scene"));
    const bool spheres_only = sc->num_tris == 0 && sc->num_spheres > 0 && sc->bvh_size == 0;
    if (!spheres_only && (sc->num_tris < 2 || sc->bvh_size != sc->num_tris - 1))
        return bail(pt::fail(PT_E_SCENE, "pt_create: need >= 2 triangles and a BVH of num_tris-1 nodes, or spheres only "
                             "(got %u tris, %u nodes, %u spheres)", sc->num_tris, sc->bvh_size, sc->num_spheres));
    if (sc->bvh_depth >= PT_MAX_BVH_DEPTH)
        return bail(pt::fail(PT_E_BVH_DEPTH, "Critical Error: BVH depth is too big (%d)", sc->bvh_depth));
    // the scene's indices and its BVH (host only: a scene the walks cannot take is refused with or without a device)
    pt::SceneCheck checked;
    if (int rc = pt::check_scene(*sc, &checked)) return bail(rc);
    timer.lap("scene validation");
    // the device
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bail(pt::fail(PT_E_NODEV, "pt_create: no HIP device"));
    if (device < 0 || device >= ndev) return bail(pt::fail(PT_E_NODEV, "pt_create: device %d out of range (%d)", device, ndev));
    if (hipSetDevice(device) != hipSuccess) return bail(pt::fail(PT_E_HIP, "hipSetDevice(%d) failed", device));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return bail(pt::fail(PT_E_HIP, "hipGetDeviceProperties failed"));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return bail(pt::fail(PT_E_NODEV, "pt_create: device %d is %s, this build targets gfx950", device, prop.gcnArchName));
    // the scene as the kernels read it
    const pt::RenderKnobs knobs = pt::read_render_knobs(kQueues, kTopNodesMax);
    pt::PackedScene P;
    timer.lap("device query");
    if (int rc = pt::pack_scene(*sc, knobs, &timer, &P, &checked)) return bail(rc);
    pt_ctx* c = new (std::nothrow) pt_ctx();
    if (!c) return bail(pt::fail(PT_E_OOM, "pt_create: out of host memory"));
    static_cast<pt::SceneInfo&>(*c) = P;
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    c->knobs = P.knobs;   // (with this scene's defaults of the knobs that were not set)
    // its arrays and the first render's buffers on the device
    if (int rc = upload_scene(c, P)) {
        pt_destroy(c);
        return bail(rc);
    }
    if (!alloc_bufs(c->rb[0]) || !create_flights(c)) {
        pt_destroy(c);
        return bail(pt::fail(PT_E_HIP, "pt_create: device allocation failed"));
    }
    if (err) *err = PT_OK;
    timer.lap("uploads");
    return c;
}

void pt_destroy(pt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    void* bufs[] = {c->nodes, c->rnodes, c->tris_leaf, c->tris_orig, c->shade, c->mats,
                    c->lights, c->jump, c->jump_bytes, c->shade_m, c->scratch_out,
                    c->nodes4, c->acc_tris, c->rparent, c->hrec,
                    c->tone_thr, c->spheres, c->tri_counts, c->emis, c->denoise.mem, c->session.dev, c->query_stage,
                    c->ray_classes, c->rays_stage};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    pt::free_pinned(c->session.host);
    for (pt_ctx::Bufs& B : c->rb)
        for (void* b : {(void*)B.spill, (void*)B.pix_states, (void*)B.lbuf, (void*)B.pmemo, (void*)B.counters,
                        (void*)B.pixel_counter, (void*)B.tile_counter, (void*)B.seed_states})
            if (b) (void)hipFree(b);
    pt::free_pinned(c->pinned);
    if (c->jump_ready) (void)hipEventDestroy(c->jump_ready);
    for (pt_ctx::Flight& f : c->fl) {
        for (hipEvent_t e : {f.ev0, f.ev1, f.ek0, f.ek1, f.done})
            if (e) (void)hipEventDestroy(e);
        if (f.hcnt) (void)hipHostFree(f.hcnt);
    }
    delete c;
}

// PT_LANE_TIMING summary of one wavefront render: wall-clock ticks (100 MHz) from the first wave's start
// to the queue's drain (the first lane without a unit), to the mean and the last lane end, and to the
// last wave exit; idle = the lane-time after each lane's end, as a fraction of lanes x kernel span.
static void write_lane_timing(const char* path, const std::vector<unsigned long long>& t, size_t lanes, int shards)
{
    const size_t waves = lanes / 64;
    unsigned long long t0 = ~0ull, drain = ~0ull, lend = 0, wexit = 0;
    for (size_t w = 0; w < waves; ++w) {
        if (t[lanes + w]) t0 = std::min(t0, t[lanes + w]);
        wexit = std::max(wexit, t[lanes + waves + w]);
    }
    double sum = 0.0;
    size_t n = 0;
    for (size_t l = 0; l < lanes; ++l) {
        if (!t[l]) continue;
        drain = std::min(drain, t[l]);
        lend = std::max(lend, t[l]);
        sum += (double)(t[l] - t0);
        ++n;
    }
    if (!n || t0 == ~0ull) return;
    const double span = (double)(wexit - t0);
    if (FILE* f = fopen(path, "a")) {
        fprintf(f, "lane_timing shards %d lanes %zu span %.0f drain %.0f mean_end %.0f last_end %.0f idle_frac %.4f\n", shards,
                n, span, (double)(drain - t0), sum / (double)n, (double)(lend - t0), 1.0 - (sum / (double)n) / span);
        fclose(f);
    }
}

// The scene half of Args: what every entry point's kernels read of the context's scene.  (Each entry sets its
// own stack_words, node_mask and spill.)
static void fill_scene_args(Args& a, const pt_ctx* c)
{
    a.nodes = c->nodes; a.rnodes = c->rnodes; a.tris_leaf = c->tris_leaf; a.tris_orig = c->tris_orig;
    a.shade = c->shade; a.mats = c->mats; a.lights = c->lights; a.jump = c->jump; a.shade_m = c->shade_m;
    a.num_lights = c->num_lights; a.total_light_area = c->total_light_area;
    a.spheres = c->spheres; a.num_spheres = c->num_spheres; a.num_tris = c->num_tris;
    a.sphere_mat_base = c->sphere_mat_base;
    a.emis = c->emis; a.num_emis = c->num_emis;
    memcpy(a.root, c->root, sizeof(a.root));
    memcpy(a.acc_root, c->acc_root, sizeof(a.acc_root));
    a.cull_rel = kCullRel;
    a.cull_abs = c->scene_extent * 1e-4f;
    a.origin_max = 64.0f * c->scene_extent;
    a.scene_fast = c->scene_fast ? 1u : 0u;
    a.nodes4 = c->nodes4;
    a.acc_tris = c->acc_tris;
    a.rparent = c->rparent;
    a.hrec = c->hrec;
}

// The camera, its view (null: the reference camera), the image and this shard's tile grid (validated parameters).
static void fill_view_args(Args& a, const pt_params& p, const pt_camera& cam, const pt_view* view)
{
    a.cam.pos[0] = cam.pos.x; a.cam.pos[1] = cam.pos.y; a.cam.pos[2] = cam.pos.z;
    a.cam.dist = cam.dist_from_film; a.cam.focal = cam.focal_length; a.cam.radius = cam.radius;
    a.cam.w = cam.pxl_width; a.cam.h = cam.pxl_height;
    a.oriented = view ? 1u : 0u;
    if (view) {
        memcpy(a.view_right, view->right, sizeof(a.view_right));
        memcpy(a.view_up, view->up, sizeof(a.view_up));
        memcpy(a.view_back, view->back, sizeof(a.view_back));
        a.film_w = view->film_w;
        a.film_h = view->film_h;
    }
    const pt::TileGrid g = pt::tile_grid(p);
    a.w = g.w; a.h = g.h;
    a.shard_index = g.shard_index; a.shard_count = g.shard_count;
    a.tiles_x = g.tiles_x; a.ntiles_shard = g.ntiles_shard;
    a.tile_w = g.tile_w; a.tile_h = g.tile_h;
    a.tile_bx = g.tile_bx; a.tile_blocks = g.tile_blocks;
    a.morton_out = (p.pixel_order == PT_ORDER_MORTON) ? 1u : 0u;
    a.npix = g.npix;
}

// ---- a render, step by step.  Each step enqueues on the render's stream; render_enqueue below is their order.

// The counters a render that does not go through init_pixel_states starts from.
static int reset_counters(const pt_ctx::Bufs& B, hipStream_t stream)
{
    HIP_TRY(hipMemsetAsync(B.counters, 0, kCounterWords * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(B.counters + CNT_T_START, 0xff, 2 * sizeof(unsigned long long), stream));   // (atomicMin slots)
    HIP_TRY(hipMemsetAsync(B.tile_counter, 0, 16, stream));
    HIP_TRY(hipMemsetAsync(B.pixel_counter, 0, kQueueStride * (kQueues + 1) * 4, stream));
    return PT_OK;
}

// The byte-position jump matrices, once per context: 512 byte-sliced 160x160 GF(2) matrices (84 MB), built on the
// stream of the first render that needs them; every later render waits for the build (jump_ready).
static int ensure_jump_tables(pt_ctx* c, hipStream_t stream)
{
    if (c->jump_bytes) {
        HIP_TRY(hipStreamWaitEvent(stream, c->jump_ready, 0));
        return PT_OK;
    }
    // (built into a local and published only once the build launched: a failure leaves the context without
    // tables, so the next render tries again instead of seeding from garbage)
    uint32_t* jb = nullptr;
    const bool ok = hipMalloc(reinterpret_cast<void**>(&jb), (size_t)512 * 20 * 256 * kJumpEntryWords * 4) == hipSuccess &&
                    (c->jump_ready || hipEventCreateWithFlags(&c->jump_ready, hipEventDisableTiming) == hipSuccess);
    if (ok) hipLaunchKernelGGL(build_jump_byte_tables, dim3(512 * 20), dim3(256), 0, stream, c->jump, jb);
    if (!ok || hipGetLastError() != hipSuccess || hipEventRecord(c->jump_ready, stream) != hipSuccess) {
        if (jb) (void)hipFree(jb);
        return pt::fail(ok ? PT_E_HIP : PT_E_OOM, "pt_render: jump-table setup failed");
    }
    c->jump_bytes = jb;
    return PT_OK;
}

// The slot's seed table for args.seed (it depends on the seed only: kept across renders).  *seeded: seed_table was
// enqueued now.  The slot is left marked invalid: the caller marks it valid only once the whole render is
// enqueued, so any error return in between leaves it unseeded and the next render seeds again instead of trusting
// a table never written.
static int ensure_seed_table(pt_ctx::Bufs& B, const Args& args, hipStream_t stream, bool* seeded)
{
    if (!B.seed_states) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&B.seed_states), (size_t)256 * kJumpEntryWords * 4));
        B.seed_valid = false;
    }
    if (B.seed_valid && B.seed_cached == args.seed) return PT_OK;
    B.seed_valid = false;
    hipLaunchKernelGGL(seed_table, dim3(1), dim3(256), 0, stream, args, B.seed_states);
    HIP_TRY(hipGetLastError());
    *seeded = true;
    return PT_OK;
}

// The wavefront launch of one render: what plan_wavefront decides besides the unit fields of Args.
struct WavefrontLaunch {
    uint32_t blocks = 0;     // of 256 threads, 4 waves
    size_t lds = 0;          // dynamic LDS bytes of a block
    bool lds_tree = false;   // the whole tree staged in LDS
};

// The launch and the work units (render_plan.cpp) of a wavefront render, written into b, and the slot's buffers
// the units need, grown on demand.  b comes in as a copy of the render's Args.
static int plan_wavefront(const pt_ctx* c, const pt_params* p, const pt::AccumPass* acc, pt_ctx::Bufs& B, Args& b,
                          WavefrontLaunch* L)
{
    const pt::RenderKnobs& K = c->knobs;
    const bool head = p->integrator == PT_INTEGRATOR_HEAD;
    // 4 waves per block; per wave an LDS ring of kRing packed entries x 64 lanes, deeper
    // entries spill to HBM (a BVH4 walk pushes at most 3 entries per level)
    b.stack_words = kRing * 64;
    b.node_mask = c->node4_mask;
    b.head = head ? 1u : 0u;
    pt::PlanInput in;
    in.num_cus = c->num_cus; in.npix = b.npix; in.spp = p->spp; in.head = head; in.count = (p->flags & PT_FLAG_COUNT) != 0;
    in.top_nodes = c->top_nodes;
    in.lds_fixed = (size_t)kWaveLdsWords * 4 * 4 + 4 * sizeof(unsigned long long) + (kSections + kHist) * 4 +
                   kProbeLdsBytes + (head ? (size_t)kHeadLdsLightBytes : 0);
    in.top_node_bytes = kTopNodeBytes;
    pt::UnitPlan plan;
    // (default budget: a quarter of the device memory free now, plus what lbuf already holds)
    auto lbuf_budget = [&B](uint64_t* bytes) -> int {
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        *bytes = ((uint64_t)fr + (uint64_t)B.lbuf_words * sizeof(double)) / 4;
        return PT_OK;
    };
    if (acc && acc->active) in.npix = acc->nactive;   // (the launch is sized by the units it has)
    if (int rc = pt::plan_units(in, K, lbuf_budget, &plan)) return rc;
    if (acc && acc->active) {
        // an adaptive pass: unit u = the whole pixel of slot active[u], no sample-chunk split (npix stays the
        // shard's slot count: the stride of the accumulator's planes)
        if (acc->nactive == 0 || acc->nactive > b.npix) return pt::fail(PT_E_INVALID, "pt_accum_add: active list of %u slots", acc->nactive);
        plan.nwhole = plan.nunits = acc->nactive;
        plan.ntail = plan.nmid = plan.nfin = 0;
        plan.chunks = plan.chunks_mid = plan.chunks_fin = 1;
        plan.blocks = std::min(plan.blocks, (acc->nactive + 255u) / 256u);
    }
    const uint32_t blocks = plan.blocks, ntail = plan.ntail;
    const uint32_t paths_per_block = 256u;
    b.top_nodes = plan.top_nodes;
    b.nwhole = plan.nwhole; b.ntail = plan.ntail; b.nmid = plan.nmid; b.chunks_mid = plan.chunks_mid;
    b.chunks = plan.chunks; b.nfin = plan.nfin; b.chunks_fin = plan.chunks_fin; b.nunits = plan.nunits;
    L->blocks = blocks;
    L->lds = in.lds_fixed + (size_t)b.top_nodes * kTopNodeBytes;
    // the whole tree staged in LDS (small scenes: C2): integrator 0's walk steps read it there too
    // (PT_WF_LDS_TREE=0: memory loads, as for a tree larger than the top)
    L->lds_tree = K.wf_lds_tree && c->n4 > 0 && b.top_nodes >= c->n4;
    // (C2: 7181 with the record's second fetch against 7267 by triangle id; C3 the other way)
    b.rec_shading = L->lds_tree ? 0u : 1u;
    if (ntail > 0) {
        if (int rc = pt::grow(&B.lbuf, &B.lbuf_words, (size_t)ntail * (size_t)p->spp * 3)) return rc;
        if (int rc = pt::grow(&B.pmemo, &B.pmemo_words, (size_t)ntail * 2)) return rc;
        b.lbuf = B.lbuf;
        b.pmemo = B.pmemo;
    }
    const size_t per_lane = stack_words_per_lane(c);
    const size_t rec_words = head ? (size_t)kHeadWords : (size_t)kColdWords;   // shading record per lane
    if (int rc = pt::grow(&B.spill, &B.spill_words, per_lane * (size_t)blocks * 256 + rec_words * (size_t)blocks * paths_per_block))
        return rc;
    b.spill = B.spill;
    b.spill_stride = blocks * 256;
    b.cold_stride = blocks * paths_per_block;
    b.cold = B.spill + per_lane * (size_t)b.spill_stride;
    if (int rc = pt::grow(&B.pix_states, &B.pix_states_words, (size_t)kUnitWords * b.nunits)) return rc;
    b.pix_states = B.pix_states;
    return PT_OK;
}

// Diagnostic (PT_LANE_TIMING=file): per-lane end / per-wave start and exit times of one wavefront render, summarised
// into the file.  It owns the device buffer, which is freed on every path out of the render.
namespace {
struct LaneTiming {
    const char* path = getenv("PT_LANE_TIMING");
    std::vector<unsigned long long> times;
    pt::ScopedDevice<unsigned long long> d_times;

    int begin(uint32_t blocks, hipStream_t stream, Args& b)
    {
        if (!path) return PT_OK;
        times.assign((size_t)blocks * 256 + 2 * (size_t)blocks * 4, 0ull);
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_times), times.size() * 8));
        HIP_TRY(hipMemsetAsync(d_times, 0, times.size() * 8, stream));
        b.lane_times = d_times;
        return PT_OK;
    }
    // (waits for the render: the times are read here)
    int finish(uint32_t blocks, hipStream_t stream, int shards)
    {
        if (!path) return PT_OK;
        HIP_TRY(hipMemcpyAsync(times.data(), d_times, times.size() * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        write_lane_timing(path, times, (size_t)blocks * 256, shards);
        return PT_OK;
    }
};
}  // namespace

// The integration kernel of a wavefront render: the instance pt::wavefront_variant names.  An oriented render
// (b.oriented) of integrator 0 takes that instance's view twin; integrator 1's instances serve both.  A jittered
// render (PT_FLAG_JITTER) takes the instance's jitter twin, which serves both cameras.
// A render along a caller's rays (rays != null) takes the ray-source instance, whose argument block is b with the
// buffer appended (RayArgs); points: the buffer holds points {p, n} and the render is an irradiance render, which
// takes the point-source instance.
static int launch_wavefront(const pt::WavefrontVariant& v, const WavefrontLaunch& L, hipStream_t stream, const Args& b,
                            const float* rays = nullptr, bool points = false)
{
    constexpr auto code = [](bool head, bool count, int min_waves, bool lds_walk, bool accum) {
        return pt::WavefrontVariant{head, count, min_waves, lds_walk, accum}.code();
    };
    void (*kernel)(Args) = nullptr;
    switch (v.code()) {   // (keep the cases' order: the compiler emits the instances in the order of their first use)
    case code(true, false, 5, false, true): kernel = render_head_accum_wf; break;
    case code(false, false, 5, true, true): kernel = render_unidir_accum_wf<true>; break;
    case code(false, false, 5, false, true): kernel = render_unidir_accum_wf<false>; break;
    case code(true, true, 5, false, false): kernel = render_head_wf<true, 5>; break;
    case code(true, false, 4, false, false): kernel = render_head_wf<false, 4>; break;
    case code(true, false, 5, false, false): kernel = render_head_wf<false, 5>; break;
    case code(false, true, 4, false, false): kernel = render_unidir_wf<true, 4>; break;
    case code(false, true, 5, true, false): kernel = render_unidir_wf<true, 5, true>; break;
    case code(false, true, 5, false, false): kernel = render_unidir_wf<true, 5>; break;
    case code(false, false, 6, false, false): kernel = render_unidir_wf<false, 6>; break;
    case code(false, false, 5, true, false): kernel = render_unidir_wf<false, 5, true>; break;
    case code(false, false, 5, false, false): kernel = render_unidir_wf<false, 5>; break;
    case code(false, false, 4, false, false): kernel = render_unidir_wf<false, 4>; break;
    default:
        return pt::fail(PT_E_INVALID, "pt_render: no wavefront kernel instance for head %d count %d waves %d lds %d accum %d",
                        v.head, v.count, v.min_waves, v.lds_walk, v.accum);
    }
    if (b.oriented && !v.head) {   // (below every plain instance, so that those are emitted first, as they were)
        switch (v.code()) {
        case code(false, false, 5, true, true): kernel = render_unidir_accum_view_wf<true>; break;
        case code(false, false, 5, false, true): kernel = render_unidir_accum_view_wf<false>; break;
        case code(false, true, 4, false, false): kernel = render_unidir_view_wf<true, 4>; break;
        case code(false, true, 5, true, false): kernel = render_unidir_view_wf<true, 5, true>; break;
        case code(false, true, 5, false, false): kernel = render_unidir_view_wf<true, 5>; break;
        case code(false, false, 6, false, false): kernel = render_unidir_view_wf<false, 6>; break;
        case code(false, false, 5, true, false): kernel = render_unidir_view_wf<false, 5, true>; break;
        case code(false, false, 5, false, false): kernel = render_unidir_view_wf<false, 5>; break;
        case code(false, false, 4, false, false): kernel = render_unidir_view_wf<false, 4>; break;
        default:
            return pt::fail(PT_E_INVALID, "pt_render: no oriented wavefront kernel instance for count %d waves %d lds %d accum %d",
                            v.count, v.min_waves, v.lds_walk, v.accum);
        }
    }
    if (b.flags & PT_FLAG_JITTER) {   // (the jitter twins: below every other instance, for the same reason)
        switch (v.code()) {
        case code(true, false, 5, false, true): kernel = render_head_accum_jitter_wf; break;
        case code(false, false, 5, true, true): kernel = render_unidir_accum_jitter_wf<true>; break;
        case code(false, false, 5, false, true): kernel = render_unidir_accum_jitter_wf<false>; break;
        case code(true, true, 5, false, false): kernel = render_head_jitter_wf<true, 5>; break;
        case code(true, false, 4, false, false): kernel = render_head_jitter_wf<false, 4>; break;
        case code(true, false, 5, false, false): kernel = render_head_jitter_wf<false, 5>; break;
        case code(false, true, 4, false, false): kernel = render_unidir_jitter_wf<true, 4>; break;
        case code(false, true, 5, true, false): kernel = render_unidir_jitter_wf<true, 5, true>; break;
        case code(false, true, 5, false, false): kernel = render_unidir_jitter_wf<true, 5>; break;
        case code(false, false, 6, false, false): kernel = render_unidir_jitter_wf<false, 6>; break;
        case code(false, false, 5, true, false): kernel = render_unidir_jitter_wf<false, 5, true>; break;
        case code(false, false, 5, false, false): kernel = render_unidir_jitter_wf<false, 5>; break;
        case code(false, false, 4, false, false): kernel = render_unidir_jitter_wf<false, 4>; break;
        default:
            return pt::fail(PT_E_INVALID, "pt_render: no jittered wavefront kernel instance for head %d count %d waves %d lds %d accum %d",
                            v.head, v.count, v.min_waves, v.lds_walk, v.accum);
        }
    }
    if (rays && !points) {   // (the ray-source instances, default occupancy only: below every other instance again)
        void (*rkernel)(RayArgs) = nullptr;
        switch (v.code()) {
        case code(true, false, 5, false, false): rkernel = render_head_rays_wf; break;
        case code(false, false, 5, true, false): rkernel = render_unidir_rays_wf<true>; break;
        case code(false, false, 5, false, false): rkernel = render_unidir_rays_wf<false>; break;
        case code(true, false, 5, false, true): rkernel = render_head_accum_rays_wf; break;   // (a ray accumulator's passes)
        case code(false, false, 5, true, true): rkernel = render_unidir_accum_rays_wf<true>; break;
        case code(false, false, 5, false, true): rkernel = render_unidir_accum_rays_wf<false>; break;
        default:
            return pt::fail(PT_E_INVALID, "pt_render_rays: no ray-source wavefront kernel instance for head %d count %d waves %d lds %d "
                            "accum %d (only the default PT_WF_MIN_WAVES / PT_HEAD_MIN_WAVES have one)",
                            v.head, v.count, v.min_waves, v.lds_walk, v.accum);
        }
        RayArgs rb;
        static_cast<Args&>(rb) = b;
        rb.rays = rays;
        hipLaunchKernelGGL(rkernel, dim3(L.blocks), dim3(256), L.lds, stream, rb);
        HIP_TRY(hipGetLastError());
        return PT_OK;
    }
    if (rays) {   // (the point-source instances of an irradiance render: default occupancy only)
        void (*pkernel)(RayArgs) = nullptr;
        switch (v.code()) {
        case code(true, false, 5, false, false): pkernel = render_head_points_wf; break;
        case code(false, false, 5, true, false): pkernel = render_unidir_points_wf<true>; break;
        case code(false, false, 5, false, false): pkernel = render_unidir_points_wf<false>; break;
        case code(true, false, 5, false, true): pkernel = render_head_accum_points_wf; break;   // (a point accumulator's passes)
        case code(false, false, 5, true, true): pkernel = render_unidir_accum_points_wf<true>; break;
        case code(false, false, 5, false, true): pkernel = render_unidir_accum_points_wf<false>; break;
        default:
            return pt::fail(PT_E_INVALID, "%s: no point-source wavefront kernel instance for head %d count %d waves "
                            "%d lds %d accum %d (only the default PT_WF_MIN_WAVES / PT_HEAD_MIN_WAVES have one)",
                            v.accum ? "pt_accum_add" : "pt_render_irradiance", v.head, v.count, v.min_waves, v.lds_walk, v.accum);
        }
        RayArgs rb;
        static_cast<Args&>(rb) = b;
        rb.rays = rays;
        hipLaunchKernelGGL(pkernel, dim3(L.blocks), dim3(256), L.lds, stream, rb);
        HIP_TRY(hipGetLastError());
        return PT_OK;
    }
    hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(256), L.lds, stream, b);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// The tile kernel of a render the wavefront kernels do not take: one wave per 8x8 block of the shard's tiles.
// (rays: a render along a caller's rays; rays_refwalk: it takes the reference's own walk -- an irregular buffer or
// one of the two reference flags; points: the buffer holds the points of an irradiance render)
static int launch_tiles(const pt_ctx* c, const pt_params* p, pt_ctx::Bufs& B, size_t lds, hipStream_t stream, Args& a,
                        const float* rays, bool rays_refwalk, bool points)
{
    uint32_t grid = (uint32_t)c->num_cus * 16;   // waves per CU
    if (grid > a.ntiles_shard * a.tile_blocks) grid = a.ntiles_shard > 0 ? a.ntiles_shard * a.tile_blocks : 1;
    if (a.tile_fast4) {   // the BVH4 walk's ring overflow and the slow walk's stack: one HBM column per lane
        if (int rc = pt::grow(&B.spill, &B.spill_words, stack_words_per_lane(c) * (size_t)grid * 64)) return rc;
        a.spill = B.spill;
        a.spill_stride = grid * 64;
    }
    const bool refwalk = (p->flags & PT_FLAG_REFERENCE_TRAVERSAL) != 0, count = (p->flags & PT_FLAG_COUNT) != 0;
    // (the instances in this order: the order of first use is the order the compiler emits them in)
#define PT_LAUNCH(I, R, C) hipLaunchKernelGGL((render_tiles<I, R, C>), dim3(grid), dim3(64), lds, stream, a)
#define PT_LAUNCH_VIEW(I, R, C) hipLaunchKernelGGL((render_tiles_view<I, R, C>), dim3(grid), dim3(64), lds, stream, a)
#define PT_LAUNCH_JITTER(I, R, C) hipLaunchKernelGGL((render_tiles_jitter<I, R, C>), dim3(grid), dim3(64), lds, stream, a)
#define PT_LAUNCH_RAYS(I, R) hipLaunchKernelGGL((render_tiles_rays<I, R, false>), dim3(grid), dim3(64), lds, stream, ra)
#define PT_LAUNCH_POINTS(I, R) hipLaunchKernelGGL((render_tiles_points<I, R, false>), dim3(grid), dim3(64), lds, stream, ra)
    const bool jitter = (p->flags & PT_FLAG_JITTER) != 0;
    if (rays) {
        // (the ray-source instances: run only here, and first used below every other instance)
    } else if (!a.oriented && !jitter) {
    if (p->integrator == PT_INTEGRATOR_HEAD) {
        if (refwalk) { if (count) PT_LAUNCH(1, true, true); else PT_LAUNCH(1, true, false); }
        else { if (count) PT_LAUNCH(1, false, true); else PT_LAUNCH(1, false, false); }
    } else {
        if (refwalk) { if (count) PT_LAUNCH(0, true, true); else PT_LAUNCH(0, true, false); }
        else { if (count) PT_LAUNCH(0, false, true); else PT_LAUNCH(0, false, false); }
    }
    } else if (!jitter && p->integrator == PT_INTEGRATOR_HEAD) {   // (the view's instances: after every plain one)
        if (refwalk) { if (count) PT_LAUNCH_VIEW(1, true, true); else PT_LAUNCH_VIEW(1, true, false); }
        else { if (count) PT_LAUNCH_VIEW(1, false, true); else PT_LAUNCH_VIEW(1, false, false); }
    } else if (!jitter) {
        if (refwalk) { if (count) PT_LAUNCH_VIEW(0, true, true); else PT_LAUNCH_VIEW(0, true, false); }
        else { if (count) PT_LAUNCH_VIEW(0, false, true); else PT_LAUNCH_VIEW(0, false, false); }
    } else if (p->integrator == PT_INTEGRATOR_HEAD) {   // (the jittered instances, either camera: after every other one)
        if (refwalk) { if (count) PT_LAUNCH_JITTER(1, true, true); else PT_LAUNCH_JITTER(1, true, false); }
        else { if (count) PT_LAUNCH_JITTER(1, false, true); else PT_LAUNCH_JITTER(1, false, false); }
    } else {
        if (refwalk) { if (count) PT_LAUNCH_JITTER(0, true, true); else PT_LAUNCH_JITTER(0, true, false); }
        else { if (count) PT_LAUNCH_JITTER(0, false, true); else PT_LAUNCH_JITTER(0, false, false); }
    }
    if (rays && !points) {
        RayArgs ra;
        static_cast<Args&>(ra) = a;
        ra.rays = rays;
        if (p->integrator == PT_INTEGRATOR_HEAD) { if (rays_refwalk) PT_LAUNCH_RAYS(1, true); else PT_LAUNCH_RAYS(1, false); }
        else { if (rays_refwalk) PT_LAUNCH_RAYS(0, true); else PT_LAUNCH_RAYS(0, false); }
    } else if (rays) {   // (the point-source instances: below the ray-source ones)
        RayArgs ra;
        static_cast<Args&>(ra) = a;
        ra.rays = rays;
        if (p->integrator == PT_INTEGRATOR_HEAD) { if (rays_refwalk) PT_LAUNCH_POINTS(1, true); else PT_LAUNCH_POINTS(1, false); }
        else { if (rays_refwalk) PT_LAUNCH_POINTS(0, true); else PT_LAUNCH_POINTS(0, false); }
    }
#undef PT_LAUNCH_POINTS
#undef PT_LAUNCH_RAYS
#undef PT_LAUNCH_JITTER
#undef PT_LAUNCH_VIEW
#undef PT_LAUNCH
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// What enqueue_wavefront reports to the render's flight slot.
struct WavefrontDone {
    uint64_t units = 0, split = 0;
    bool seeded = false;     // seed_table enqueued for this render's seed
};

// The wavefront path of one render, from its plan to finalize_pixels.  a: the render's Args; F: its flight slot.
// (rays: a render along a caller's rays, or null; points: the buffer holds the points of an irradiance render or of a
// point accumulator)
static int enqueue_wavefront(pt_ctx* c, const pt_params* p, const pt::AccumPass* acc, const Args& a, pt_ctx::Flight& F,
                             pt_ctx::Bufs& B, hipStream_t stream, WavefrontDone* done, const float* rays, bool points)
{
    const pt::RenderKnobs& K = c->knobs;
    Args b = a;
    WavefrontLaunch L;
    if (int rc = plan_wavefront(c, p, acc, B, b, &L)) return rc;
    LaneTiming timing;
    if (int rc = timing.begin(L.blocks, stream, b)) return rc;
    if (K.use_jump_bytes) {
        if (int rc = ensure_jump_tables(c, stream)) return rc;
        if (int rc = ensure_seed_table(B, b, stream, &done->seeded)) return rc;
        b.jump_bytes = c->jump_bytes;
        b.seed_states = B.seed_states;
    }
    const bool jitter = (b.flags & PT_FLAG_JITTER) != 0;   // (its set-up kernels mark every unit "ray formed per sample")
    if (acc && acc->active && !rays)
        hipLaunchKernelGGL(jitter ? init_active_states_jitter : init_active_states, dim3((b.nunits + 255) / 256), dim3(256), 0,
                           stream, b, B.pix_states, acc->active);
    else if (acc && acc->active) {   // (an adaptive pass of a ray accumulator: the active set-up's ray twin)
        RayArgs rb;
        static_cast<Args&>(rb) = b;
        rb.rays = rays;
        // (points: a point accumulator's, whose every unit is a lens unit)
        hipLaunchKernelGGL(points ? init_active_states_points : init_active_states_rays, dim3((b.nunits + 255) / 256), dim3(256), 0,
                           stream, rb, B.pix_states, acc->active);
    } else if (!rays)
        hipLaunchKernelGGL(jitter ? init_pixel_states_jitter : init_pixel_states, dim3((b.npix + 255) / 256), dim3(256), 0, stream,
                           b, B.pix_states);
    else {   // (a render along rays: the set-up that reads each unit's direction from the buffer)
        RayArgs rb;
        static_cast<Args&>(rb) = b;
        rb.rays = rays;
        if (points) hipLaunchKernelGGL(init_pixel_states_points, dim3((b.npix + 255) / 256), dim3(256), 0, stream, rb, B.pix_states);
        else hipLaunchKernelGGL(init_pixel_states_rays, dim3((b.npix + 255) / 256), dim3(256), 0, stream, rb, B.pix_states);
    }
    // A render queued on another stream while one is in flight: its seeding pre-pass runs beside the
    // earlier render's last waves (its own buffers), but the integration kernel waits until the earlier
    // render is complete (finalisation included), so a persistent grid never takes the CU slots an
    // earlier frame's finalisation needs (that one would otherwise wait out the whole next frame)
    if (c->fl_n > 0) HIP_TRY(hipStreamWaitEvent(stream, c->fl[(c->fl_head + c->fl_n - 1) % pt_ctx::kFlights].ev1, 0));
    HIP_TRY(hipEventRecord(F.ek0, stream));
    done->units = b.nunits;
    done->split = b.ntail;
    const pt::WavefrontVariant v = pt::wavefront_variant(b.head != 0, (p->flags & PT_FLAG_COUNT) != 0, acc != nullptr, L.lds_tree,
                                                         K.wf_min_waves, K.head_min_waves);
    if (int rc = launch_wavefront(v, L, stream, b, rays, points)) return rc;
    HIP_TRY(hipEventRecord(F.ek1, stream));
    if (b.ntail > 0) hipLaunchKernelGGL(finalize_pixels, dim3((b.ntail + 255) / 256), dim3(256), 0, stream, b);
    HIP_TRY(hipGetLastError());
    return timing.finish(L.blocks, stream, p->shard_count);
}

// One render enqueued on `stream` in the context's next flight slot: the body of pt_render_device_async.
// acc: the render is a pass of an accumulator (pt::accum_pass) -- p->spp more samples of every pixel on top
// of its acc->n0, from and to the accumulator's state; d_out may then be null.  Everything else -- the
// unit split, the buffers' growth, the jump and seed tables, the flight slots -- is the plain render's.
// d_rays: a render along the caller's rays (pt_render_rays_device, which has classified them, or a pass of a ray
// accumulator, whose rays were classified when it was created; cam is then a stand-in that only carries the image
// size); rays_irregular: the buffer holds an irregular ray, so the whole render
// takes the tile kernel with the reference's own walk.  points: d_rays holds the points {p, n} of an irradiance render
// (pt_render_irradiance_device) or of a point accumulator's pass, classified likewise.
static int render_enqueue(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, float* d_out, void* stream_v,
                          const pt::AccumPass* acc, const float* d_rays = nullptr, bool rays_irregular = false, bool points = false)
{
    if (!c || !p || !cam || (!d_out && !acc)) return pt::fail(PT_E_INVALID, "pt_render: null argument");
    if (c->fl_n >= pt_ctx::kFlights)
        return pt::fail(PT_E_INVALID, "pt_render_device_async: %d renders in flight (pt_render_wait first)", c->fl_n);
    if (int rc = pt::validate_render(p, cam)) return rc;
    if (view)
        if (int rc = pt::validate_view("pt_render", view)) return rc;
    // the per-triangle counts live in one context-wide buffer (pt_tri_counts reads it back): only one render
    // in flight may fill them
    if ((p->flags & PT_FLAG_COUNT) && (p->flags & PT_FLAG_TRI_COUNTS) && c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_render_device_async: PT_FLAG_TRI_COUNTS while a render is in flight");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    // this render's slot: its events and its buffer set.  The slot's previous render was collected by
    // pt_render_wait (its events synchronised), so two queued renders -- on one stream or on two, where
    // they may run concurrently -- never share a buffer.
    const int slot = (c->fl_head + c->fl_n) % pt_ctx::kFlights;
    pt_ctx::Flight& F = c->fl[slot];
    pt_ctx::Bufs& B = c->rb[slot];
    if (!alloc_bufs(B)) return pt::fail(PT_E_HIP, "pt_render: device allocation failed");
    const pt::RenderKnobs& K = c->knobs;

    // the arguments every kernel of this render shares
    Args a;
    memset(&a, 0, sizeof(a));
    fill_scene_args(a, c);
    fill_view_args(a, *p, *cam, view);
    a.out = d_out; a.counters = B.counters; a.tile_counter = B.tile_counter;
    a.spp = p->spp; a.bounces = p->bounces; a.flags = p->flags; a.seed = p->seed;
    const bool count = (p->flags & PT_FLAG_COUNT) != 0;
    const uint32_t levels = (uint32_t)c->depth + 2;
    a.stack_words = std::max<uint32_t>(levels * 128, (uint32_t)kWaveLdsWords);   // (culled walk's stack, or the BVH4 rings)
    const size_t lds = (size_t)a.stack_words * 4;
    // (not reachable while pt_create caps bvh_depth at PT_MAX_BVH_DEPTH - 1 = 63: this limit starts at depth 319)
    static_assert((size_t)(PT_MAX_BVH_DEPTH - 1 + 2) * 128 * 4 <= 160 * 1024, "every depth pt_create accepts fits the LDS stack");
    if (lds > 160 * 1024) return pt::fail(PT_E_BVH_DEPTH, "pt_render: BVH depth %d needs %zu B of LDS stack", c->depth, lds);
    a.pixel_counter = B.pixel_counter;
    a.nunits = a.npix;
    a.wf_threshold = K.wf_threshold;
    a.root_first = K.wf_root_first;
    a.unit_queues = K.wf_queues;
    a.wf_iters = K.wf_iters;
    a.node_mask = c->node_mask;
    // the tile kernel traces with the render-path BVH4 walk under the wavefront kernel's conditions
    // (PT_TILE_FAST4=0: the reference-BVH culled walk, as before)
    a.tile_fast4 = (!(p->flags & (PT_FLAG_REFERENCE_TRAVERSAL | PT_FLAG_REFERENCE_BVH)) && pt::near_camera(cam, c->scene_extent) &&
                    !rays_irregular && K.tile_fast4 && c->num_tris > 0) ? 1u : 0u;
    const bool wavefront = pt::takes_wavefront(p, cam, c->scene_extent, K.head_wf) && !rays_irregular;
    const bool rays_refwalk = d_rays && (rays_irregular || (p->flags & (PT_FLAG_REFERENCE_TRAVERSAL | PT_FLAG_REFERENCE_BVH)) != 0);
    if (d_rays && wavefront && (K.wf_min_waves != 5 || K.head_min_waves != 5))   // (never another kernel in silence)
        return pt::fail(PT_E_INVALID, "%s: only the default-occupancy wavefront kernels take a %s buffer "
                        "(PT_WF_MIN_WAVES / PT_HEAD_MIN_WAVES are set)", points ? "pt_render_irradiance" : "pt_render_rays",
                        points ? "point" : "ray");
    if (acc) {   // (pt_accum_create refused these already: never a silent fall-back to another kernel)
        if (!wavefront || count || K.wf_min_waves != 5 || K.head_min_waves != 5)
            return pt::fail(PT_E_INVALID, "pt_accum_add: this mode has no accumulating kernel");
        if ((uint64_t)acc->n0 + (uint64_t)p->spp > kAccumMaxSamples)
            return pt::fail(PT_E_INVALID, "pt_accum_add: %u + %d samples exceed what a unit word carries (%u)", acc->n0, p->spp,
                            kAccumMaxSamples);
        a.accum = 1u; a.acc_n0 = acc->n0; a.acc_rng = acc->rng; a.acc_mean = acc->mean;
    }
    const bool has_work = p->spp > 0 && a.ntiles_shard > 0;

    // (the wavefront path's init_pixel_states resets the counters itself: one launch less per frame)
    if (!(has_work && wavefront))
        if (int rc = reset_counters(B, stream)) return rc;
    if (count && (p->flags & PT_FLAG_TRI_COUNTS)) {   // per-triangle test counts of this render (pt_tri_counts)
        HIP_TRY(hipMemsetAsync(c->tri_counts, 0, (size_t)std::max<uint32_t>(c->num_tris, 1u) * 4, stream));
        a.tri_counts = c->tri_counts;
    }
    HIP_TRY(hipEventRecord(F.ev0, stream));
    WavefrontDone wf;
    if (has_work && wavefront) {
        if (int rc = enqueue_wavefront(c, p, acc, a, F, B, stream, &wf, d_rays, points)) return rc;
    } else if (has_work) {
        if (int rc = launch_tiles(c, p, B, lds, stream, a, d_rays, rays_refwalk, points)) return rc;
    }
    HIP_TRY(hipEventRecord(F.ev1, stream));
    HIP_TRY(hipMemcpyAsync(F.hcnt, B.counters, kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(F.done, stream));
    F.kernel_events = has_work && wavefront;   // ek0/ek1 recorded around the integration kernel
    F.count = count;
    F.units = wf.units;
    F.split = wf.split;
    F.spp = p->spp;
    F.bounces = p->bounces;
    if (wf.seeded) {
        B.seed_cached = p->seed;
        B.seed_valid = true;
    }
    ++c->fl_n;
    return PT_OK;
}

int pt_render_device_view_async(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, float* d_out,
                                void* stream_v)
{
    if (!d_out) return pt::fail(PT_E_INVALID, "pt_render: null argument");
    return render_enqueue(c, p, cam, view, d_out, stream_v, nullptr);
}

int pt_render_device_async(pt_ctx* c, const pt_params* p, const pt_camera* cam, float* d_out, void* stream_v)
{
    return pt_render_device_view_async(c, p, cam, nullptr, d_out, stream_v);
}

int pt_render_wait(pt_ctx* c, pt_stats* st)
{
    if (!c) return pt::fail(PT_E_INVALID, "pt_render_wait: null context");
    if (c->fl_n == 0) return pt::fail(PT_E_INVALID, "pt_render_wait: no render in flight");
    HIP_TRY(hipSetDevice(c->device));
    pt_ctx::Flight& F = c->fl[c->fl_head];
    c->fl_head = (c->fl_head + 1) % pt_ctx::kFlights;
    --c->fl_n;
    // (the counters' copy is the render's last operation on its stream)
    HIP_TRY(hipEventSynchronize(F.done));
    const unsigned long long* cnt = F.hcnt;
    if (F.count) {
        if (const char* path = getenv("PT_SECTION_DUMP")) {   // counting runs: shading section profile
            if (FILE* f = fopen(path, "a")) {
                fprintf(f, "sections");
                for (int k = 0; k < kSections; ++k) fprintf(f, " %llu", cnt[CNT_SECTIONS + k]);
                fprintf(f, "\nwalk_hist");
                for (int k = 0; k < kHist; ++k) fprintf(f, " %llu", cnt[CNT_SECTIONS + kSections + k]);
                fprintf(f, "\ntrace_slots %llu walk_slots %llu nodes %llu leaf_steps %llu start_wait %llu top_visits %llu\n", cnt[CNT_TRACE_SLOTS], cnt[CNT_WALK_SLOTS],
                        cnt[CNT_NODES], cnt[CNT_LEAF_STEPS], cnt[CNT_START_WAIT], cnt[CNT_TOP_VISITS]);
                fprintf(f, "wall_clock start %llu drained %llu last_exit %llu mean_exit %.1f waves %llu (ticks)\n", cnt[CNT_T_START], cnt[CNT_T_DRAINED],
                        cnt[CNT_T_LAST_EXIT], cnt[CNT_WAVES] ? (double)cnt[CNT_T_EXIT_SUM] / (double)cnt[CNT_WAVES] : 0.0, cnt[CNT_WAVES]);
                fprintf(f, "lane_end_mean %.1f (ticks since start)\ntail_lane_end_log2_10us",
                        cnt[CNT_WAVES] ? (double)cnt[CNT_LANE_END_SUM] / (64.0 * (double)cnt[CNT_WAVES]) : 0.0);
                for (int k = 0; k < kTailBins; ++k) fprintf(f, " %llu", cnt[CNT_LANE_BINS + k]);
                fprintf(f, "\ntail_wave_exit_log2_10us");
                for (int k = 0; k < kTailBins; ++k) fprintf(f, " %llu", cnt[CNT_WAVE_BINS + k]);
                fprintf(f, "\niters_by_deep_lanes 0:%llu 1-4:%llu 5-8:%llu more:%llu no_leaf %llu neither %llu\n", cnt[CNT_ITERS],
                        cnt[CNT_ITERS + 1], cnt[CNT_ITERS + 2], cnt[CNT_ITERS + 3], cnt[CNT_ITERS + 4], cnt[CNT_ITERS + 5]);
                fclose(f);
            }
        }
    }
    float ms = 0.0f, kms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, F.ev0, F.ev1));
    if (F.kernel_events) HIP_TRY(hipEventElapsedTime(&kms, F.ek0, F.ek1));
    else kms = ms;   // (the tile kernel is the render's only launch)
    if (st) {
        st->seconds = ms * 1e-3;
        st->kernel_ms = kms;
        st->work_units = F.units;
        st->split_pixels = F.split;
        st->rays_traced = cnt[CNT_TRACED];
        st->rays_reference = cnt[CNT_REFERENCE];
        st->node_tests = cnt[CNT_NODES];
        st->tri_tests = cnt[CNT_TRIS];
        st->samples = cnt[CNT_SAMPLES];
        st->walk_lane_slots = cnt[CNT_WALK_SLOTS];
        st->leaf_steps = cnt[CNT_LEAF_STEPS];
        st->shade_lane_slots = cnt[CNT_SHADE_SLOTS];
        st->accel_fallbacks = cnt[CNT_FALLBACKS];
        st->walk_cycles = cnt[CNT_WALK_CYCLES];
        st->shade_cycles = cnt[CNT_SHADE_CYCLES];
        st->spill_entries = cnt[CNT_SPILL];
        st->lds_node_tests = cnt[CNT_TOP_VISITS];
        const uint64_t shard_px = cnt[CNT_SAMPLES] / (uint64_t)(F.spp > 0 ? F.spp : 1);
        st->rays_nominal = shard_px * (uint64_t)F.spp * (uint64_t)(F.bounces + 1);
    }
    return PT_OK;
}

int pt_render_device_view(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, float* d_out, void* stream,
                          pt_stats* st)
{
    if (c && c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_render_device: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    if (int rc = pt_render_device_view_async(c, p, cam, view, d_out, stream)) return rc;
    return pt_render_wait(c, st);
}

int pt_render_device(pt_ctx* c, const pt_params* p, const pt_camera* cam, float* d_out, void* stream, pt_stats* st)
{
    return pt_render_device_view(c, p, cam, nullptr, d_out, stream, st);
}

}  // extern "C"

// ---- accumulating passes (host_internal.h): the render context's side of pt_accum.cpp
int pt::accum_check(const pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view)
{
    if (int rc = validate_render(p, cam)) return rc;
    if (view)
        if (int rc = validate_view("pt_accum_create", view)) return rc;
    const RenderKnobs& K = c->knobs;
    if (p->flags & ~(uint32_t)(PT_FLAG_NO_DEAD_PATH_SKIP | PT_FLAG_NO_PRIMARY_CACHE | PT_FLAG_JITTER | PT_FLAG_JITTER_TENT))
        return pt::fail(PT_E_INVALID, "pt_accum_create: flags 0x%x: only PT_FLAG_NO_DEAD_PATH_SKIP, PT_FLAG_NO_PRIMARY_CACHE and "
                        "the jitter flags accumulate (the reference walks and the counting variants have no accumulating kernel)", p->flags);
    if (!takes_wavefront(p, cam, c->scene_extent, K.head_wf))
        return pt::fail(PT_E_INVALID, "pt_accum_create: this render would take the tile kernel (%s), which does not accumulate",
                        (p->integrator == PT_INTEGRATOR_HEAD && !K.head_wf) ? "integrator 1 with PT_HEAD_WF=0"
                                                                              : "camera beyond 64 scene extents");
    if (K.wf_min_waves != 5 || K.head_min_waves != 5)
        return pt::fail(PT_E_INVALID, "pt_accum_create: only the default-occupancy kernels accumulate (PT_WF_MIN_WAVES / "
                        "PT_HEAD_MIN_WAVES are set)");
    return PT_OK;
}

int pt::accum_pass(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, const AccumPass& acc, float* d_out,
                   void* stream, pt_stats* stats)
{
    if (c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_accum_add: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    if (int rc = render_enqueue(c, p, cam, view, d_out, stream, &acc, acc.rays, false, acc.points)) return rc;   // (rays: all regular)
    return pt_render_wait(c, stats);
}

void pt::ctx_scene_id(const pt_ctx* c, uint64_t* digest, uint32_t* num_tris, uint32_t* num_spheres)
{
    *digest = c->scene_digest;
    *num_tris = c->num_tris;
    *num_spheres = c->scene_spheres;
}
int pt::ctx_in_flight(const pt_ctx* c) { return c->fl_n; }
pt::DenoiseScratch* pt::ctx_denoise_scratch(pt_ctx* c) { return &c->denoise; }
pt::SessionScratch* pt::ctx_session_scratch(pt_ctx* c) { return &c->session; }
int pt::ctx_num_cus(const pt_ctx* c) { return c->num_cus; }
uint32_t pt::accum_max_samples() { return kAccumMaxSamples; }

int pt::copy_to_host(void* dst, const void* src, size_t bytes, void* stream_v, void** pinned, size_t* pinned_bytes)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    if (*pinned_bytes < bytes) {
        free_pinned(*pinned);
        *pinned = nullptr;
        *pinned_bytes = 0;
        if (hipHostMalloc(pinned, bytes, hipHostMallocDefault) != hipSuccess) {
            *pinned = nullptr;   // (no pinned memory: the runtime's own pageable path)
            HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            return PT_OK;
        }
        *pinned_bytes = bytes;
    }
    HIP_TRY(hipMemcpyAsync(*pinned, src, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const unsigned nt = (unsigned)std::min<size_t>(pt::host_threads(), std::max<size_t>(1, bytes >> 21));   // >= 2 MB each
    const char* s = static_cast<const char*>(*pinned);
    char* d = static_cast<char*>(dst);
    auto part = [&](unsigned k) {
        const size_t b0 = (bytes * k / nt) & ~(size_t)4095, b1 = (k + 1 == nt) ? bytes : ((bytes * (k + 1) / nt) & ~(size_t)4095);
        memcpy(d + b0, s + b0, b1 - b0);
    };
    if (nt <= 1) {
        memcpy(d, s, bytes);
    } else {
        std::vector<std::thread> th;
        th.reserve(nt - 1);
        for (unsigned k = 1; k < nt; ++k) th.emplace_back(part, k);
        part(0);
        for (std::thread& t : th) t.join();
    }
    return PT_OK;
}

void pt::free_pinned(void* p)
{
    if (p) (void)hipHostFree(p);
}

extern "C" {

int pt_render(pt_ctx* c, const pt_params* p, const pt_camera* cam, float* out_rgb, pt_stats* st)
{
    return pt_render_view(c, p, cam, nullptr, out_rgb, st);
}

int pt_render_view(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, float* out_rgb, pt_stats* st)
{
    if (!c || !p || !out_rgb) return pt::fail(PT_E_INVALID, "pt_render: null argument");
    if (p->width <= 0 || p->height <= 0) return pt::fail(PT_E_INVALID, "pt_render: bad image size");
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)p->width * (size_t)p->height * 3 * sizeof(float);
    if (int rc = pt::grow(&c->scratch_out, &c->scratch_floats, bytes / sizeof(float))) return rc;
    HIP_TRY(hipMemsetAsync(c->scratch_out, 0, bytes, nullptr));
    int rc = pt_render_device_view(c, p, cam, view, c->scratch_out, nullptr, st);
    if (rc != PT_OK) return rc;
    return pt::copy_to_host(out_rgb, c->scratch_out, bytes, nullptr, &c->pinned, &c->pinned_bytes);
}

}  // extern "C"

extern "C" int pt_trace(pt_ctx* c, uint32_t n, const float* rays, int32_t* tri_out, float* t_out, uint32_t flags)
{
    return pt_trace_counts(c, n, rays, tri_out, t_out, flags, nullptr, nullptr);
}

extern "C" int pt_tri_counts(pt_ctx* c, uint32_t* counts, uint32_t n)
{
    pt::clear_error();
    if (!c || !counts) return pt::fail(PT_E_INVALID, "pt_tri_counts: null argument");
    if (c->fl_n > 0) return pt::fail(PT_E_INVALID, "pt_tri_counts: renders in flight (pt_render_wait first)");
    if (n != c->num_tris) return pt::fail(PT_E_INVALID, "pt_tri_counts: n = %u, the scene has %u triangles", n, c->num_tris);
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(counts, c->tri_counts, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_trace_counts(pt_ctx* c, uint32_t n, const float* rays, int32_t* tri_out, float* t_out, uint32_t flags,
                               uint32_t* tri_counts, uint64_t* spill_entries)
{
    pt::clear_error();
    if (!c) return pt::fail(PT_E_INVALID, "pt_trace: null context");
    if (c->fl_n > 0) return pt::fail(PT_E_INVALID, "pt_trace: renders in flight (pt_render_wait first)");
    if (n == 0) return PT_OK;
    if (!rays || !tri_out || !t_out) return pt::fail(PT_E_INVALID, "pt_trace: null buffer");
    HIP_TRY(hipSetDevice(c->device));
    Args a;
    memset(&a, 0, sizeof(a));
    fill_scene_args(a, c);
    a.counters = c->rb[0].counters;
    a.node_mask = c->node4_mask;
    a.stack_words = (uint32_t)(c->depth + 2) * 64;
    if (a.stack_words < (uint32_t)kWaveLdsWords) a.stack_words = kWaveLdsWords;
    const size_t lds = (size_t)a.stack_words * 4 * 4;
    // (not reachable while pt_create caps bvh_depth at 63: this limit starts at depth 159)
    static_assert((size_t)(PT_MAX_BVH_DEPTH - 1 + 2) * 64 * 16 <= 160 * 1024, "every depth pt_create accepts fits the LDS stack");
    if (lds > 160 * 1024) return pt::fail(PT_E_BVH_DEPTH, "pt_trace: BVH depth %d too deep for the LDS stack", c->depth);
    uint32_t blocks = (n + 255) / 256;
    const uint32_t cap = (uint32_t)c->num_cus * 8u;
    if (blocks > cap) blocks = cap;
    if (int rc = pt::grow(&c->rb[0].spill, &c->rb[0].spill_words, stack_words_per_lane(c) * (size_t)blocks * 256)) return rc;
    a.spill = c->rb[0].spill;
    a.spill_stride = blocks * 256;
    pt::ScopedDevice<float> d_rays, d_t;
    pt::ScopedDevice<int32_t> d_tri;
    pt::ScopedDevice<uint32_t> d_cnt;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_rays), (size_t)n * 24));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_tri), (size_t)n * 4));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_t), (size_t)n * 4));
    HIP_TRY(hipMemcpy(d_rays, rays, (size_t)n * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->rb[0].counters, 0, kCounterWords * sizeof(unsigned long long)));
    const bool count = tri_counts != nullptr || spill_entries != nullptr;
    if (tri_counts && c->num_tris > 0) {   // (own scratch: the last render's counts stay for pt_tri_counts)
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_cnt), (size_t)c->num_tris * 4));
        HIP_TRY(hipMemset(d_cnt, 0, (size_t)c->num_tris * 4));
        a.tri_counts = d_cnt;
    }
    const bool ref = (flags & PT_FLAG_REFERENCE_BVH) != 0;
    if (ref && count) hipLaunchKernelGGL((trace_rays<true, true>), dim3(blocks), dim3(256), lds, 0, a, d_rays, n, d_tri, d_t);
    else if (ref) hipLaunchKernelGGL((trace_rays<true, false>), dim3(blocks), dim3(256), lds, 0, a, d_rays, n, d_tri, d_t);
    else if (count) hipLaunchKernelGGL((trace_rays<false, true>), dim3(blocks), dim3(256), lds, 0, a, d_rays, n, d_tri, d_t);
    else hipLaunchKernelGGL((trace_rays<false, false>), dim3(blocks), dim3(256), lds, 0, a, d_rays, n, d_tri, d_t);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(tri_out, d_tri, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t_out, d_t, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (tri_counts && c->num_tris > 0) {   // added to the caller's counts (kernel.cu:133 accumulates)
        std::vector<uint32_t> h(c->num_tris);
        HIP_TRY(hipMemcpy(h.data(), d_cnt, (size_t)c->num_tris * 4, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < c->num_tris; ++k) tri_counts[k] += h[k];
    }
    if (spill_entries) {
        unsigned long long v = 0;
        HIP_TRY(hipMemcpy(&v, c->rb[0].counters + CNT_SPILL, sizeof(v), hipMemcpyDeviceToHost));
        *spill_entries = v;
    }
    return PT_OK;
}

// ---- ray queries on device buffers (pt_trace_device, pt_occluded_device, pt_occluded; query_rays)

// An integer knob of the queries, read on every call: the variable's value clamped to lo..hi, or dflt when unset.
static uint32_t query_knob(const char* name, uint32_t lo, uint32_t hi, uint32_t dflt)
{
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    return (uint32_t)std::min<long long>(std::max<long long>(atoll(e), (long long)lo), (long long)hi);
}

// Rays per launch: no ray index wraps and 6 * index stays below 2^32 (trace_rays indexes in 32 bits).
constexpr uint32_t kQueryLaunchRays = 1u << 29;
constexpr uint32_t kQueryRefillAt = 32;   // idle lanes of a wave at which it refills

// What the three calls check, in this order: the context; n == 0 (PT_OK, nothing else looked at); the flags; the
// buffers; renders in flight; the LDS stack (as pt_trace).
static int query_check(const pt_ctx* c, const char* who, uint32_t n, uint32_t flags, uint32_t allowed, bool buffers, bool* done)
{
    *done = true;
    if (!c) return pt::fail(PT_E_INVALID, "%s: null context", who);
    if (n == 0) return PT_OK;
    if (flags & ~allowed) return pt::fail(PT_E_INVALID, "%s: unknown flags 0x%x (allowed: 0x%x)", who, flags & ~allowed, allowed);
    if (!buffers) return pt::fail(PT_E_INVALID, "%s: null buffer", who);
    if (c->fl_n > 0) return pt::fail(PT_E_INVALID, "%s: %d asynchronous renders in flight (pt_render_wait first)", who, c->fl_n);
    // (not reachable while pt_create caps bvh_depth at 63, as in pt_trace: kept for a larger PT_MAX_BVH_DEPTH)
    if ((size_t)std::max<uint32_t>((uint32_t)(c->depth + 2) * 64, (uint32_t)kWaveLdsWords) * 16 > 160 * 1024)
        return pt::fail(PT_E_BVH_DEPTH, "%s: BVH depth %d too deep for the LDS stack", who, c->depth);
    *done = false;
    return PT_OK;
}

// Enqueue the query of n rays on `stream` and wait for it.  occluded: d_occ (and d_tmax or null); else d_tri, d_t.
static int query_run(pt_ctx* c, bool occluded, bool ref, uint32_t n, const float* d_rays, const float* d_tmax, int32_t* d_tri,
                     float* d_t, uint8_t* d_occ, hipStream_t stream)
{
    HIP_TRY(hipSetDevice(c->device));
    if (!alloc_bufs(c->rb[0])) return pt::fail(PT_E_HIP, "ray query: device allocation failed");
    Args a;
    memset(&a, 0, sizeof(a));
    fill_scene_args(a, c);
    a.counters = c->rb[0].counters;
    a.node_mask = c->node4_mask;
    // PT_QUERY_REFILL: the idle lanes at which a wave refills (64: lock-step; tools/query_cost.py)
    const uint32_t refill_at = query_knob("PT_QUERY_REFILL", 1, 64, kQueryRefillAt);
    const void* kernel = occluded ? (const void*)query_rays<true> : (const void*)query_rays<false>;
    size_t lds = (size_t)kWaveLdsWords * 4 * 4;
    uint32_t cap = (uint32_t)c->num_cus * 8u;   // trace_rays' grid (pt_trace)
    // PT_QUERY_LOCKSTEP=1: pt_trace_device runs pt_trace's own kernel, trace_rays<false, false>, on the caller's buffers
    // (the same bits; the baseline tools/query_cost.py measures query_rays against)
    const bool lockstep = !occluded && !ref && query_knob("PT_QUERY_LOCKSTEP", 0, 1, 0) != 0;
    if (ref || lockstep) {
        a.stack_words = std::max<uint32_t>((uint32_t)(c->depth + 2) * 64, (uint32_t)kWaveLdsWords);
        lds = (size_t)a.stack_words * 4 * 4;
    } else {
        // a persistent grid: the blocks the device holds at once, or PT_QUERY_BLOCKS of them
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds));
        cap = (uint32_t)c->num_cus * (uint32_t)std::max(per_cu, 1);
        cap = query_knob("PT_QUERY_BLOCKS", 1, cap, cap);
    }
    for (uint64_t first = 0; first < n; first += kQueryLaunchRays) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(n - first, kQueryLaunchRays);
        const uint32_t blocks = std::min((m + 255u) / 256u, cap);
        if (int rc = pt::grow(&c->rb[0].spill, &c->rb[0].spill_words, stack_words_per_lane(c) * (size_t)blocks * 256)) return rc;
        a.spill = c->rb[0].spill;
        a.spill_stride = blocks * 256;
        const float* rays = d_rays + first * 6;
        if (ref) {
            hipLaunchKernelGGL((trace_rays<true, false>), dim3(blocks), dim3(256), lds, stream, a, rays, m, d_tri + first, d_t + first);
        } else if (lockstep) {
            hipLaunchKernelGGL((trace_rays<false, false>), dim3(blocks), dim3(256), lds, stream, a, rays, m, d_tri + first, d_t + first);
        } else {
            const float* tmax = d_tmax ? d_tmax + first : nullptr;
            if (!occluded)
                hipLaunchKernelGGL((query_rays<false>), dim3(blocks), dim3(256), lds, stream, a, rays, tmax, m, refill_at,
                                   d_tri + first, d_t + first, (uint8_t*)nullptr);
            else
                hipLaunchKernelGGL((query_rays<true>), dim3(blocks), dim3(256), lds, stream, a, rays, tmax, m, refill_at,
                                   (int32_t*)nullptr, (float*)nullptr, d_occ + first);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));   // (the next launch reuses the spill columns)
    }
    return PT_OK;
}

extern "C" int pt_trace_device(pt_ctx* c, uint32_t n, const float* d_rays, int32_t* d_tri, float* d_t, uint32_t flags, void* stream)
{
    pt::clear_error();
    bool done;
    if (int rc = query_check(c, "pt_trace_device", n, flags, PT_FLAG_REFERENCE_BVH, d_rays && d_tri && d_t, &done)) return rc;
    if (done) return PT_OK;
    return query_run(c, false, (flags & PT_FLAG_REFERENCE_BVH) != 0, n, d_rays, nullptr, d_tri, d_t, nullptr,
                     reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pt_occluded_device(pt_ctx* c, uint32_t n, const float* d_rays, const float* d_tmax, uint8_t* d_occ, uint32_t flags,
                                  void* stream)
{
    pt::clear_error();
    bool done;
    if (int rc = query_check(c, "pt_occluded_device", n, flags, 0u, d_rays && d_occ, &done)) return rc;
    if (done) return PT_OK;
    return query_run(c, true, false, n, d_rays, d_tmax, nullptr, nullptr, d_occ, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pt_occluded(pt_ctx* c, uint32_t n, const float* rays, const float* tmax, uint8_t* occ, uint32_t flags)
{
    pt::clear_error();
    bool done;
    if (int rc = query_check(c, "pt_occluded", n, flags, 0u, rays && occ, &done)) return rc;
    if (done) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    // the context's staging buffer: the rays (24 n bytes), the bounds (4 n), the answers (n)
    if (int rc = pt::grow(&c->query_stage, &c->query_stage_bytes, (size_t)n * 29)) return rc;
    float* const d_rays = reinterpret_cast<float*>(c->query_stage);
    float* const d_tmax = d_rays + (size_t)n * 6;
    uint8_t* const d_occ = c->query_stage + (size_t)n * 28;
    HIP_TRY(hipMemcpy(d_rays, rays, (size_t)n * 24, hipMemcpyHostToDevice));
    if (tmax) HIP_TRY(hipMemcpy(d_tmax, tmax, (size_t)n * 4, hipMemcpyHostToDevice));
    if (int rc = query_run(c, true, false, n, d_rays, tmax ? d_tmax : nullptr, nullptr, nullptr, d_occ, nullptr)) return rc;
    HIP_TRY(hipMemcpy(occ, d_occ, n, hipMemcpyDeviceToHost));
    return PT_OK;
}

// ---- renders along caller-supplied rays (pt_render_rays_device, pt_render_rays, pt_rays_classify_device)

// The classes of n rays at d_rays, through the context's four words: what both entry points below run first.
// (points: the records are the points {p, n} of an irradiance render)
static int classify_ctx_rays(pt_ctx* c, const char* who, uint32_t n, const float* d_rays, hipStream_t stream, pt_ray_classes* out,
                             bool points = false)
{
    if (reinterpret_cast<uintptr_t>(d_rays) % 8 != 0)
        return pt::fail(PT_E_INVALID, "%s: the %s buffer must be 8-byte aligned", who, points ? "point" : "ray");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = pt::grow(&c->ray_classes, &c->ray_classes_words, 4)) return rc;
    return pt::classify_ray_buffer(d_rays, n, 64.0f * c->scene_extent, c->num_cus, c->ray_classes, stream, out, points);
}

// The stand-in camera of a call that takes rays: it carries the image size for the checks and sits at the origin,
// within any scene's reach.
static pt_camera rays_stand_in(const pt_params* p)
{
    pt_camera cam;
    memset(&cam, 0, sizeof(cam));
    cam.dist_from_film = 1.0f; cam.focal_length = 1.0f;
    cam.pxl_width = p->width; cam.pxl_height = p->height;
    return cam;
}

// The classes of an image's rays (p validated: width, height <= 65535), and the refusal of a buffer with an invalid
// ray, its lowest pixel named.
static int classify_image_rays(pt_ctx* c, const char* who, const pt_params* p, const float* d_rays, hipStream_t stream,
                               pt_ray_classes* cls, bool points = false)
{
    const uint32_t n = (uint32_t)p->width * (uint32_t)p->height;
    if (int rc = classify_ctx_rays(c, who, n, d_rays, stream, cls, points)) return rc;
    if (cls->invalid != 0) {
        uint32_t x = cls->first_invalid % (uint32_t)p->width, y = cls->first_invalid / (uint32_t)p->width;
        if (p->pixel_order == PT_ORDER_MORTON) pt_morton_i_to_pxl(cls->first_invalid, &x, &y);
        if (points)
            return pt::fail(PT_E_INVALID, "%s: %llu invalid points (a non-finite component or a normal that is not of unit length), "
                            "the first at index %u, pixel (%u, %u)", who, (unsigned long long)cls->invalid, cls->first_invalid, x, y);
        return pt::fail(PT_E_INVALID, "%s: %llu invalid rays (a non-finite component or a zero direction), the first at "
                        "index %u, pixel (%u, %u)", who, (unsigned long long)cls->invalid, cls->first_invalid, x, y);
    }
    return PT_OK;
}

extern "C" int pt_rays_classify_device(pt_ctx* c, uint32_t n, const float* d_rays, void* stream, pt_ray_classes* out)
{
    pt::clear_error();
    if (!c || !out) return pt::fail(PT_E_INVALID, "pt_rays_classify_device: null argument");
    if (n > 0 && !d_rays) return pt::fail(PT_E_INVALID, "pt_rays_classify_device: null buffer");
    if (c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_rays_classify_device: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    return classify_ctx_rays(c, "pt_rays_classify_device", n, d_rays, reinterpret_cast<hipStream_t>(stream), out);
}

extern "C" int pt_render_rays_device(pt_ctx* c, const pt_params* p, const float* d_rays, float* d_out, void* stream, pt_stats* st)
{
    pt::clear_error();
    if (!c || !p || !d_rays || !d_out) return pt::fail(PT_E_INVALID, "pt_render_rays: null argument");
    if (c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_render_rays: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    constexpr uint32_t allowed = PT_FLAG_NO_DEAD_PATH_SKIP | PT_FLAG_NO_PRIMARY_CACHE | PT_FLAG_REFERENCE_TRAVERSAL | PT_FLAG_REFERENCE_BVH;
    if (p->flags & ~allowed)
        return pt::fail(PT_E_INVALID, "pt_render_rays: flags 0x%x: a render along rays takes only PT_FLAG_NO_DEAD_PATH_SKIP, "
                        "PT_FLAG_NO_PRIMARY_CACHE, PT_FLAG_REFERENCE_TRAVERSAL and PT_FLAG_REFERENCE_BVH (no counting variants, and "
                        "no film to jitter on)", p->flags & ~allowed);
    const pt_camera cam = rays_stand_in(p);
    if (int rc = pt::validate_render(p, &cam)) return rc;
    pt_ray_classes cls;
    if (int rc = classify_image_rays(c, "pt_render_rays", p, d_rays, reinterpret_cast<hipStream_t>(stream), &cls)) return rc;
    if (int rc = render_enqueue(c, p, &cam, nullptr, d_out, stream, nullptr, d_rays, cls.irregular != 0)) return rc;
    return pt_render_wait(c, st);
}

// ---- accumulators over a ray buffer or a point buffer (pt_accum_create_rays*, pt_accum_create_points*, pt_accum.cpp):
// the context's side
int pt::accum_check_rays(const pt_ctx* c, const pt_params* p, pt_camera* stand_in, bool points)
{
    const char* who = points ? "pt_accum_create_points" : "pt_accum_create_rays";
    constexpr uint32_t allowed = PT_FLAG_NO_DEAD_PATH_SKIP | PT_FLAG_NO_PRIMARY_CACHE;
    if (p->flags & ~allowed)
        return pt::fail(PT_E_INVALID, "%s: flags 0x%x: an accumulator over %s takes only PT_FLAG_NO_DEAD_PATH_SKIP "
                        "and PT_FLAG_NO_PRIMARY_CACHE (the reference walks and the counting variants have no accumulating kernel, "
                        "and there is no film to jitter on)", who, p->flags & ~allowed, points ? "points" : "rays");
    *stand_in = rays_stand_in(p);
    if (int rc = validate_render(p, stand_in)) return rc;
    const RenderKnobs& K = c->knobs;
    if (!takes_wavefront(p, stand_in, c->scene_extent, K.head_wf))
        return pt::fail(PT_E_INVALID, "%s: this render would take the tile kernel (integrator 1 with PT_HEAD_WF=0), "
                        "which does not accumulate", who);
    if (K.wf_min_waves != 5 || K.head_min_waves != 5)
        return pt::fail(PT_E_INVALID, "%s: only the default-occupancy kernels accumulate (PT_WF_MIN_WAVES / "
                        "PT_HEAD_MIN_WAVES are set)", who);
    return PT_OK;
}

int pt::accum_classify_rays(pt_ctx* c, const pt_params* p, const float* d_rays, void* stream, bool points)
{
    pt_ray_classes cls;
    if (int rc = classify_image_rays(c, points ? "pt_accum_create_points" : "pt_accum_create_rays", p, d_rays,
                                     reinterpret_cast<hipStream_t>(stream), &cls, points))
        return rc;
    if (cls.irregular != 0 && points)   // (never a silent fall-back: the accumulating kernels are the wavefront kernels)
        return pt::fail(PT_E_INVALID, "pt_accum_create_points: %llu irregular points (a position beyond 64 scene extents); "
                        "accumulation runs on the wavefront kernels only -- pt_render_irradiance takes such a buffer",
                        (unsigned long long)cls.irregular);
    if (cls.irregular != 0)
        return pt::fail(PT_E_INVALID, "pt_accum_create_rays: %llu irregular rays (an origin beyond 64 scene extents, or a direction "
                        "longer than a normalised one); accumulation runs on the wavefront kernels only -- pt_render_rays takes "
                        "such a buffer", (unsigned long long)cls.irregular);
    return PT_OK;
}

extern "C" int pt_render_rays(pt_ctx* c, const pt_params* p, const float* rays, float* out_rgb, pt_stats* st)
{
    pt::clear_error();
    if (!c || !p || !rays || !out_rgb) return pt::fail(PT_E_INVALID, "pt_render_rays: null argument");
    if (p->width <= 0 || p->height <= 0 || p->width > 65535 || p->height > 65535)
        return pt::fail(PT_E_INVALID, "pt_render_rays: image size %dx%d out of range (1..65535)", p->width, p->height);
    if (c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_render_rays: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    HIP_TRY(hipSetDevice(c->device));
    const size_t npx = (size_t)p->width * (size_t)p->height, bytes = npx * 3 * sizeof(float);
    if (int rc = pt::grow(&c->rays_stage, &c->rays_stage_floats, npx * 6)) return rc;
    if (int rc = pt::grow(&c->scratch_out, &c->scratch_floats, npx * 3)) return rc;
    HIP_TRY(hipMemcpy(c->rays_stage, rays, npx * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(c->scratch_out, 0, bytes, nullptr));
    if (int rc = pt_render_rays_device(c, p, c->rays_stage, c->scratch_out, nullptr, st)) return rc;
    return pt::copy_to_host(out_rgb, c->scratch_out, bytes, nullptr, &c->pinned, &c->pinned_bytes);
}

// ---- irradiance renders at caller-supplied points (pt_render_irradiance_device, pt_render_irradiance,
// pt_points_classify_device): pt_render_rays*'s entry points over a point buffer, word for word

extern "C" int pt_points_classify_device(pt_ctx* c, uint32_t n, const float* d_points, void* stream, pt_ray_classes* out)
{
    pt::clear_error();
    if (!c || !out) return pt::fail(PT_E_INVALID, "pt_points_classify_device: null argument");
    if (n > 0 && !d_points) return pt::fail(PT_E_INVALID, "pt_points_classify_device: null buffer");
    if (c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_points_classify_device: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    return classify_ctx_rays(c, "pt_points_classify_device", n, d_points, reinterpret_cast<hipStream_t>(stream), out, true);
}

extern "C" int pt_render_irradiance_device(pt_ctx* c, const pt_params* p, const float* d_points, float* d_out, void* stream,
                                           pt_stats* st)
{
    pt::clear_error();
    if (!c || !p || !d_points || !d_out) return pt::fail(PT_E_INVALID, "pt_render_irradiance: null argument");
    if (c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_render_irradiance: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    constexpr uint32_t allowed = PT_FLAG_NO_DEAD_PATH_SKIP | PT_FLAG_NO_PRIMARY_CACHE | PT_FLAG_REFERENCE_TRAVERSAL | PT_FLAG_REFERENCE_BVH;
    if (p->flags & ~allowed)
        return pt::fail(PT_E_INVALID, "pt_render_irradiance: flags 0x%x: an irradiance render takes only PT_FLAG_NO_DEAD_PATH_SKIP, "
                        "PT_FLAG_NO_PRIMARY_CACHE, PT_FLAG_REFERENCE_TRAVERSAL and PT_FLAG_REFERENCE_BVH (no counting variants, and "
                        "no film to jitter on)", p->flags & ~allowed);
    const pt_camera cam = rays_stand_in(p);
    if (int rc = pt::validate_render(p, &cam)) return rc;
    pt_ray_classes cls;
    if (int rc = classify_image_rays(c, "pt_render_irradiance", p, d_points, reinterpret_cast<hipStream_t>(stream), &cls, true)) return rc;
    if (int rc = render_enqueue(c, p, &cam, nullptr, d_out, stream, nullptr, d_points, cls.irregular != 0, true)) return rc;
    return pt_render_wait(c, st);
}

extern "C" int pt_render_irradiance(pt_ctx* c, const pt_params* p, const float* points, float* out_rgb, pt_stats* st)
{
    pt::clear_error();
    if (!c || !p || !points || !out_rgb) return pt::fail(PT_E_INVALID, "pt_render_irradiance: null argument");
    if (p->width <= 0 || p->height <= 0 || p->width > 65535 || p->height > 65535)
        return pt::fail(PT_E_INVALID, "pt_render_irradiance: image size %dx%d out of range (1..65535)", p->width, p->height);
    if (c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_render_irradiance: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    HIP_TRY(hipSetDevice(c->device));
    const size_t npx = (size_t)p->width * (size_t)p->height, bytes = npx * 3 * sizeof(float);
    if (int rc = pt::grow(&c->rays_stage, &c->rays_stage_floats, npx * 6)) return rc;   // (the ray renders' staging buffer)
    if (int rc = pt::grow(&c->scratch_out, &c->scratch_floats, npx * 3)) return rc;
    HIP_TRY(hipMemcpy(c->rays_stage, points, npx * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(c->scratch_out, 0, bytes, nullptr));
    if (int rc = pt_render_irradiance_device(c, p, c->rays_stage, c->scratch_out, nullptr, st)) return rc;
    return pt::copy_to_host(out_rgb, c->scratch_out, bytes, nullptr, &c->pinned, &c->pinned_bytes);
}

// What pt_render_features* checks before touching the device; *vp = params with the ignored fields neutral.
static int features_check(const pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, const void* feat,
                          pt_params* vp)
{
    if (!c || !p || !cam || !feat) return pt::fail(PT_E_INVALID, "pt_render_features: null argument");
    if (c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_render_features: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    *vp = *p;
    // (of the flags only the jitter bits matter: PT_FLAG_JITTER moves the ray to the footprint's centre)
    vp->spp = 0; vp->bounces = 1; vp->integrator = PT_INTEGRATOR_UNIDIR; vp->seed = 0;
    vp->flags = p->flags & (PT_FLAG_JITTER | PT_FLAG_JITTER_TENT);
    if (int rc = pt::validate_render(vp, cam)) return rc;
    if (view)
        if (int rc = pt::validate_view("pt_render_features", view)) return rc;
    if ((uint64_t)c->num_tris + (uint64_t)c->num_spheres >= (uint64_t)PT_FEATURE_EMISSIVE)
        return pt::fail(PT_E_INVALID, "pt_render_features: %u triangles + %u spheres do not fit the 30 id bits of pt_feature.prim",
                        c->num_tris, c->num_spheres);
    return PT_OK;
}

extern "C" int pt_render_features_device(pt_ctx* c, const pt_params* p_in, const pt_camera* cam, pt_feature* d_feat, void* stream_v)
{
    return pt_render_features_view_device(c, p_in, cam, nullptr, d_feat, stream_v);
}

extern "C" int pt_render_features_view_device(pt_ctx* c, const pt_params* p_in, const pt_camera* cam, const pt_view* view,
                                              pt_feature* d_feat, void* stream_v)
{
    pt::clear_error();
    static_assert(sizeof(pt_feature) == 48, "pt_feature is 48 B");
    pt_params pv;
    if (int rc = features_check(c, p_in, cam, view, d_feat, &pv)) return rc;
    if (reinterpret_cast<uintptr_t>(d_feat) % 16 != 0)
        return pt::fail(PT_E_INVALID, "pt_render_features_device: d_feat must be 16-byte aligned");
    const pt_params* p = &pv;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    Args a;
    memset(&a, 0, sizeof(a));
    fill_scene_args(a, c);
    fill_view_args(a, *p, *cam, view);
    a.node_mask = c->node4_mask;
    a.stack_words = kWaveLdsWords;
    const size_t lds = (size_t)a.stack_words * 4 * 4;
    if (a.npix == 0) return PT_OK;
    uint32_t blocks = (uint32_t)(((uint64_t)a.npix + 255) / 256);
    const uint32_t cap = (uint32_t)c->num_cus * 8u;
    if (blocks > cap) blocks = cap;
    if (int rc = pt::grow(&c->rb[0].spill, &c->rb[0].spill_words, stack_words_per_lane(c) * (size_t)blocks * 256)) return rc;
    a.spill = c->rb[0].spill;
    a.spill_stride = blocks * 256;
    a.flags = p->flags;
    hipLaunchKernelGGL((p->flags & PT_FLAG_JITTER) ? primary_features_jitter : a.oriented ? primary_features_view : primary_features,
                       dim3(blocks), dim3(256), lds, stream, a,
                       reinterpret_cast<float4*>(d_feat));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}

extern "C" int pt_render_features(pt_ctx* c, const pt_params* p, const pt_camera* cam, pt_feature* feat)
{
    return pt_render_features_view(c, p, cam, nullptr, feat);
}

extern "C" int pt_render_features_view(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, pt_feature* feat)
{
    pt::clear_error();
    pt_params pv;
    if (int rc = features_check(c, p, cam, view, feat, &pv)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)p->width * (size_t)p->height;
    pt_feature none;
    memset(&none, 0, sizeof(none));
    none.prim = -1;
    for (size_t i = 0; i < n; ++i) feat[i] = none;   // pixels outside the shard stay like this
    pt::ScopedDevice<pt_feature> d_feat;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_feat), n * sizeof(pt_feature)));
    HIP_TRY(hipMemcpy(d_feat, feat, n * sizeof(pt_feature), hipMemcpyHostToDevice));
    if (int rc = pt_render_features_view_device(c, p, cam, view, d_feat, nullptr)) return rc;
    HIP_TRY(hipMemcpy(feat, d_feat, n * sizeof(pt_feature), hipMemcpyDeviceToHost));
    return PT_OK;
}

// ---- feature buffers over a ray buffer (pt_render_features_rays_device, pt_render_features_rays)

// What both calls check before touching the device, in pt.h's order; *vp = params with the ignored fields neutral.
static int features_rays_check(const pt_ctx* c, const pt_params* p, const float* rays, const void* feat, pt_params* vp)
{
    if (!c || !p || !rays || !feat) return pt::fail(PT_E_INVALID, "pt_render_features_rays: null argument");
    if (c->fl_n > 0)
        return pt::fail(PT_E_INVALID, "pt_render_features_rays: %d asynchronous renders in flight (pt_render_wait first)", c->fl_n);
    *vp = *p;
    vp->spp = 0; vp->bounces = 1; vp->integrator = PT_INTEGRATOR_UNIDIR; vp->seed = 0;
    vp->flags = 0;   // (nothing jitters: there is no film)
    const pt_camera cam = rays_stand_in(p);
    if (int rc = pt::validate_render(vp, &cam)) return rc;
    if ((uint64_t)c->num_tris + (uint64_t)c->num_spheres >= (uint64_t)PT_FEATURE_EMISSIVE)
        return pt::fail(PT_E_INVALID, "pt_render_features_rays: %u triangles + %u spheres do not fit the 30 id bits of pt_feature.prim",
                        c->num_tris, c->num_spheres);
    return PT_OK;
}

extern "C" int pt_render_features_rays_device(pt_ctx* c, const pt_params* p_in, const float* d_rays, pt_feature* d_feat, void* stream_v)
{
    pt::clear_error();
    pt_params pv;
    if (int rc = features_rays_check(c, p_in, d_rays, d_feat, &pv)) return rc;
    if (reinterpret_cast<uintptr_t>(d_feat) % 16 != 0)
        return pt::fail(PT_E_INVALID, "pt_render_features_rays_device: d_feat must be 16-byte aligned");
    const pt_params* p = &pv;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    pt_ray_classes cls;   // (an irregular ray is legal here: the kernel chooses the walk per ray)
    if (int rc = classify_image_rays(c, "pt_render_features_rays", p, d_rays, stream, &cls)) return rc;
    RayArgs a;
    memset(&a, 0, sizeof(a));
    fill_scene_args(a, c);
    fill_view_args(a, *p, rays_stand_in(p), nullptr);
    a.rays = d_rays;
    a.node_mask = c->node4_mask;
    a.stack_words = kWaveLdsWords;
    const size_t lds = (size_t)a.stack_words * 4 * 4;
    if (a.npix == 0) return PT_OK;
    uint32_t blocks = (uint32_t)(((uint64_t)a.npix + 255) / 256);
    const uint32_t cap = (uint32_t)c->num_cus * 8u;
    if (blocks > cap) blocks = cap;
    if (int rc = pt::grow(&c->rb[0].spill, &c->rb[0].spill_words, stack_words_per_lane(c) * (size_t)blocks * 256)) return rc;
    a.spill = c->rb[0].spill;
    a.spill_stride = blocks * 256;
    hipLaunchKernelGGL(primary_features_rays, dim3(blocks), dim3(256), lds, stream, a, reinterpret_cast<float4*>(d_feat));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}

extern "C" int pt_render_features_rays(pt_ctx* c, const pt_params* p, const float* rays, pt_feature* feat)
{
    pt::clear_error();
    pt_params pv;
    if (int rc = features_rays_check(c, p, rays, feat, &pv)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)p->width * (size_t)p->height;
    if (int rc = pt::grow(&c->rays_stage, &c->rays_stage_floats, n * 6)) return rc;
    HIP_TRY(hipMemcpy(c->rays_stage, rays, n * 24, hipMemcpyHostToDevice));
    std::vector<pt_feature> host(n);   // (the caller's buffer is written only once the call has succeeded)
    pt_feature none;
    memset(&none, 0, sizeof(none));
    none.prim = -1;
    for (size_t i = 0; i < n; ++i) host[i] = none;   // pixels outside the shard stay like this
    pt::ScopedDevice<pt_feature> d_feat;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_feat), n * sizeof(pt_feature)));
    HIP_TRY(hipMemcpy(d_feat, host.data(), n * sizeof(pt_feature), hipMemcpyHostToDevice));
    if (int rc = pt_render_features_rays_device(c, p, c->rays_stage, d_feat, nullptr)) return rc;
    HIP_TRY(hipMemcpy(feat, d_feat, n * sizeof(pt_feature), hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_shard_pixels(int w, int h, int shard_index, int shard_count, int tile_w, int tile_h, uint32_t* out,
                               uint32_t cap, uint32_t* n_out)
{
    pt::clear_error();
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535 || shard_count < 1 || shard_index < 0 || shard_index >= shard_count || !n_out)
        return pt::fail(PT_E_INVALID, "pt_shard_pixels: bad arguments");
    for (const int v : {tile_w, tile_h})
        if (v != 0 && (v < 8 || v > 256 || v % 8 != 0)) return pt::fail(PT_E_INVALID, "pt_shard_pixels: tile size %dx%d", tile_w, tile_h);
    pt_params p;
    memset(&p, 0, sizeof(p));
    p.width = w; p.height = h; p.shard_index = shard_index; p.shard_count = shard_count; p.tile_w = tile_w; p.tile_h = tile_h;
    const pt::TileGrid m = pt::tile_grid(p);
    if (!m.fits()) return pt::fail(PT_E_INVALID, "pt_shard_pixels: %dx%d pads to more than 2^32-1 pixel slots", w, h);
    const uint64_t slots = m.npix;
    uint32_t n = 0;
    for (uint64_t q = 0; q < slots; ++q) {
        uint32_t px, py;
        if (!unit_pixel(m, (uint32_t)q, &px, &py)) continue;
        if (out) {
            if (n >= cap) return pt::fail(PT_E_INVALID, "pt_shard_pixels: buffer of %u entries too small", cap);
            out[n] = py * (uint32_t)w + px;
        }
        ++n;
    }
    *n_out = n;
    return PT_OK;
}

int pt::shard_slots(const pt_params* p, std::vector<uint32_t>* pix)
{
    const pt::TileGrid m = pt::tile_grid(*p);
    const size_t slots = m.npix;   // (= Args::npix of this shard's renders)
    pix->assign(slots, 0xffffffffu);
    for (size_t q = 0; q < slots; ++q) {
        uint32_t px, py;
        if (unit_pixel(m, (uint32_t)q, &px, &py)) (*pix)[q] = py * (uint32_t)p->width + px;
    }
    return PT_OK;
}

extern "C" int pt_tonemap_device(pt_ctx* c, const float* d_rgb, int w, int h, int32_t* d_codes, void* stream_v)
{
    pt::clear_error();
    if (!c || !d_rgb || !d_codes || w <= 0 || h <= 0) return pt::fail(PT_E_INVALID, "pt_tonemap_device: bad arguments");
    if (!c->tone_ok) return pt::fail(PT_E_INVALID, "pt_tonemap_device: host tone map not monotone; use pt_tonemap_u8");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    const size_t n = (size_t)w * (size_t)h * 3;
    size_t blocks = (n + 255) / 256;
    if (blocks > (size_t)c->num_cus * 32) blocks = (size_t)c->num_cus * 32;
    hipLaunchKernelGGL(tonemap_codes, dim3((unsigned)blocks), dim3(256), 0, stream, d_rgb, n, c->tone_thr, d_codes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}

extern "C" int pt_tonemap(pt_ctx* c, const float* rgb, int w, int h, int32_t* codes)
{
    pt::clear_error();
    if (!c || !rgb || !codes || w <= 0 || h <= 0) return pt::fail(PT_E_INVALID, "pt_tonemap: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)w * (size_t)h * 3;
    pt::ScopedDevice<float> d_rgb;
    pt::ScopedDevice<int32_t> d_codes;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_rgb), n * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_codes), n * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(d_rgb, rgb, n * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = pt_tonemap_device(c, d_rgb, w, h, d_codes, nullptr)) return rc;
    HIP_TRY(hipMemcpy(codes, d_codes, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
        if (codes[i] == INT32_MAX) codes[i] = pt_tonemap_u8((double)rgb[i]);
    return PT_OK;
}
