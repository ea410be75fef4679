// pt_render.hip -- the gfx950 render kernels: device code only.  The host half of this translation unit (the
// render context, pt_create / pt_destroy and the render, trace, features and tone-map entry points of pt/pt.h) is
// pt_render_host.h, included once as the last line.  Text after the kernels cannot change how they compile, and an
// edit confined to that header leaves this file, and any hash taken over the kernel sources, as it is.
//
// Sections, in order:
//   Args, counter slots        the one argument block every kernel takes
//   tile-path integrators      spheres, the per-lane tracer, integrators 0 and 1, the camera, render_tiles.  One wave
//                              renders one 8x8 image tile: lane l owns pixel (8*tx + mx(l), 8*ty + my(l)) with
//                              (mx, my) the Morton decode of l, and runs ALL of that pixel's samples in order with
//                              its XORWOW state and f64 running mean in registers (the reference keeps both in HBM
//                              and re-launches drawPixel per sample, kernel.cu:535-553, 709-736).  Waves are
//                              persistent and pull tiles from an atomic counter; tile t belongs to shard
//                              t % shard_count.
//   unit set-up                init_pixel_states, init_active_states, seed_table, build_jump_byte_tables,
//                              finalize_pixels: the wavefront kernels' work units and RNG tables
//   wavefront shading          what the two shading passes share (unit dealing, winner check, hit bookkeeping,
//                              stream store-back, whole-pixel end), then the passes of integrator 0 and integrator 1
//   wf_main, kernel instances  render_unidir_wf, render_head_wf and their accumulating twins
//   output / trace / features  tonemap_codes, trace_rays, primary_features
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>

#include "../host/host_internal.h"
#include "../host/render_plan.h"
#include "pt_device.h"
#include "pt_scene_pack.h"

using namespace ptd;

namespace {

constexpr uint32_t kTile = pt::kTile;   // 8x8 = 64 pixels = one wave

// A box is skipped when its entry lies beyond best_t * kCullRel (DESIGN.md "Traversal" 4)
constexpr float kCullRel = 1.0f + 1.0f / 1024.0f;
struct Args {
    const DNode* nodes;
    const RNode* rnodes;
    const DTri* tris_leaf;     // DFS leaf order (culled walk)
    const DTri* tris_orig;     // original order (reference walk)
    const DShade* shade;
    const DMat* mats;
    const DLight* lights;
    const uint32_t* jump;
    const uint32_t* jump_bytes;     // byte-position jump matrices J(b << 8) and J(b << 16), b < 256,
                                    // byte-sliced (build_jump_byte_tables); null: per-bit jumps only
    const uint32_t* seed_states;    // curand_init(seed, s0, 0) for s0 < 256: v0..v4 (kJumpEntryWords
                                    // words each; seed_table), with jump_bytes
    float* out;
    unsigned long long* counters;   // kCounterWords words, slots CNT_*
    uint32_t* tile_counter;
    uint32_t num_lights;
    float total_light_area;
    float root[6];
    Cam cam;
    int32_t w, h, spp, bounces;
    uint32_t flags;
    uint64_t seed;
    int32_t shard_index, shard_count;
    uint32_t tiles_x, ntiles_shard;
    uint32_t tile_w, tile_h;        // shard tile (multiples of 8): 8x8 blocks of 64 work slots, row-major
    uint32_t tile_bx, tile_blocks;  // 8x8 blocks per tile row / per tile
    uint32_t morton_out;            // PT_ORDER_MORTON: pixel (x,y) written at out[mortonPxltoI(x,y)*3]
    uint32_t stack_words;           // LDS words per wave
    float cull_rel, cull_abs;
    uint32_t* pixel_counter;        // wavefront kernel: next pixel unit
    uint32_t nunits;                // work units: npix * chunks
    uint32_t scene_fast;            // all scene coordinates admit the Markstein quotient
    uint32_t wf_threshold;          // leave the walk when this many lanes wait for shading
    uint32_t wf_iters;              // shading iterations a lane may run per pass before yielding
    uint32_t node_mask;             // low bits of a packed stack entry holding the node index
    uint32_t top_nodes;             // wavefront kernel: BVH4 nodes 0..top_nodes-1 staged in LDS
    uint32_t root_first;            // wavefront kernel: a new ray's root visit in the shading pass (begin_trace)
    uint32_t unit_queues;           // wavefront kernel: units dealt from kQueues counters (> 1) or one
    uint32_t tile_fast4;            // tile kernel: trace with the render-path BVH4 walk (winner check, exact
                                    // slow walk as fallback) instead of the reference-BVH culled walk
    const DNode4* nodes4;           // render-path BVH4 (collapsed SAH BVH)
    const DTri* acc_tris;           // its leaf-order triangle records (id, reference rank, parent)
    const uint32_t* rparent;        // reference BVH: parent of each node (winner chain check)
    const float4* hrec;             // per render-path slot, 48 B: {reference parent's lo, hi.x}, {hi.y, hi.z,
                                    // parent index, triangle id}, {normal, material} -- the winner check's
                                    // words (both integrators) and, for integrator 0, the checked hit's
                                    // shading normal and material on the same line
    uint32_t* spill;                // LDS-stack overflow, entry k of lane g at spill[(k-kRing)*stride + g]
    uint32_t spill_stride;
    uint32_t cold_stride;           // records of the cold array (one per resident lane)
    float acc_root[6];
    uint32_t* cold;                 // per-lane shading state of the wavefront kernel (ColdRec)
    const uint32_t* pix_states;     // per work unit u, word k at [k*nunits + u] (kUnitWords, init_pixel_states)
    uint32_t npix;                  // pixel slots of this shard (ntiles_shard * tile_w * tile_h)
    uint32_t nwhole;                // slots 0..nwhole-1 are whole-pixel units (unit u = slot u); the
    uint32_t ntail;                 // ntail = npix - nwhole last slots are split: the first nmid of them
    uint32_t nmid;                  // into chunks_mid sample chunks, the rest into `chunks`; units are
    uint32_t chunks_mid;            // numbered whole, then mid (chunk-major), then the rest (chunk-major)
    uint32_t chunks;                // (init_pixel_states writes each unit's pixel and sample range)
    uint32_t nfin;                  // ... of which the last nfin slots form a third grade of chunks_fin
    uint32_t chunks_fin;            // chunks (the queue's final, shortest units)
    uint32_t* pmemo;                // split slots: primary hit of tail slot t as one 64-bit word: lo = tri + 2
                                    // (0 = not yet), hi = t
    double* lbuf;                   // split slots: per-sample radiance, channel k of sample n of tail slot t
                                    // at lbuf[((n-1) * ntail + t) * 3 + k] (sample-major: a wave of
                                    // finalize_pixels reads 64 slots' sample n as 1.5 KB in a row)
    const float4* spheres;          // sphere primitives: center xyz, radius (hit ids num_tris + i)
    uint32_t num_spheres;
    uint32_t num_tris;
    uint32_t sphere_mat_base;       // material of sphere i = mats[sphere_mat_base + i]
    uint32_t* tri_counts;           // PT_FLAG_COUNT: per-triangle test counts by original id (kernel.cu:133)
    const float4* shade_m;          // per triangle 48 B: {normal, Le.r}, {albedo, Le.g}, {Le.b, material, -, -} --
                                    // the material's f64 colours as floats, set only when every material's colours
                                    // are float-exact (MTL values are floats): one fetch per bounce, not two
                                    // dependent ones (shade, then mats); null: shade + mats
    const DTri* emis;               // last-bounce light probe: the emissive triangles' records (see begin_trace)
    uint32_t num_emis;              // 0 = probe off
    uint32_t rec_shading;           // integrator 0's checked hits take their normal and material from hrec (a
                                    // scene larger than the LDS top); 0: from shade_m by triangle id (a tree
                                    // held whole in LDS -- C2 -- where that one fetch is an L2 hit anyway)
    unsigned long long* lane_times; // diagnostic (PT_LANE_TIMING): wall clock of each lane's end, then each
                                    // wave's start and exit (render_unidir_wf), or null
    uint32_t head;                  // integrator 1 on the wavefront kernel (init_pixel_states' replay)
    // A pass of an accumulator (pt_accum_add; kAccum kernels): spp is then the samples of THIS pass, which
    // are the pixel's samples acc_n0 + 1 .. acc_n0 + spp.  (New fields go here, at the end: the offsets
    // above are what the plain kernels' scalar loads were tuned with.)
    uint32_t accum;                 // 1: accumulating pass
    uint32_t acc_n0;                // samples every pixel of the shard has already (N)
    float origin_max;               // trace_rays, primary_features: largest |o_k| of a regular ray (ray_regular):
                                    // 64 scene extents, near_camera()'s rule per ray.  (It fills the 4 bytes of
                                    // padding before acc_rng: no offset moves and the struct does not grow.)
    uint32_t* acc_rng;              // per pixel slot q: XORWOW after its last finished sample, word k (v0..v4, d)
                                    // at [k * npix + q] (a wave's 64 slots: one 256-B row per word)
    double* acc_mean;               // per pixel slot q: the f64 running mean, channel k at [k * npix + q]
    // The oriented camera (pt_view; camera_ray_view).  At the very end for the same reason: a NULL view is
    // today's code, and every offset above -- what the kernels' scalar loads were tuned with -- stays where it is.
    uint32_t oriented;              // 1: rays through the view below; 0: the reference camera (camera_ray)
    float view_right[3], view_up[3], view_back[3];   // world-space images of camera +x, +y, +z
    float film_w, film_h;           // film extent (1, 1 = the reference's unit square)
};
// A render along a caller's rays (pt_render_rays*): Args with the ray buffer appended at its end.  Only the kRays
// kernels take it -- as their one struct argument, so what they share with the other kernels reads it as the Args it
// begins with -- and every other kernel keeps its argument block, byte for byte.
struct RayArgs : Args {
    const float* rays;              // {o.xyz, d.xyz} of pixel (x, y) at its out_pixel index
};
// Slots of Args::counters: the kernels add to them; pt_render_wait (pt_stats, PT_SECTION_DUMP) and
// pt_trace_counts read them.
enum : uint32_t {
    CNT_TRACED = 0, CNT_REFERENCE, CNT_NODES, CNT_TRIS, CNT_SAMPLES, CNT_WALK_SLOTS, CNT_LEAF_STEPS, CNT_SHADE_SLOTS,
    CNT_FALLBACKS, CNT_WALK_CYCLES, CNT_SHADE_CYCLES, CNT_TRACE_SLOTS, CNT_START_WAIT, CNT_TOP_VISITS,
    CNT_ITERS = 14,                     // 6 classes of walk iterations
    CNT_T_START = 20, CNT_T_DRAINED,    // wall-clock minima (atomicMin: they start as ~0, not 0)
    CNT_T_LAST_EXIT, CNT_T_EXIT_SUM, CNT_WAVES, CNT_SPILL, CNT_LANE_END_SUM,
    CNT_SECTIONS = 32,                  // kSections section counts, then kHist walk-length buckets
    CNT_LANE_BINS = 64, CNT_WAVE_BINS = 80   // kTailBins each
};
static_assert(offsetof(Args, origin_max) + 4 == offsetof(Args, acc_rng), "origin_max sits in Args' padding");
static_assert(offsetof(Args, oriented) == offsetof(Args, acc_mean) + 8, "the view's words follow everything else");
static_assert(sizeof(Args) % 8 == 0 && sizeof(RayArgs) == sizeof(Args) + 8, "the ray buffer directly follows Args");
constexpr int kCounterWords = 96;
// Unit words of an accumulating pass: UW_N0 bit 30 marks a pixel's first unit of the pass (chunk 0, or the
// whole pixel) -- `n == 1` no longer does; its sample numbers are the 30 bits below.
constexpr uint32_t kUnitFirst = 0x40000000u;
constexpr uint32_t kAccumMaxSamples = kUnitFirst - 1u;

__device__ __forceinline__ V3 ld_norm(const DShade* s, int32_t tri)
{
    const float4 q = *reinterpret_cast<const float4*>(s + tri);
    return v3(q.x, q.y, q.z);
}
__device__ __forceinline__ int32_t ld_mat(const DShade* s, int32_t tri) { return s[tri].mat; }

// ------------------------------------------------------------------ spheres
// The reference has sphere.h but no sphere code; the semantics are this build's, shared with
// the oracle (or_sphere_t): unit d, oc = o - c, b = oc.d, disc = b*b - (oc.oc - r*r), nearer
// root -b - sqrt(disc) if > 0, else -b + sqrt(disc) if > 0.  Spheres are tested after every
// triangle with strict <, so a tie keeps the triangle.
__device__ __forceinline__ float sphere_t(V3 o, V3 d, float4 sp)
{
    const V3 oc = o - v3(sp.x, sp.y, sp.z);
    const float b = dot(oc, d);
    const float c = dot(oc, oc) - sp.w * sp.w;
    const float disc = b * b - c;
    if (!(disc >= 0.0f)) return kMaxFloat;
    const float q = sqrtf(disc);
    float t = -b - q;
    if (t > 0.0f) return t;
    t = -b + q;
    if (t > 0.0f) return t;
    return kMaxFloat;
}
// closest of (htri, ht) and the spheres
__device__ __forceinline__ void apply_spheres(const Args& a, V3 o, V3 d, int32_t* htri, float* ht)
{
    for (uint32_t k = 0; k < a.num_spheres; ++k) {
        const float t = sphere_t(o, d, a.spheres[k]);
        if (0.0f < t && t < *ht) { *ht = t; *htri = (int32_t)(a.num_tris + k); }
    }
}
// primitive id -> material index / normal at p (spheres: (p - c) / r)
__device__ __forceinline__ int32_t prim_mat(const Args& a, int32_t id)
{
    return ((uint32_t)id < a.num_tris) ? ld_mat(a.shade, id) : (int32_t)(a.sphere_mat_base + ((uint32_t)id - a.num_tris));
}
__device__ __forceinline__ V3 prim_normal(const Args& a, int32_t id, V3 p)
{
    if ((uint32_t)id < a.num_tris) return ld_norm(a.shade, id);
    const float4 sp = a.spheres[(uint32_t)id - a.num_tris];
    return (p - v3(sp.x, sp.y, sp.z)) / sp.w;
}

// ------------------------------------------------------------------ per-lane tracer
template <bool kRefWalk, bool kCount>
struct Tracer {
    const Args* a;
    uint32_t* stack;
    int lane;
    Counters cnt;
    uint32_t traced;
    uint32_t reference;
    // primary-ray memo (exact: keyed on the ray's bits)
    bool have;
    uint32_t ko[3], kd[3];
    Hit kh;


    __device__ __forceinline__ Hit trace(V3 o, V3 d)
    {
        ++traced;
        Hit h;
        h.tri = -1;
        h.t = kMaxFloat;
        if (a->num_tris > 0) {
            if (kRefWalk) {
                h = trace_reference<kCount>(o, d, a->rnodes, a->tris_orig, stack, lane, cnt);
            } else if (a->tile_fast4) {
                // the wavefront kernel's walk, run to its end by this lane (DESIGN.md "Traversal"); its
                // LDS rings (this block's one wave) and HBM spill column
                const uint32_t lane_off = (blockIdx.x * 64u + (uint32_t)lane) * 4u;
                Stack4 S;
                S.ring = stack + lane;
                S.stride = a->spill_stride;
                S.spill_base = a->spill;
                S.lane_off = &lane_off;
                S.off_mask = ~0u;
                if ((a->scene_fast != 0u) && ray_fast(o, d)) {
                W4 w;
                if (walk4_begin(w, o, d, a->acc_root, a->cull_abs)) {
                    while (walk4_step<kCount>(w, o, d, a->nodes4, a->acc_tris, S, a->cull_rel, a->cull_abs, a->node_mask,
                                              cnt)) {
                    }
                    h.t = w.best_t;
                    bool ok = true;
                    if (w.best_slot != kNone) {
                        const float4 C = a->acc_tris[w.best_slot].c;
                        h.tri = (int32_t)__float_as_uint(C.y);
                        ok = ref_tested(__float_as_uint(C.w), o, d, a->rnodes, a->rparent);
                    }
                    if (!ok) {
                        atomicAdd(a->counters + CNT_FALLBACKS, 1ull);   // (accel_fallbacks, as trace_rays counts them)
                        trace_slow(o, d, a->root, a->nodes, a->tris_leaf, S.spill(), S.stride, a->cull_rel, a->cull_abs,
                                   &h.tri, &h.t, cnt.tri_counts);
                    }
                }
                } else {   // outside the Markstein preconditions: the exact slow walk
                    atomicAdd(a->counters + CNT_FALLBACKS, 1ull);
                    trace_slow(o, d, a->root, a->nodes, a->tris_leaf, S.spill(), S.stride, a->cull_rel, a->cull_abs,
                               &h.tri, &h.t, cnt.tri_counts);
                }
            } else {
                h = trace_culled<kCount>(o, d, a->root, a->nodes, a->tris_leaf, stack, lane, a->cull_rel, a->cull_abs, cnt);
            }
        }
        if (a->num_spheres) apply_spheres(*a, o, d, &h.tri, &h.t);
        return h;
    }

    __device__ Hit trace_primary(V3 o, V3 d, bool memo)
    {
        ++reference;
        if (memo && have && ko[0] == __float_as_uint(o.x) && ko[1] == __float_as_uint(o.y) &&
            ko[2] == __float_as_uint(o.z) && kd[0] == __float_as_uint(d.x) && kd[1] == __float_as_uint(d.y) &&
            kd[2] == __float_as_uint(d.z))
            return kh;
        Hit h = trace(o, d);
        if (memo) {
            have = true;
            ko[0] = __float_as_uint(o.x); ko[1] = __float_as_uint(o.y); ko[2] = __float_as_uint(o.z);
            kd[0] = __float_as_uint(d.x); kd[1] = __float_as_uint(d.y); kd[2] = __float_as_uint(d.z);
            kh = h;
        }
        return h;
    }

    __device__ Hit trace_secondary(V3 o, V3 d)
    {
        ++reference;
        return trace(o, d);
    }
};


// kernel.cu:44-54
__device__ __forceinline__ V3 get_tangent(V3 n)
{
    const V3 c1 = cross(n, v3(0, 0, 1));
    const V3 c2 = cross(n, v3(0, 1, 0));
    return (dot(c1, c1) > dot(c2, c2)) ? c1 : c2;
}
__device__ __forceinline__ V3 to_frame(V3 n, float lx, float ly, float lz)   // kernel.cu:70-75, 91-96
{
    const V3 tg = get_tangent(n);
    const V3 bt = cross(n, tg);
    return normalized(n * ly + tg * lx + bt * lz);
}
__device__ __forceinline__ V3 cosine_ray(V3 n, Rng& rng)                     // kernel.cu:78-99
{
    const float u1 = rng_uniform(rng);
    const float u2 = rng_uniform(rng);
    const float r = sqrtf(u1);
    const float theta = (float)(2 * 3.14159 * (double)u2);
    float s, c;
    det_sincos(theta, &s, &c);
    const float x = r * c;
    const float z = r * s;
    const float y = sqrtf(__builtin_fmaxf(0.0f, 1.0f - u1));
    return to_frame(n, x, y, z);
}
__device__ __forceinline__ V3 rand_ray(V3 n, Rng& rng)                       // kernel.cu:60-77
{
    const float u1 = rng_uniform(rng);
    const float u2 = rng_uniform(rng);
    const float r = sqrtf(1.0f - u1 * u1);
    const float phi = (float)(2 * 3.14159 * (double)u2);
    float s, c;
    det_sincos(phi, &s, &c);
    return to_frame(n, r * c, u1, r * s);
}
__device__ __forceinline__ C3 mat_albedo(const DMat* m) { return c3(m->albedo[0], m->albedo[1], m->albedo[2]); }
__device__ __forceinline__ C3 mat_emission(const DMat* m) { return c3(m->emission[0], m->emission[1], m->emission[2]); }
__device__ __forceinline__ C3 brdf(const DMat* m) { return cmulf(mat_albedo(m), (float)(1 / 3.14159)); }  // kernel.cu:101-104

// Area-CDF pick over the light records lt[0..num_lights) (global, or staged in LDS), ra = total area * u
// (kernel.cu:466-495 / 231-262); num_lights is the slot of triangle 0 (nothing picked).  The scan stops once
// randArea <= 0: no later light can then satisfy randArea > 0 (areas are >= 0), so the selection is unchanged.
__device__ __forceinline__ uint32_t light_scan(const DLight* lt, uint32_t num_lights, float ra)
{
    uint32_t sel = num_lights;
    for (uint32_t j = 0; j < num_lights && ra > 0; ++j) {
        const float area = lt[j].area;
        if (ra < area && ra > 0) sel = j;
        ra -= area;
    }
    return sel;
}
// uniform point of a sphere light (d8): z = 1 - 2u, phi = 2*3.14159*v
__device__ __forceinline__ V3 light_point_sphere(const DLight& L, float u, float v)
{
    const float z = 1.0f - 2.0f * u;
    const float rxy = sqrtf(__builtin_fmaxf(0.0f, 1.0f - z * z));
    const float phi = (float)(2 * 3.14159 * (double)v);
    float si, co;
    det_sincos(phi, &si, &co);
    return v3(L.v0[0], L.v0[1], L.v0[2]) + v3(rxy * co, rxy * si, z) * L.a1[0];
}
__device__ __forceinline__ int32_t pick_light(const Args& a, Rng& rng, V3* p)
{
    const uint32_t sel = light_scan(a.lights, a.num_lights, a.total_light_area * rng_uniform(rng));
    float u = rng_uniform(rng);
    float v = rng_uniform(rng);
    const DLight& L = a.lights[sel];
    if (L.pad != 0.0f) {
        *p = light_point_sphere(L, u, v);
        return L.tri;
    }
    const V3 v0 = v3(L.v0[0], L.v0[1], L.v0[2]);
    const V3 a1 = v3(L.a1[0], L.a1[1], L.a1[2]);
    const V3 a2 = v3(L.a2[0], L.a2[1], L.a2[2]);
    if ((double)(u + v) > 1.0) {
        u = (float)((double)u + 2 * (0.5 - (double)u));
        v = (float)((double)v + 2 * (0.5 - (double)v));
    }
    *p = v0 + a1 * u + a2 * v;
    return L.tri;
}

// ------------------------------------------------------------------ integrator 0
// radianceAlongSingleStep2, kernel.cu:417-515.  Dead-path skip: once weight == 0 every later
// bounce adds weight*Le = 0, so (unless PT_FLAG_NO_DEAD_PATH_SKIP) the lane stops tracing and
// only replays the RNG draws each remaining bounce would make (1 + 2, or 1 + 3 and the
// i = max(i, D-2) jump), keeping its stream aligned with the reference.
template <bool kRefWalk, bool kCount>
__device__ C3 radiance_unidir(const Args& a, Tracer<kRefWalk, kCount>& tr, V3 o, V3 dir, Rng& rng, bool skip_dead,
                              bool memo)
{
    C3 accum = c3(0, 0, 0);
    C3 weight = c3(1, 1, 1);
    const int D = a.bounces;
    for (int i = 0; i < D; ++i) {
        if (skip_dead && i > 0 && czero(weight)) {
            ++tr.reference;
            const float u = rng_uniform(rng);
            if (u < 0.5) { rng_next(rng); rng_next(rng); }
            else { rng_next(rng); rng_next(rng); rng_next(rng); i = (i > D - 2) ? i : D - 2; }
            continue;
        }
        Hit h = (i == 0) ? tr.trace_primary(o, dir, memo) : tr.trace_secondary(o, dir);
        int32_t tri = h.tri;
        float t = (float)((double)h.t - 0.001);                                 // :431
        if ((double)t < 0.001) weight = c3(0, 0, 0);                             // :432
        if (t > kMaxFloat - 1) { weight = c3(0, 0, 0); tri = 0; t = 0; }         // :436
        const V3 pos = o + dir * t;                                               // :449
        const DMat* cm = a.mats + prim_mat(a, tri);
        const V3 normal = prim_normal(a, tri, pos);
        if (cm->emission[0] != 0) {                                               // :453
            accum = cadd(accum, cmul(weight, mat_emission(cm)));
            weight = c3(0, 0, 0);
        }
        V3 ldir;
        const float u = rng_uniform(rng);
        if (u < 0.5) {                                                            // :460
            ldir = cosine_ray(normal, rng);
            weight = cmul(weight, cmulf(brdf(cm), (float)3.14159));
        } else {                                                                  // :466
            V3 p1;
            pick_light(a, rng, &p1);
            const V3 d = p1 - pos;
            ldir = normalized(d);
            const float inv_prob = a.total_light_area;
            const float cos_l = __builtin_fmaxf(0.0f, dot(ldir, normal));
            const float cos_o = __builtin_fmaxf(0.0f, dot(v3(0, -1, 0), ldir * -1));
            const float G = cos_l * cos_o / dot(d, d);
            weight = cmul(weight, cmulf(cmulf(brdf(cm), G), inv_prob));
            i = (i > D - 2) ? i : D - 2;
        }
        o = pos;
        dir = ldir;
    }
    return accum;
}

// ------------------------------------------------------------------ integrator 1
__device__ __forceinline__ float geo_term(V3 xa, V3 xb, V3 na, V3 nb)      // kernel.cu:370-373
{
    const V3 seg = xa - xb;
    const V3 ray = normalized(seg);
    float G = __builtin_fabsf(dot(ray, na) * dot(ray, nb)) / dot(seg, seg);
    if (G != G) G = 0;
    return G;
}

// radianceAlongSingleStep, kernel.cu:217-415 (decision d2: a miss on the camera's second
// bounce uses triangle 0 and t = 0 instead of reading tris[-1]).
template <bool kRefWalk, bool kCount>
__device__ C3 radiance_head(const Args& a, Tracer<kRefWalk, kCount>& tr, V3 cam_o, V3 cam_d, Rng& rng, bool memo)
{
    V3 x[5], nrm[5];
    int32_t mat[5] = {0, 0, 0, 0, 0};
    float ip[5];
    {
        V3 p;
        const int32_t sel = pick_light(a, rng, &p);
        const V3 n = prim_normal(a, sel, p);
        x[0] = p + n * 0.001f;
        nrm[0] = n;
        mat[0] = prim_mat(a, sel);
        ip[0] = a.total_light_area;
    }
    {
        const V3 od = rand_ray(nrm[0], rng);
        Hit h = tr.trace_secondary(x[0], od);
        int32_t tri = h.tri;
        float t = (float)((double)h.t - 0.001);
        if (t > kMaxFloat - 1) { tri = 0; t = 0; }
        const V3 pos = x[0] + od * t;
        const V3 n2 = prim_normal(a, tri, pos);
        const float G = __builtin_fabsf(dot(n2, od)) / __builtin_fmaxf(0.001f, t * t);
        x[1] = pos; nrm[1] = n2; mat[1] = prim_mat(a, tri);
        ip[1] = (float)(2 * 3.14159 / (double)G);
    }
    x[4] = cam_o; nrm[4] = cam_d; ip[4] = 1;
    {
        Hit h = tr.trace_primary(cam_o, cam_d, memo);
        int32_t tri = h.tri;
        float t = (float)((double)h.t - 0.001);
        if (t > kMaxFloat - 1) { tri = 0; t = 0; }
        x[3] = cam_o + cam_d * t;
        nrm[3] = prim_normal(a, tri, x[3]);
        mat[3] = prim_mat(a, tri);
        ip[3] = 1;
    }
    {
        const V3 d = cosine_ray(nrm[3], rng);
        Hit h = tr.trace_secondary(x[3], d);
        int32_t tri = h.tri;
        float t = (float)((double)h.t - 0.001);
        if (t > kMaxFloat - 1 || tri < 0) { tri = 0; t = 0; }
        x[2] = x[3] + d * t;
        const V3 n = prim_normal(a, tri, x[2]);
        float G = __builtin_fabsf(dot(nrm[3], d) * dot(n, d)) / (t * t);
        if (G == 0) G = 1;
        if (G != G) G = 1;
        nrm[2] = n;
        mat[2] = prim_mat(a, tri);
        ip[2] = (float)(3.14159 / (double)G);
    }
    C3 accum = c3(0, 0, 0);
    const C3 le = mat_emission(a.mats + mat[0]);
    const C3 e3 = mat_emission(a.mats + mat[3]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 2; j < 4; ++j) {
            C3 w = cmulf(le, ip[0]);
#pragma unroll
            for (int k = 1; k <= i; ++k) {
                const float G = geo_term(x[k], x[k - 1], nrm[k], nrm[k - 1]);
                w = cmulf(cmulf(cmul(w, cdivf(mat_albedo(a.mats + mat[k]), 3.14159f)), G), ip[k]);
            }
#pragma unroll
            for (int k = j + 1; k < 4; ++k) {
                const float G = geo_term(x[k], x[k - 1], nrm[k], nrm[k - 1]);
                w = cmulf(cmulf(cmul(w, cdivf(mat_albedo(a.mats + mat[k]), 3.14159f)), G), ip[k]);
            }
            const V3 seg = x[j] - x[i];
            const float len = length(seg);
            const V3 ray = normalized(seg);
            float G = __builtin_fmaxf(0.0f, dot(ray, nrm[j]) * dot(ray * -1, nrm[i])) / dot(seg, seg);
            if (G != G) G = 0;
            w = cmulf(cmulf(cmul(w, cdivf(mat_albedo(a.mats + mat[j]), 3.14159f)), G), ip[j]);
            const float m = (float)fmax(w.r, fmax(w.g, w.b));
            float V = 0;
            if ((double)m > 0.01) {
                Hit h = tr.trace_secondary(x[i], ray);
                if ((double)__builtin_fabsf(h.t - len) <= 0.01) V = 1;
            }
            w = cmulf(w, V);
            accum = cadd(accum, w);
            accum = cadd(accum, e3);
        }
    }
    return accum;
}

// ------------------------------------------------------------------ camera (camera.h:77-97)
// A kernel-argument value made opaque at its use, so that the compiler derives what it needs from
// it there (e.g. a conversion) instead of hoisting the result out of the persistent loop into
// registers that stay live across the walk (where they cost spills).
template <typename T>
__device__ __forceinline__ T fresh(T x)
{
    asm volatile("" : "+s"(x));
    return x;
}

// (kFresh: the image size made opaque at its use -- the wavefront kernel's register discipline; the
// tile kernel, whose arguments may live in memory, takes them as they are)
template <bool kFresh = true>
__device__ __forceinline__ void camera_ray(const Cam& cam, uint32_t px, uint32_t py, bool lens, float u1, float u2,
                                           V3* o, V3* d)
{
    const int cw = kFresh ? fresh(cam.w) : cam.w, ch = kFresh ? fresh(cam.h) : cam.h;
    V3 film = v3((float)px / (float)cw - 0.5f, (float)py / (float)ch - 0.5f, 0.0f);
    V3 lo = v3(0.0f, 0.0f, 0.0f);
    if (lens) {
        const float r = cam.radius * sqrtf(u1);
        const float theta = (float)(2 * 3.14159 * (double)u2);
        float s, c;
        det_sincos(theta, &s, &c);
        lo = v3(r * c, r * s, 0.0f);
    }
    film.z = cam.dist;
    film = (film * -cam.focal) / cam.dist;
    *o = lo + v3(cam.pos[0], cam.pos[1], cam.pos[2]);
    *d = normalized(film - lo);
}

// The ray of an oriented camera (pt_view, pt.h: no counterpart in the reference): camera_ray's camera-space part
// with the film scaled to film_w x film_h, then the view's basis applied to the direction (and to the lens offset).
// Every operation is rounded on its own (no contraction); a pinhole origin is 0 + pos, as the kernels form it.
// The set-up kernels and integrator 1's wavefront kernels take it under the wave-uniform a.oriented, a branch inside
// the existing instances; integrator 0's wavefront kernels, the tile kernel and the features kernel have instances
// of their own for it (kView), because the branch moved their register allocation.  (kFresh: every word of the view made opaque at its use, as cam's are
// in the wavefront kernels, so nothing of it is hoisted across the walk.)
template <bool kFresh = true>
__device__ __forceinline__ void camera_ray_view(const Args& a, uint32_t px, uint32_t py, bool lens, float u1, float u2,
                                                V3* o, V3* d)
{
    const Cam& cam = a.cam;
    auto w = [](float x) { return kFresh ? fresh(x) : x; };
    const int cw = kFresh ? fresh(cam.w) : cam.w, ch = kFresh ? fresh(cam.h) : cam.h;
    V3 film = v3(((float)px / (float)cw - 0.5f) * w(a.film_w), ((float)py / (float)ch - 0.5f) * w(a.film_h), cam.dist);
    film = (film * -cam.focal) / cam.dist;
    V3 lo = v3(0.0f, 0.0f, 0.0f);
    if (lens) {
        const float r = cam.radius * sqrtf(u1);
        const float theta = (float)(2 * 3.14159 * (double)u2);
        float s, c;
        det_sincos(theta, &s, &c);
        lo = v3(r * c, r * s, 0.0f);
    }
    const V3 c = film - lo;
    const V3 R = v3(w(a.view_right[0]), w(a.view_right[1]), w(a.view_right[2]));
    const V3 U = v3(w(a.view_up[0]), w(a.view_up[1]), w(a.view_up[2]));
    const V3 B = v3(w(a.view_back[0]), w(a.view_back[1]), w(a.view_back[2]));
    *d = normalized(v3((R.x * c.x + U.x * c.y) + B.x * c.z, (R.y * c.x + U.y * c.y) + B.y * c.z, (R.z * c.x + U.z * c.y) + B.z * c.z));
    if (lens)
        *o = v3((R.x * lo.x + U.x * lo.y) + cam.pos[0], (R.y * lo.x + U.y * lo.y) + cam.pos[1], (R.z * lo.x + U.z * lo.y) + cam.pos[2]);
    else
        *o = v3(0.0f, 0.0f, 0.0f) + v3(cam.pos[0], cam.pos[1], cam.pos[2]);
}

// Sub-pixel jitter (PT_FLAG_JITTER, pt.h: no counterpart in the reference).  A sample's first two draws (ua, ub)
// place its camera ray in the pixel's footprint: the offset itself (box), or 0.5 + the inverse CDF of the tent of
// half-width 1 pixel (PT_FLAG_JITTER_TENT).  Every operation rounded on its own, IEEE square root.
__device__ __forceinline__ float jitter_tent(float u)
{
    return (u < 0.5f) ? sqrtf(2.0f * u) - 1.0f : 1.0f - sqrtf(2.0f - 2.0f * u);
}
__device__ __forceinline__ void jitter_offset(uint32_t flags, float ua, float ub, float* jx, float* jy)
{
    if (flags & PT_FLAG_JITTER_TENT) { *jx = 0.5f + jitter_tent(ua); *jy = 0.5f + jitter_tent(ub); }
    else { *jx = ua; *jy = ub; }
}
// The ray of a jittered sample: camera_ray's / camera_ray_view's arithmetic, operation for operation, with
// (px + jx, py + jy) in the place of the pixel's corner (jx = jy = 0 gives their bits).  The view is taken under the
// wave-uniform a.oriented -- the jittered kernels are instances of their own (kJit), one set for both cameras -- and
// only where the two cameras differ (the film's scale, the basis), so the lens offset's sin/cos stands once in them.
// `lens`: the sample drew a lens pair (u1, u2) -- radius != 0 or Morton index 0, as everywhere.
template <bool kFresh = true>
__device__ __forceinline__ void camera_ray_jitter(const Args& a, uint32_t px, uint32_t py, float jx, float jy, bool lens,
                                                  float u1, float u2, V3* o, V3* d)
{
    const Cam& cam = a.cam;
    auto w = [](float x) { return kFresh ? fresh(x) : x; };
    const int cw = kFresh ? fresh(cam.w) : cam.w, ch = kFresh ? fresh(cam.h) : cam.h;
    const uint32_t oriented = kFresh ? fresh(a.oriented) : a.oriented;
    const float sx = (float)px + jx, sy = (float)py + jy;
    V3 film = v3(sx / (float)cw - 0.5f, sy / (float)ch - 0.5f, cam.dist);
    if (oriented) { film.x = film.x * w(a.film_w); film.y = film.y * w(a.film_h); }
    film = (film * -cam.focal) / cam.dist;
    V3 lo = v3(0.0f, 0.0f, 0.0f);
    if (lens) {
        const float r = cam.radius * sqrtf(u1);
        const float theta = (float)(2 * 3.14159 * (double)u2);
        float s, c;
        det_sincos(theta, &s, &c);
        lo = v3(r * c, r * s, 0.0f);
    }
    const V3 c = film - lo;
    const V3 pos = v3(cam.pos[0], cam.pos[1], cam.pos[2]);
    // (one store of each result, after the branch: stores in both arms left the two vectors in scratch)
    V3 dir = c, org = lo + pos;
    if (oriented) {
        const V3 R = v3(w(a.view_right[0]), w(a.view_right[1]), w(a.view_right[2]));
        const V3 U = v3(w(a.view_up[0]), w(a.view_up[1]), w(a.view_up[2]));
        const V3 B = v3(w(a.view_back[0]), w(a.view_back[1]), w(a.view_back[2]));
        dir = v3((R.x * c.x + U.x * c.y) + B.x * c.z, (R.y * c.x + U.y * c.y) + B.y * c.z, (R.z * c.x + U.z * c.y) + B.z * c.z);
        if (lens) org = v3((R.x * lo.x + U.x * lo.y) + pos.x, (R.y * lo.x + U.y * lo.y) + pos.y, (R.z * lo.x + U.z * lo.y) + pos.z);
        else org = v3(0.0f, 0.0f, 0.0f) + pos;
    }
    *d = normalized(dir);
    *o = org;
}
// A pixel draws a lens pair when the camera has a lens or the pixel is Morton index 0 (the reference's quirk):
// what CF_LENS says in a plain render.  In a jittered render every unit carries CF_LENS ("the ray is formed per
// sample"), and the kernels recompute this from the pixel.
__device__ __forceinline__ bool lens_pixel(const Args& a, uint32_t px, uint32_t py)
{
    return ((px | py) == 0u) || (fresh(a.cam.radius) != 0.0f);
}

__device__ __forceinline__ uint32_t morton2(uint32_t x, uint32_t y)   // camera.h:66-75
{
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        r |= ((x >> b) & 1u) << (2 * b);
        r |= ((y >> b) & 1u) << (2 * b + 1);
    }
    return r;
}

// Work slot q of this shard -> pixel: tile q / (tile_w*tile_h) of the shard (tile t = shard_index +
// that * shard_count, row-major over the tile grid), 8x8 block ((q >> 6) mod tile_blocks) of the tile
// (row-major), Morton order within the block -- 64 consecutive slots (a wave's lanes) are one 8x8
// block.  False for a slot outside the image (partial tiles at the right / bottom edge).
// (host and device: pt_shard_pixels exports the same mapping; T = Args or pt::TileGrid)
template <typename T>
__host__ __device__ __forceinline__ bool unit_pixel(const T& a, uint32_t q, uint32_t* px, uint32_t* py)
{
    const uint32_t k = q >> 6, l = q & 63u;
    const uint32_t tl = (a.tile_blocks == 1u) ? k : k / a.tile_blocks;
    const uint32_t b = k - tl * a.tile_blocks;
    const uint32_t t = (uint32_t)a.shard_index + tl * (uint32_t)a.shard_count;
    const uint32_t qx = (l & 1) | ((l >> 1) & 2) | ((l >> 2) & 4);
    const uint32_t qy = ((l >> 1) & 1) | ((l >> 2) & 2) | ((l >> 3) & 4);
    const uint32_t by = (a.tile_bx == 1u) ? b : b / a.tile_bx;
    *px = (t % a.tiles_x) * a.tile_w + (b - by * a.tile_bx) * kTile + qx;
    *py = (t / a.tiles_x) * a.tile_h + by * kTile + qy;
    return *px < (uint32_t)a.w && *py < (uint32_t)a.h;
}
// index of pixel (px, py) in the output buffer (pt_params.pixel_order)
__device__ __forceinline__ size_t out_pixel(const Args& a, uint32_t px, uint32_t py)
{
    return a.morton_out ? (size_t)morton2(px, py) : (size_t)py * (size_t)a.w + px;
}

// A render along a caller's rays (the kRays kernels, whose argument block `a` is the head of a RayArgs): the origin
// and the direction of pixel (px, py), as given.
__device__ __forceinline__ V3 ray_origin(const Args& a, uint32_t px, uint32_t py)
{
    const float* r = static_cast<const RayArgs&>(a).rays + out_pixel(a, px, py) * 6;
    return v3(r[0], r[1], r[2]);
}
__device__ __forceinline__ V3 ray_direction(const Args& a, uint32_t px, uint32_t py)
{
    const float* r = static_cast<const RayArgs&>(a).rays + out_pixel(a, px, py) * 6 + 3;
    return v3(r[0], r[1], r[2]);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ------------------------------------------------------------------ the render kernel
// (kView: the camera ray goes through the view, camera_ray_view -- render_tiles_view, kernels of their own launched
// for an oriented render, so that the plain ones keep their names and compile exactly as they did without it;
// kJit: a jittered render, render_tiles_jitter -- every sample draws its film point first and forms its own ray,
// through the view or not (a.oriented), and the primary memo is off;
// kRays: a render along the caller's rays, render_tiles_rays -- the pixel's ray is read from RayArgs::rays, no sample
// draws a lens pair, Morton index 0 included, and the ray is the same for every sample, so the memo works;
// kPts: an irradiance render, render_tiles_points -- RayArgs::rays holds the pixel's point {p, n}; every sample draws a
// pair and leaves p along cosine_ray(n), the bounces' own function, so there is no memo)
template <int kIntegrator, bool kRefWalk, bool kCount, bool kView, bool kJit = false, bool kRays = false, bool kPts = false>
__device__ __forceinline__ void render_tiles_body(Args& a)
{
    extern __shared__ uint32_t lds_stack[];
    const int lane = threadIdx.x;
    Tracer<kRefWalk, kCount> tr;
    tr.a = &a;
    tr.stack = lds_stack;
    tr.lane = lane;
    if (kCount) tr.cnt.tri_counts = a.tri_counts;
    tr.traced = 0;
    tr.reference = 0;
    unsigned long long samples = 0;
    const bool skip_dead = !(a.flags & PT_FLAG_NO_DEAD_PATH_SKIP);
    const bool memo = !kJit && !kPts && !(a.flags & PT_FLAG_NO_PRIMARY_CACHE);
    for (;;) {
        uint32_t k = 0;   // the next 8x8 block of this shard's tiles (64 work slots)
        if (lane == 0) k = atomicAdd(a.tile_counter, 1u);
        k = __shfl(k, 0, 64);
        if (k >= a.ntiles_shard * a.tile_blocks) break;
        uint32_t px, py;
        if (!unit_pixel(a, k * 64u + (uint32_t)lane, &px, &py)) continue;
        const uint32_t idx = morton2(px, py);
        Rng rng;
        rng_init(rng, a.seed, idx, a.jump);
        const bool lens = !kRays && !kPts && ((idx == 0) || (a.cam.radius != 0.0f));
        tr.have = false;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0;
        for (int n = 1; n <= a.spp; ++n) {
            float u1 = 0.0f, u2 = 0.0f, jx = 0.0f, jy = 0.0f;
            if (kJit) {   // the sample's film point: its first two draws
                const float ua = rng_uniform(rng), ub = rng_uniform(rng);
                jitter_offset(a.flags, ua, ub, &jx, &jy);
            }
            if (lens) { u1 = rng_uniform(rng); u2 = rng_uniform(rng); }
            V3 o, d;
            if (kPts) { o = ray_origin(a, px, py); d = cosine_ray(ray_direction(a, px, py), rng); }   // (the sample's pair is drawn here)
            else if (kRays) { o = ray_origin(a, px, py); d = ray_direction(a, px, py); }
            else if (kJit) camera_ray_jitter<false>(a, px, py, jx, jy, lens, u1, u2, &o, &d);
            else if (kView) camera_ray_view<false>(a, px, py, lens, u1, u2, &o, &d);
            else camera_ray<false>(a.cam, px, py, lens, u1, u2, &o, &d);
            C3 L;
            if (kIntegrator == PT_INTEGRATOR_HEAD) L = radiance_head(a, tr, o, d, rng, memo);
            else L = radiance_unidir(a, tr, o, d, rng, skip_dead, memo);
            const double fn1 = (double)(float)(n - 1), fn = (double)(float)n;   // kernel.cu:551-552
            m0 = (m0 * fn1) / fn + L.r / fn;
            m1 = (m1 * fn1) / fn + L.g / fn;
            m2 = (m2 * fn1) / fn + L.b / fn;
        }
        samples += (unsigned long long)a.spp;
        float* o3 = a.out + out_pixel(a, px, py) * 3;
        o3[0] = (float)m0;
        o3[1] = (float)m1;
        o3[2] = (float)m2;
    }
    const unsigned long long c0 = wave_sum(tr.traced), c1 = wave_sum(tr.reference), c4 = wave_sum(samples);
    unsigned long long c2 = 0, c3v = 0;
    if (kCount) { c2 = wave_sum(tr.cnt.nodes); c3v = wave_sum(tr.cnt.tris); }
    if (lane == 0) {
        atomicAdd(a.counters + CNT_TRACED, c0);
        atomicAdd(a.counters + CNT_REFERENCE, c1);
        atomicAdd(a.counters + CNT_SAMPLES, c4);
        if (kCount) { atomicAdd(a.counters + CNT_NODES, c2); atomicAdd(a.counters + CNT_TRIS, c3v); }
    }
}
template <int kIntegrator, bool kRefWalk, bool kCount>
__global__ __launch_bounds__(64) void render_tiles(Args a)
{
    render_tiles_body<kIntegrator, kRefWalk, kCount, false>(a);
}
template <int kIntegrator, bool kRefWalk, bool kCount>
__global__ __launch_bounds__(64) void render_tiles_view(Args a)
{
    render_tiles_body<kIntegrator, kRefWalk, kCount, true>(a);
}
template <int kIntegrator, bool kRefWalk, bool kCount>
__global__ __launch_bounds__(64) void render_tiles_jitter(Args a)
{
    render_tiles_body<kIntegrator, kRefWalk, kCount, false, true>(a);
}

// ------------------------------------------------------------------ wavefront kernel
// Integrator 0 as a per-lane state machine (the persistent "while-while" scheme): each lane owns
// one pixel at a time and walks through its samples and bounces; the wave alternates between
// (a) BVH walk steps for the lanes that are tracing, kept running until wf_threshold lanes are
// waiting, and (b) a shading pass in which every waiting lane consumes its hit, draws its next
// direction, finishes samples / pixels and fetches new pixels.  Lanes therefore do not idle
// until the slowest ray of the wave is done, which is where the tile kernel loses most time.
// Arithmetic and RNG consumption per lane are exactly those of radianceAlongSingleStep2.
enum : uint32_t { ST_IDLE = 0, ST_TRACE = 1, ST_SHADE = 2, ST_DONE = 3, ST_SLOW = 4, ST_CHECK = 5,
                  ST_WALKED = 6 };   // (walk finished in this walk phase: CHECK / SHADE / SLOW decided after it)

// Per-lane shading state ("cold": not needed while the lane walks) lives in HBM and is loaded /
// stored only around the shading phase, so the walk phase's register footprint is the ray, the
// walk state and the stack -- which is what sets the kernel's occupancy.
// Layout: 16-B cells, lane-major within a cell row -- word w of record g at byte
// ((w / 4) * records + g) * 16 + (w % 4) * 4 -- so the words a pass always needs come as four
// coalesced 16-B-per-lane loads (and stores) instead of fifteen 4-B ones: a vector-memory
// instruction costs about the same address-pipeline time at 4 and at 16 B per lane.
enum : int {
    CW_N = 0, CW_I, CW_FLAGS, CW_RNG_D,       // cell 0
    CW_RNG_V0 = 4,                            // cell 1: v0..v3
    CW_WGT = 8,                               // cells 2, 3.lo: wgt (f64 x 3, lo/hi words)
    CW_RNG_V4 = 14, CW_NEND = 15,             // cell 3.hi: v4, last sample number of the unit
    CW_ACC = 16,                              // cells 4, 5.lo: acc (f64 x 3)
    CW_M = 22,                                // cells 5.hi, 6: running mean m0..m2 (f64)
    CW_PX = 28, CW_PY, CW_MTRI, CW_MT,        // cell 7: pixel, primary memo (tri, t)
    CW_CD = 32,                               // cell 8: camera ray direction of a pinhole unit (CF_CAMC) ...
    CW_Q = 35,                                //         ... and a split unit's tail slot (per-sample buffer row)
    kColdWords = 36
};
// CF_ACC0: the sample's accumulator is 0 (not yet written: the record's acc words are stale)
enum : uint32_t { CF_LENS = 1, CF_HAVE = 2, CF_PRIMARY = 4, CF_OWNER = 8, CF_SHARE = 16, CF_MEMO = 32, CF_CAMC = 64,
                  CF_ACC0 = 128, CF_SPLIT = 256, CF_CHUNK0 = 512 };
// CF_CHUNK0 (integrator 0): a split pixel's first chunk (samples 1..chunk_first(1)) keeps the running mean
// itself, as a whole pixel does, and leaves it in its slot's sample-1 row of lbuf for finalize_pixels to
// continue from.

// Accessed as raw buffer loads/stores: one VGPR lane offset for the whole record and the cell
// offset (w / 4) * stride in an SGPR, so no per-word 64-bit addresses are held across the phase.
// ld/st: one word; ld2/st2: words k, k+1 (k even); ld4/st4: a whole cell (k % 4 == 0).
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
struct ColdRec {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t voff;      // lane byte offset (16 * record)
    uint32_t sbytes;    // bytes between consecutive cells of one record (16 * records)
    __device__ __forceinline__ int vo(int k) const { return (int)(voff + 4u * (uint32_t)(k & 3)); }
    __device__ __forceinline__ int so(int k) const { return (int)((uint32_t)(k >> 2) * sbytes); }
    __device__ __forceinline__ uint32_t ld(int k) const
    {
        return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, vo(k), so(k), 0);
    }
    __device__ __forceinline__ void st(int k, uint32_t v) const
    {
        __builtin_amdgcn_raw_buffer_store_b32(v, rs, vo(k), so(k), 0);
    }
    __device__ __forceinline__ uint2 ld2(int k) const
    {
        const u2v v = __builtin_amdgcn_raw_buffer_load_b64(rs, vo(k), so(k), 0);
        return make_uint2(v.x, v.y);
    }
    __device__ __forceinline__ void st2(int k, uint32_t x, uint32_t y) const
    {
        __builtin_amdgcn_raw_buffer_store_b64(u2v{x, y}, rs, vo(k), so(k), 0);
    }
    __device__ __forceinline__ uint4 ld4(int k) const
    {
        const u4v v = __builtin_amdgcn_raw_buffer_load_b128(rs, vo(k), so(k), 0);
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    __device__ __forceinline__ void st4(int k, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const
    {
        __builtin_amdgcn_raw_buffer_store_b128(u4v{x, y, z, w}, rs, vo(k), so(k), 0);
    }
    __device__ __forceinline__ double ldd(int k) const
    {
        const uint2 v = ld2(k);
        return __hiloint2double((int)v.y, (int)v.x);
    }
    __device__ __forceinline__ void std_(int k, double v) const
    {
        st2(k, (uint32_t)__double2loint(v), (uint32_t)__double2hiint(v));
    }
};
__device__ __forceinline__ double dbl(uint32_t lo, uint32_t hi) { return __hiloint2double((int)hi, (int)lo); }
__device__ __forceinline__ uint32_t dlo(double v) { return (uint32_t)__double2loint(v); }
__device__ __forceinline__ uint32_t dhi(double v) { return (uint32_t)__double2hiint(v); }

// kMinWaves: waves per SIMD the register allocation must allow (launch bound); 4 = 128 VGPRs,
// 5 = 96, 6 = 80 -- more resident waves hide more memory latency, at the price of spilling
// shading-phase values (the walk loop itself stays spill-free down to 96).
// Work unit u = sample chunk c = u / npix of pixel slot q = u % npix: samples
// [c*spp/chunks, (c+1)*spp/chunks).  With one chunk a unit is a whole pixel.
// Per-unit words of init_pixel_states' output beyond the XORWOW state (words 0..5: v0..v4, d)
enum : uint32_t { UW_PXY = 6, UW_N0, UW_NEND, UW_TQ, UW_CD, kUnitWords = UW_CD + 3 };
constexpr uint32_t kNoPixel = 0xffffffffu;   // UW_PXY of a slot outside the image
constexpr uint32_t kNoUnit = 0xffffffffu;
constexpr uint32_t kQueueBlock = 64;         // units per block of a counter's class
constexpr uint32_t kQueueStride = 32;        // words between the counters (one 128-B line each)
// LDS of a wavefront block after the counters: the probe's emitter count (16 B) and records, then the
// staged BVH4 top nodes
// then the NEE light records (lights[0..num_lights], the last being "nothing picked") when at most
// kLdsLights of them: the area-CDF pick and the picked record read LDS, not two dependent fetches
constexpr uint32_t kLdsLights = 5;
constexpr uint32_t kProbeLdsBytes = 16 + kMaxProbeEmitters * (uint32_t)sizeof(DTri) + kLdsLights * (uint32_t)sizeof(DLight);
__device__ __forceinline__ uint32_t chunk_first(const Args& a, uint32_t c, uint32_t chunks)
{
    return (uint32_t)(((uint64_t)c * (uint32_t)a.spp) / chunks);
}
// The chunk count of split slot t (its grade: the first nmid slots mid, the last nfin final, the rest fine) -- the one
// definition init_pixel_states (which deals the chunks), the render kernel (CF_CHUNK0's end) and finalize_pixels
// (which continues chunk 0's running mean from sample chunk_first(1) on) share.
__device__ __forceinline__ uint32_t slot_chunks(const Args& a, uint32_t t)
{
    return t < a.nmid ? a.chunks_mid : t >= a.ntail - a.nfin ? a.chunks_fin : a.chunks;
}

// The XORWOW draws one sample of radianceAlongSingleStep2 consumes, without tracing: the count
// depends only on the draws themselves (lens pair; per bounce u, then 2 for a cosine direction or
// 3 for a light sample, which also jumps i to D-2) -- the same replay as the dead-path skip.
// (jitter: the two draws of a jittered sample's film point, before the lens pair)
__device__ __forceinline__ void replay_sample(Rng& rng, bool lens, int D, bool jitter = false)
{
    if (jitter) { rng_next(rng); rng_next(rng); }
    if (lens) { rng_next(rng); rng_next(rng); }
    int i = 0;
    while (i < D) {
        const float u = rng_uniform(rng);
        if (u < 0.5) { rng_next(rng); rng_next(rng); }
        else { rng_next(rng); rng_next(rng); rng_next(rng); i = (i > D - 2) ? i : D - 2; }
        ++i;
    }
}

// The XORWOW state pixel slot q (Morton index idx) starts a render or a pass from: curand_init, or after
// n_done samples of an accumulator the stream its last sample left (init_pixel_states, init_active_states).
__device__ __forceinline__ void slot_stream(const Args& a, uint32_t q, uint32_t idx, uint32_t n_done, Rng& r)
{
    if (n_done != 0u) {
        // a later pass of an accumulator: the stream continues where the pixel's last sample left it
        const size_t P = a.npix;
        r.v0 = a.acc_rng[q]; r.v1 = a.acc_rng[P + q]; r.v2 = a.acc_rng[2 * P + q];
        r.v3 = a.acc_rng[3 * P + q]; r.v4 = a.acc_rng[4 * P + q]; r.d = a.acc_rng[5 * P + q];
    } else if (a.jump_bytes) {
        // curand_init(seed, idx, 0) = J(idx) v(seed): the jump matrices are powers of one matrix,
        // so they commute and J(idx) = J(idx & 0xff0000) J(idx & 0xff00) J(idx & 0xff) -- the low
        // byte's product is tabulated per render (seed_states), the next two bytes' per context
        // (jump_bytes): 40 lookups instead of 20 per set bit of idx
        uint32_t v[5];
        const uint32_t* p0 = a.seed_states + (size_t)(idx & 255u) * kJumpEntryWords;
        for (int k = 0; k < 5; ++k) v[k] = p0[k];
        const uint32_t b1 = (idx >> 8) & 255u, b2 = (idx >> 16) & 255u;
        constexpr size_t kMat = (size_t)20 * 256 * kJumpEntryWords;
        if (b1) jump_apply(v, a.jump_bytes + (size_t)b1 * kMat);
        if (b2) jump_apply(v, a.jump_bytes + (size_t)(256u + b2) * kMat);
        for (int k = 24; k < 32; ++k)   // (images beyond 4096 x 4096: the remaining bits one by one)
            if ((idx >> k) & 1u) jump_apply(v, a.jump + (size_t)k * kMat);
        r.d = rng_seed_d(a.seed);
        r.v0 = v[0]; r.v1 = v[1]; r.v2 = v[2]; r.v3 = v[3]; r.v4 = v[4];
    } else {
        rng_init(r, a.seed, idx, a.jump);
    }
}

// The direction of pixel (px, py)'s pinhole ray, stored with its units (a lens pixel: 0, its rays are formed per sample).
__device__ __forceinline__ V3 pinhole_dir(const Args& a, uint32_t px, uint32_t py, bool lens)
{
    V3 o, d = v3(0.0f, 0.0f, 0.0f);
    if (!lens) {
        if (a.oriented) camera_ray_view(a, px, py, false, 0.0f, 0.0f, &o, &d);
        else camera_ray(a.cam, px, py, false, 0.0f, 0.0f, &o, &d);
    }
    return d;
}
// This render's counters, unit counters and wall-clock minima, by the first block of the unit set-up kernel
// (no memset launches).
__device__ __forceinline__ void reset_render_counters(const Args& a)
{
    for (uint32_t k = threadIdx.x; k < (uint32_t)kCounterWords; k += 256u)
        a.counters[k] = (k == CNT_T_START || k == CNT_T_DRAINED) ? ~0ull : 0ull;
    for (uint32_t k = threadIdx.x; k < kQueueStride * (kQueues + 1); k += 256u) a.pixel_counter[k] = 0u;
    if (threadIdx.x < 4) a.tile_counter[threadIdx.x] = 0u;
}

// setupCurand (kernel.cu:527-533) for the wavefront kernel: the XORWOW state of every work unit
// of this shard -- curand_init of its pixel, fast-forwarded over the unit's earlier samples --
// computed in parallel before the render, so that a lane starting a unit inside the state
// machine loads 20 B instead of running the jump-ahead with its wave waiting.
// (kJit: the set-up of a jittered render, init_pixel_states_jitter.  No pixel of it has a sample-invariant ray, so
// every unit is marked as a lens unit is -- the ray is formed per sample: no UW_CD direction, no CF_CAMC, no memo --
// and the replay skips two more draws per sample.
// kRays: the set-up of a render along the caller's rays, init_pixel_states_rays.  Every unit is a pinhole unit whose
// direction is the pixel's in RayArgs::rays -- Morton index 0 too: no sample draws a lens pair -- so the memos work.
// kPts: the set-up of an irradiance render, init_pixel_states_points.  Every sample draws a pair and forms its own
// ray, so every unit is marked and replayed as a lens unit is: no UW_CD direction, no CF_CAMC, no memo.)
template <bool kJit, bool kRays = false, bool kPts = false>
__device__ __forceinline__ void init_pixel_states_body(const Args& a, uint32_t* __restrict__ st)
{
    // one lane per pixel slot: curand_init, then one pass over the samples that writes the state
    // at the start of every chunk, with everything else a lane needs to start the unit (pixel,
    // sample range, pinhole camera ray): the refill in the render kernel is then a few loads
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x == 0) reset_render_counters(a);
    if (q >= a.npix) return;
    const bool split = q >= a.nwhole;
    const uint32_t t = q - a.nwhole;   // split slot (row of the per-sample buffer)
    if (split) {   // its primary-hit word (pmemo): none yet
        a.pmemo[2 * t] = 0u;
        a.pmemo[2 * t + 1] = 0u;
    }
    const bool mid = split && t < a.nmid;
    const uint32_t f0 = a.ntail - a.nfin;   // first slot of the final grade
    const bool fin = split && t >= f0;
    const uint32_t nc = split ? slot_chunks(a, t) : 1u;
    auto unit = [&](uint32_t c) -> size_t {
        if (!split) return (size_t)q;
        if (mid) return (size_t)a.nwhole + (size_t)c * a.nmid + t;
        const size_t fine0 = (size_t)a.nwhole + (size_t)a.chunks_mid * a.nmid;
        if (!fin) return fine0 + (size_t)c * (f0 - a.nmid) + (t - a.nmid);
        return fine0 + (size_t)a.chunks * (f0 - a.nmid) + (size_t)c * a.nfin + (t - f0);
    };
    const size_t N = a.nunits;
    uint32_t px, py;
    if (!unit_pixel(a, q, &px, &py)) {   // a slot outside the image (partial tile): no unit
        for (uint32_t c = 0; c < nc; ++c) st[UW_PXY * N + unit(c)] = kNoPixel;
        return;
    }
    const uint32_t idx = morton2(px, py);
    Rng r;
    const uint32_t n_done = a.accum ? a.acc_n0 : 0u;   // samples the pixel has before this render
    slot_stream(a, q, idx, n_done, r);
    const bool lens = kPts || (!kRays && ((idx == 0) || (a.cam.radius != 0.0f)));
    const bool per_sample = kJit || lens;   // the unit's mark: its rays are formed per sample
    const V3 d = kRays ? ray_direction(a, px, py) : pinhole_dir(a, px, py, per_sample);
    uint32_t done = 0;
    for (uint32_t c = 0; c < nc; ++c) {
        const uint32_t s0 = split ? chunk_first(a, c, nc) : 0u;
        if (a.head) {   // integrator 1: a fixed 7 draws per sample (+2 lens, +2 jitter): light pick 3, rand_ray 2, cosine 2
            for (; done < s0; ++done)
                for (int k = (lens ? 9 : 7) + (kJit ? 2 : 0); k > 0; --k) rng_next(r);
        }
        for (; done < s0; ++done) replay_sample(r, lens, a.bounces, kJit);
        const size_t u = unit(c);
        st[u] = r.v0;
        st[N + u] = r.v1;
        st[2 * N + u] = r.v2;
        st[3 * N + u] = r.v3;
        st[4 * N + u] = r.v4;
        st[5 * N + u] = r.d;       // the Weyl counter advances with every draw
        st[UW_PXY * N + u] = px | (py << 16);
        // (an accumulating pass: sample numbers continue from n_done, the pixel's first unit is flagged,
        // and a whole-pixel unit carries its slot -- the row of its stored mean and XORWOW state)
        st[UW_N0 * N + u] = (n_done + s0 + 1u) | (per_sample ? 0x80000000u : 0u) | ((a.accum && c == 0u) ? kUnitFirst : 0u);
        st[UW_NEND * N + u] = n_done + (split ? chunk_first(a, c + 1, nc) : (uint32_t)a.spp);
        st[UW_TQ * N + u] = split ? t : (a.accum ? q : 0u);
        st[UW_CD * N + u] = __float_as_uint(d.x);
        st[(UW_CD + 1) * N + u] = __float_as_uint(d.y);
        st[(UW_CD + 2) * N + u] = __float_as_uint(d.z);
    }
}
__global__ __launch_bounds__(256) void init_pixel_states(Args a, uint32_t* __restrict__ st)
{
    init_pixel_states_body<false>(a, st);
}

// The unit set-up of an adaptive pass (pt_accum_add once a pixel is frozen): one lane per entry u of the active
// list, unit u = the whole pixel of slot q = list[u] -- the words init_pixel_states writes for a whole-pixel
// accumulating unit, whose UW_TQ names the slot: the row (stride npix, the shard's slot count) the integration
// kernels load the unit's mean from and store its mean and stream to.  nunits = nwhole = the list's length.
// (kRays: the active list of a ray accumulator, init_active_states_rays -- a pinhole unit whose direction is the
// pixel's in RayArgs::rays, Morton index 0 too, as in init_pixel_states_body;
// kPts: the active list of a point accumulator, init_active_states_points -- every unit is marked as a lens unit is,
// with no UW_CD direction: a sample draws its pair and forms its ray itself, again as in init_pixel_states_body)
template <bool kJit, bool kRays = false, bool kPts = false>
__device__ __forceinline__ void init_active_states_body(const Args& a, uint32_t* __restrict__ st, const uint32_t* __restrict__ list)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x == 0) reset_render_counters(a);
    const size_t N = a.nunits;
    if (u >= a.nunits) return;
    const uint32_t q = list[u];
    uint32_t px, py;
    if (q >= a.npix || !unit_pixel(a, q, &px, &py)) {   // (the list holds slots of the image only)
        st[UW_PXY * N + u] = kNoPixel;
        return;
    }
    const uint32_t idx = morton2(px, py);
    Rng r;
    slot_stream(a, q, idx, a.acc_n0, r);
    const bool lens = kPts || (!kRays && (kJit || (idx == 0) || (a.cam.radius != 0.0f)));   // (kJit: every unit's rays are formed per sample)
    const V3 d = kRays ? ray_direction(a, px, py) : pinhole_dir(a, px, py, lens);
    st[u] = r.v0;
    st[N + u] = r.v1;
    st[2 * N + u] = r.v2;
    st[3 * N + u] = r.v3;
    st[4 * N + u] = r.v4;
    st[5 * N + u] = r.d;
    st[UW_PXY * N + u] = px | (py << 16);
    st[UW_N0 * N + u] = (a.acc_n0 + 1u) | (lens ? 0x80000000u : 0u) | kUnitFirst;
    st[UW_NEND * N + u] = a.acc_n0 + (uint32_t)a.spp;
    st[UW_TQ * N + u] = q;
    st[UW_CD * N + u] = __float_as_uint(d.x);
    st[(UW_CD + 1) * N + u] = __float_as_uint(d.y);
    st[(UW_CD + 2) * N + u] = __float_as_uint(d.z);
}
__global__ __launch_bounds__(256) void init_active_states(Args a, uint32_t* __restrict__ st, const uint32_t* __restrict__ list)
{
    init_active_states_body<false>(a, st, list);
}

// The per-render table of init_pixel_states: curand_init(seed, s0, 0) for the 256 low bytes s0.
__global__ __launch_bounds__(256) void seed_table(Args a, uint32_t* __restrict__ out)
{
    Rng r;
    rng_init(r, a.seed, threadIdx.x, a.jump);
    uint32_t* e = out + (size_t)threadIdx.x * kJumpEntryWords;
    e[0] = r.v0; e[1] = r.v1; e[2] = r.v2; e[3] = r.v3; e[4] = r.v4;
}

// Per context: the byte-sliced matrices J(b << 8) (m = b) and J(b << 16) (m = 256 + b), b < 256,
// entry (j, x) = J * (x << 8j), each the product of the per-bit matrices J_k of b's set bits
// (applied to the entry's basis combination through the per-bit byte-sliced tables).
__global__ __launch_bounds__(256) void build_jump_byte_tables(const uint32_t* __restrict__ jb, uint32_t* __restrict__ out)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;   // (m, j, x), x fastest
    if (g >= 512u * 20u * 256u) return;
    const uint32_t x = g & 255u, j = (g >> 8) % 20u, m = (g >> 8) / 20u;
    const uint32_t b = m & 255u, shift = (m < 256u) ? 8u : 16u;
    uint32_t v[5] = {0u, 0u, 0u, 0u, 0u};
    v[j >> 2] = x << (8 * (j & 3));
    constexpr size_t kMat = (size_t)20 * 256 * kJumpEntryWords;
    for (uint32_t i = 0; i < 8; ++i)
        if ((b >> i) & 1u) jump_apply(v, jb + (size_t)(shift + i) * kMat);
    uint32_t* e = out + (size_t)g * kJumpEntryWords;
    e[0] = v[0]; e[1] = v[1]; e[2] = v[2]; e[3] = v[3]; e[4] = v[4];
    e[5] = 0u; e[6] = 0u; e[7] = 0u;
}

// The running mean of kernel.cu:551-552 after sample n of radiance l: m * (n-1) / n + l / n, every operation rounded
// on its own.  The six quotients by fn as one IEEE reciprocal + Markstein corrections (RN(x/fn) for finite x clear
// of under/overflow) -- else the whole wave divides.
__device__ __forceinline__ C3 mean_step(int n, double m0, double m1, double m2, C3 l)
{
    const double fn1 = (double)(float)(n - 1), fn = (double)(float)n;
    const double x0 = m0 * fn1, x1 = m1 * fn1, x2 = m2 * fn1;
    if (__ballot(!(quot_ok(x0) && quot_ok(x1) && quot_ok(x2) && quot_ok(l.r) && quot_ok(l.g) && quot_ok(l.b))) == 0ull) {
        const double rf = 1.0 / fn;
        return c3(div_mk_d(x0, fn, rf) + div_mk_d(l.r, fn, rf), div_mk_d(x1, fn, rf) + div_mk_d(l.g, fn, rf),
                  div_mk_d(x2, fn, rf) + div_mk_d(l.b, fn, rf));
    }
    return c3(x0 / fn + l.r / fn, x1 / fn + l.g / fn, x2 / fn + l.b / fn);
}

// Split slots: the running mean of kernel.cu:551-552, in sample order, over the stored
// per-sample radiance of each split pixel of this shard.
__global__ __launch_bounds__(256) void finalize_pixels(Args a)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.ntail) return;
    uint32_t px, py;
    if (!unit_pixel(a, a.nwhole + t, &px, &py)) return;
    const size_t pix = out_pixel(a, px, py);
    const double* L = a.lbuf + (size_t)t * 3;
    const size_t stride = (size_t)a.ntail * 3;   // one sample of every slot
    // integrator 0: chunk 0 left its running mean after samples 1..e0 in the sample-1 row (CF_CHUNK0);
    // integrator 1 stores every sample (its chunk 0 keeping the mean measured -1% on the 1/8 shard)
    const uint32_t e0 = a.head ? 0u : chunk_first(a, 1u, slot_chunks(a, t));
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    // an accumulating pass: the fold continues the slot's stored mean (unless chunk 0 already did), over
    // this pass's rows, with the pixel's own sample numbers nb + 1 .. nb + spp
    const int nb = a.accum ? (int)a.acc_n0 : 0;
    double* const am = a.accum ? a.acc_mean + (size_t)a.nwhole + t : nullptr;
    if (e0 != 0u) { m0 = L[0]; m1 = L[1]; m2 = L[2]; }
    else if (am) { m0 = am[0]; m1 = am[a.npix]; m2 = am[2 * (size_t)a.npix]; }
    L += (size_t)e0 * stride;
    auto step = [&](int n, double l0, double l1, double l2) {
        const C3 m = mean_step(n, m0, m1, m2, c3(l0, l1, l2));
        m0 = m.r; m1 = m.g; m2 = m.b;
    };
    // eight samples' loads issued together, the next eight issued before these are consumed (a wave's
    // loads of one sample are 64 consecutive slots: whole lines)
    int n = (int)e0 + 1;
    double v[24];
    if (n + 7 <= a.spp) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[3 * k] = L[k * stride]; v[3 * k + 1] = L[k * stride + 1]; v[3 * k + 2] = L[k * stride + 2]; }
    }
    for (; n + 7 <= a.spp; n += 8) {
        L += 8 * stride;
        double q[24];
        const bool more = n + 15 <= a.spp;
        if (more) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { q[3 * k] = L[k * stride]; q[3 * k + 1] = L[k * stride + 1]; q[3 * k + 2] = L[k * stride + 2]; }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) step(nb + n + k, v[3 * k], v[3 * k + 1], v[3 * k + 2]);
        if (more) {
#pragma unroll
            for (int k = 0; k < 24; ++k) v[k] = q[k];
        }
    }
    for (; n <= a.spp; ++n, L += stride) step(nb + n, L[0], L[1], L[2]);
    if (am) {
        am[0] = m0; am[a.npix] = m1; am[2 * (size_t)a.npix] = m2;
        if (!a.out) return;
    }
    float* o3 = a.out + pix * 3;
    o3[0] = (float)m0;
    o3[1] = (float)m1;
    o3[2] = (float)m2;
}

// One event per active lane added to an LDS counter with a single atomic per wave.
__device__ __forceinline__ void wave_count(unsigned long long* c, int lane)
{
    const uint64_t m = __ballot(1);
    if (lane == __ffsll((long long)m) - 1) atomicAdd(c, (unsigned long long)__popcll(m));
}

// The shading half of the wavefront state machine, for the lanes that are not tracing: consume
// the pending hit (winner check; exact slow walk when needed), run bounces, finish and start
// samples until the lane needs a trace or its unit is done, then give finished lanes new units.
// On return the lane's state is ST_TRACE (w set up for its ray), ST_SHADE / ST_SLOW (shading
// pending: a memo hit, a root miss or a slow ray right after a refill) or ST_DONE.
// Counting variant only: SEC(k) counts the waves that execute section k of the shading code
// (counters[32 + k]; a profile of where shading issue slots go -- DESIGN.md "Measurement").
enum : int { SEC_PASS = 0, SEC_CHECK, SEC_SLOW, SEC_BOUNCE, SEC_EMIT, SEC_COSINE, SEC_LIGHT, SEC_SAMPLE_END,
             SEC_START, SEC_CAMERA, SEC_DEAD, SEC_BEGIN, SEC_REFILL, SEC_MEMO, SEC_RECORD, SEC_PROBE, kSections = 16 };
constexpr int kHist = 16;   // counting variant: walk steps per ray, log2 buckets (counters[48 + b])
static_assert(CNT_SECTIONS + kSections + kHist <= CNT_LANE_BINS, "counter slots");
constexpr int kTailBins = 16;   // counting variant: lane end / wave exit times after the queue drained,
                                // bin k = [10 us x 2^(k-1), 10 us x 2^k) of the 100-MHz wall clock (bin 0: < 10 us)
static_assert(CNT_LANE_BINS + kTailBins == CNT_WAVE_BINS && CNT_WAVE_BINS + kTailBins == kCounterWords, "counter slots");
__device__ __forceinline__ uint32_t tail_bin(unsigned long long ticks)
{
    const unsigned long long q = ticks / 1000ull;
    return q == 0ull ? 0u : min((uint32_t)kTailBins - 1, 64u - (uint32_t)__clzll((long long)q));
}
#ifdef PT_SEC_MARKERS   // analysis builds: mark the sections in the ISA listing
#define SEC_MARK(k) asm volatile("; SEC " #k)
#else
#define SEC_MARK(k)
#endif
#define SEC(k)                                                                                   \
    do {                                                                                         \
        SEC_MARK(k);                                                                             \
        if (kCount) {                                                                            \
            const uint64_t m_ = __ballot(1);                                                     \
            if (lane == __ffsll((long long)m_) - 1)                                              \
                atomicAdd(reinterpret_cast<uint32_t*>(lcnt + 4) + (k), 1u);                      \
        }                                                                                        \
    } while (0)

// The kernel arguments as the shading pass reads them: from the kernarg segment (render_unidir_wf's
// only explicit argument, at offset 0) through a pointer made opaque at the pass's start, so that the
// scalar loads of the shading-only fields cannot be hoisted to the kernel's entry -- which would keep
// dozens of SGPRs live across the walk loop and push the walk's own values into SGPR spills.
typedef const __attribute__((address_space(4))) Args KArgs;
__device__ __forceinline__ const Args& kernel_args_opaque()
{
    KArgs* p = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const Args*)p;
}

// ------------------------------------------------------------------ shared by the two shading passes
// The refill's unit dealing: lanes `idle` of the wave take the next units of this shard from the unit
// counters; returns this lane's unit (`me`: this lane is idle), a.nunits once every counter is exhausted.
// With unit_queues > 1 the units are dealt from kQueues counters (one 128-B line each), counter x owning the
// blocks j = x (mod kQueues) of kQueueBlock units in order -- so the unit sequence is still taken roughly front
// to back -- each wave starting at its block's counter and moving on when that one is exhausted (the block's LDS
// mask, so every wave of the block and every lane sees the same): the refill's atomics spread over kQueues
// addresses.  Which units a lane gets never changes what it computes.
// Counting variant: a lane that finds the queue drained leaves its end's ticks after the drain and since the
// kernel's start in done_rel (binned at the kernel's end).
template <bool kCount>
__device__ __forceinline__ uint32_t take_unit(const Args& a, int lane, uint64_t idle, bool me, const uint32_t* lprobe,
                                              uint32_t* done_rel)
{
    uint32_t u = kNoUnit;
    if (a.unit_queues > 1u) {
        uint32_t qdone = *reinterpret_cast<volatile const uint32_t*>(lprobe + 1);
        const uint32_t x0 = blockIdx.x & (kQueues - 1u);
        for (uint32_t r = 0; r < kQueues && idle && qdone != (1u << kQueues) - 1u; ++r) {
            const uint32_t x = (x0 + r) & (kQueues - 1u);
            if (qdone & (1u << x)) continue;
            const int leader = __ffsll((long long)idle) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(a.pixel_counter + kQueueStride * (x + 1u), (uint32_t)__popcll(idle));
            base = __shfl(base, leader, 64);
            if (me && u == kNoUnit) {
                const uint32_t k = base + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
                const uint64_t uq = ((uint64_t)(k / kQueueBlock) * kQueues + x) * kQueueBlock + (k % kQueueBlock);
                if (uq < a.nunits) u = (uint32_t)uq;
            }
            const uint64_t left = __ballot(me && u == kNoUnit);
            if (left) {   // (a counter only grows: past its class's end for good)
                qdone |= 1u << x;
                if (lane == leader) atomicOr(const_cast<uint32_t*>(lprobe + 1), 1u << x);
            }
            idle = left;
        }
        if (me && u == kNoUnit) u = a.nunits;   // every counter exhausted
    } else {
        const uint32_t need = (uint32_t)__popcll(idle);
        const int leader = __ffsll((long long)idle) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(a.pixel_counter, need);
        base = __shfl(base, leader, 64);
        if (me) u = base + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
    }
    if (kCount && me && u >= a.nunits) {
        const unsigned long long now = wall_clock64();
        atomicMin(a.counters + CNT_T_DRAINED, now);
        const unsigned long long d0 = __hip_atomic_load(a.counters + CNT_T_DRAINED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long s0 = __hip_atomic_load(a.counters + CNT_T_START, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        done_rel[0] = (uint32_t)min(now - min(now, d0), 0xffffffffull);
        done_rel[1] = (uint32_t)min(now - min(now, s0), 0xffffffffull);
    }
    return u;
}

// The winner check of a finished walk (ST_CHECK; htri: the winner's render-path slot): the winner must be a
// triangle the reference tests (DESIGN.md "Traversal"); if not (rare), the exact reference-BVH walk redoes the
// ray (false: ST_SLOW).  htri becomes the triangle's id.
__device__ __forceinline__ bool check_winner(const Args& a, int32_t& htri, const V3& ro, const V3& rd)
{
    const float4* hr = a.hrec + 3 * (size_t)(uint32_t)htri;
    const float4 b0 = hr[0], b1 = hr[1];
    htri = (int32_t)__float_as_uint(b1.w);
    return ref_tested_box(b0, b1, __float_as_uint(b1.z), ro, rd, a.rnodes, a.rparent);
}

// A hit is at hand (after a walk, the slow walk or the memo): the spheres unless it is a memo, then the primary
// memo's bookkeeping -- a unit's first primary hit goes to the record (words memo_w, memo_w + 1) and, from the
// pixel's owner, to pmemo[the slot in word slot_w] for the pixel's other chunks.
__device__ __forceinline__ void take_hit(const Args& a, const ColdRec& R, int memo_w, int slot_w, uint32_t& fl, V3 ro,
                                         V3 rd, int32_t& htri, float& ht)
{
    if (a.num_spheres && !(fl & CF_MEMO)) apply_spheres(a, ro, rd, &htri, &ht);
    fl &= ~CF_MEMO;
    if (fl & CF_PRIMARY) {
        fl = (fl | CF_HAVE) & ~CF_PRIMARY;
        R.st2(memo_w, (uint32_t)htri, __float_as_uint(ht));
        if (fl & CF_OWNER) {
            const uint32_t q = R.ld(slot_w);
            // (one relaxed 64-bit store: no release, i.e. no write-back of this XCD's L2)
            __hip_atomic_store(reinterpret_cast<uint64_t*>(a.pmemo) + q,
                               ((uint64_t)__float_as_uint(ht) << 32) | (uint32_t)(htri + 2), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            fl &= ~CF_OWNER;
        }
    }
}

// An accumulating pass: the XORWOW state after a pixel's last sample of the pass, to its slot's row ar of acc_rng
// (word k at stride P = npix).
__device__ __forceinline__ void store_stream(size_t P, uint32_t* ar, uint32_t v0, uint32_t v1, uint32_t v2,
                                             uint32_t v3, uint32_t v4, uint32_t d)
{
    ar[0] = v0; ar[P] = v1; ar[2 * P] = v2; ar[3 * P] = v3; ar[4 * P] = v4;
    ar[5 * P] = d;
}

// A whole pixel's unit ends: an accumulating pass keeps the slot's mean and stream for the next pass; the pixel's
// floats go to the image (an accumulating pass: when it has one).
template <bool kAccum>
__device__ __forceinline__ void finish_pixel(const Args& a, uint32_t slot, uint32_t px, uint32_t py, double m0, double m1,
                                             double m2, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t v4,
                                             uint32_t d)
{
    if (kAccum) {
        const size_t P = a.npix;
        double* am = a.acc_mean + slot;
        am[0] = m0; am[P] = m1; am[2 * P] = m2;
        store_stream(P, a.acc_rng + slot, v0, v1, v2, v3, v4, d);
    }
    if (!kAccum || a.out) {
        float* o3 = a.out + out_pixel(a, px, py) * 3;
        o3[0] = (float)m0;
        o3[1] = (float)m1;
        o3[2] = (float)m2;
    }
}

// ------------------------------------------------------------------ wavefront kernel, integrator 0
// kAccum: a pass of an accumulator (Args::accum): a pixel's first unit starts from the slot's stored f64
// mean, the unit that runs a pixel's last sample of the pass stores the XORWOW state back, and a whole
// pixel's unit stores its mean.  Sample numbers, and so the divisors of the mean, continue from acc_n0.
// kView: the lens units' camera ray goes through the view (camera_ray_view); the host launches these instances
// for an oriented render, so the plain ones compile exactly as they did without the view.
// kJit: a jittered render (PT_FLAG_JITTER; instances of their own for the same reason).  Every unit arrives as a lens
// unit (CF_LENS: the ray is formed per sample, so no CF_CAMC and no memo of any kind); a sample draws its film point
// first, then the lens pair if its pixel is a lens pixel (lens_pixel), and takes the view under a.oriented.
// kRays: a render along the caller's rays (RayArgs::rays; instances of their own again).  Every unit arrives as a
// pinhole unit with its direction present (CF_CAMC); a sample's origin is read from the buffer by the pixel's index.
// kPts: an irradiance render (RayArgs::rays holds points {p, n}; instances of their own once more).  Every unit arrives
// as a lens unit; a sample reads its pixel's 24 bytes and leaves p along cosine_ray(n), whose two draws are the
// sample's first.  The memo paths are compiled out.
template <bool kCount, bool kAccum, bool kView = false, bool kJit = false, bool kRays = false, bool kPts = false>
__device__ __forceinline__ void shade_lane(const Args& a_in, const ColdRec& R, int lane, uint32_t& state, V3& ro, V3& rd,
                                           int32_t& htri, float& ht, W4& w, const Stack4& S,
                                           unsigned long long* lcnt, const uint32_t* lprobe, uint32_t* done_rel,
                                           Counters& cnt)
{
    (void)a_in;
    const Args& a = kernel_args_opaque();
    const int D = a.bounces;
    SEC(SEC_PASS);
    // the words every pass needs: four 16-B cells (issued first: their round trip overlaps the
    // winner check's two dependent ones)
    const uint4 k0 = R.ld4(CW_N), k1 = R.ld4(CW_RNG_V0), k2 = R.ld4(CW_WGT), k3 = R.ld4(CW_WGT + 4);
    // the checked winner's slot: the bounce that follows reads its normal and material from the slot's
    // record (the line the check just fetched) instead of the triangle's shading record
    uint32_t hslot = kNone;
    if (state == ST_CHECK) {
        SEC(SEC_CHECK);
        const uint32_t slot = (uint32_t)htri;
        state = check_winner(a, htri, ro, rd) ? ST_SHADE : ST_SLOW;
        if (state == ST_SHADE && a.num_spheres == 0 && a.rec_shading) hslot = slot;
    }
    int n = (int)k0.x, i = (int)k0.y;
    uint32_t fl = k0.z;
    Rng rng;
    rng.d = k0.w; rng.v0 = k1.x; rng.v1 = k1.y; rng.v2 = k1.z; rng.v3 = k1.w; rng.v4 = k3.z;
    uint32_t nend = k3.w;
    C3 wgt = c3(dbl(k2.x, k2.y), dbl(k2.z, k2.w), dbl(k3.x, k3.y));

    // begin a trace of (o, d); true = the lane continues shading at once (root miss, or
    // a ray outside the Markstein preconditions, which takes the exact slow walk).  bound: the walk
    // accepts hits with t < bound (kMaxFloat: a plain trace; see the light probe below)
    auto begin_trace = [&](V3 o, V3 d, float bound) -> bool {
        wave_count(lcnt + 0, lane);
        SEC(SEC_BEGIN);
        // (the wave-uniform tests first, as scalar branches; then one lane mask)
        if (a.num_tris == 0) { htri = -1; ht = kMaxFloat; state = ST_SHADE; return true; }   // spheres only
        if (a.scene_fast == 0u) { state = ST_SLOW; return true; }
        if (!ray_fast_m(o, d)) { state = ST_SLOW; return true; }
        if (!walk4_begin(w, o, d, a.acc_root, a.cull_abs)) {
            htri = -1; ht = kMaxFloat;
            state = (bound == kMaxFloat) ? ST_SHADE : ST_SLOW;
            return true;
        }
        w.best_t = bound;
        state = ST_TRACE;
        return false;
    };
    // start sample n of pixel (px, py): camera ray, then memo or trace
    // (c7 / c8: the record's cells 7 (pixel, memo) and 8 (pinhole direction) when the caller already
    // holds them -- fetched with the previous sample's end, or just written by the refill -- so the
    // start costs no dependent fetch)
    auto start_sample = [&](uint32_t px, uint32_t py, bool have_cells, uint4 c7, uint4 c8) -> bool {
        i = 0;
        fl |= CF_ACC0;   // acc = 0 (stored on the sample's first emission)
        wgt = c3(1, 1, 1);
        float u1 = 0.0f, u2 = 0.0f;
        const bool lens = kPts || (!kRays && (fl & CF_LENS) != 0u);
        float jx = 0.0f, jy = 0.0f;
        bool pair = !kPts && lens;   // the sample draws a lens pair (kPts: cosine_ray draws the sample's pair itself)
        if (kJit) {
            const float ua = rng_uniform(rng), ub = rng_uniform(rng);
            jitter_offset(fresh(a.flags), ua, ub, &jx, &jy);
            pair = lens_pixel(a, px, py);
        }
        if (pair) { u1 = rng_uniform(rng); u2 = rng_uniform(rng); }
        SEC(SEC_START);
        if (!kRays && (lens || !(fl & CF_CAMC))) {
            SEC(SEC_CAMERA);
            if (kPts) { ro = ray_origin(a, px, py); rd = cosine_ray(ray_direction(a, px, py), rng); }
            else if (kJit) camera_ray_jitter(a, px, py, jx, jy, pair, u1, u2, &ro, &rd);
            else if (kView) camera_ray_view(a, px, py, lens, u1, u2, &ro, &rd);
            else camera_ray(a.cam, px, py, lens, u1, u2, &ro, &rd);
            if (!lens) {   // a pinhole ray is the same for every sample of the pixel
                R.st(CW_CD, __float_as_uint(rd.x)); R.st(CW_CD + 1, __float_as_uint(rd.y)); R.st(CW_CD + 2, __float_as_uint(rd.z));
                fl |= CF_CAMC;
            }
        } else {
            if (kRays) ro = ray_origin(a, px, py);   // (12 bytes per sample start; the direction is the record's)
            else ro = v3(0.0f, 0.0f, 0.0f) + v3(fresh(a.cam.pos[0]), fresh(a.cam.pos[1]), fresh(a.cam.pos[2]));   // as camera_ray forms it
            const uint4 cd = have_cells ? c8 : R.ld4(CW_CD);
            rd = v3(__uint_as_float(cd.x), __uint_as_float(cd.y), __uint_as_float(cd.z));
        }
        wave_count(lcnt + 1, lane);
        if (!kPts && (fl & CF_HAVE)) {
            SEC(SEC_MEMO);
            const uint2 mm = have_cells ? make_uint2(c7.z, c7.w) : R.ld2(CW_MTRI);
            htri = (int32_t)mm.x; ht = __uint_as_float(mm.y);
            fl = (fl & ~CF_PRIMARY) | CF_MEMO; state = ST_SHADE;
            return true;
        }
        if (!kPts && (fl & CF_SHARE)) {
            // the pixel's chunk 0 may have published the (sample-invariant) primary hit
            const uint32_t q = have_cells ? c8.w : R.ld(CW_Q);
            // hit and flag in one word: a relaxed agent-scope load (coherent across the XCDs' L2s
            // for this word) needs no acquire, i.e. no invalidation of this XCD's L2
            const uint64_t mv = __hip_atomic_load(reinterpret_cast<uint64_t*>(a.pmemo) + q, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
            if ((uint32_t)mv != 0u) {
                htri = (int32_t)((uint32_t)mv - 2u);
                ht = __uint_as_float((uint32_t)(mv >> 32));
                fl = (fl | CF_PRIMARY | CF_MEMO) & ~CF_SHARE;   // stores the unit memo on shading
                state = ST_SHADE;
                return true;
            }
        }
        fl = (!(a.flags & PT_FLAG_NO_PRIMARY_CACHE) && !lens) ? (fl | CF_PRIMARY) : (fl & ~CF_PRIMARY);
        return begin_trace(ro, rd, kMaxFloat);
    };

    // A lane whose samples need no trace (primary memo hit on an emitter or a miss: the path is
    // dead after bounce 0) would otherwise run sample after sample here while the rest of the
    // wave waits; after wf_iters shading iterations it yields with its pending hit (ST_SHADE /
    // ST_SLOW) and resumes in the next pass, alongside the other lanes' work.
    // The refill (lanes whose unit is finished take the next units of this shard) runs after the
    // first shading iteration, so a unit that starts from a known first hit (a split pixel's memo)
    // is shaded in the second iteration of the same pass instead of waiting out a walk phase.
    bool again = (state == ST_SHADE || state == ST_SLOW);
    for (uint32_t iters = 0; iters < a.wf_iters; ++iters) {
      if (again) {
        again = false;
        if (state == ST_SLOW) {
            wave_count(lcnt + 3, lane);
            SEC(SEC_SLOW);
            trace_slow(ro, rd, a.root, a.nodes, a.tris_leaf, S.spill(), S.stride, a.cull_rel, a.cull_abs,
                       &htri, &ht, kCount ? a.tri_counts : nullptr);
        }
        state = ST_SHADE;
        take_hit(a, R, CW_MTRI, CW_Q, fl, ro, rd, htri, ht);
        // bounce i of radianceAlongSingleStep2 (kernel.cu:427-512) on hit (htri, ht)
        {
            SEC(SEC_BOUNCE);
            int32_t tri = htri;
            float t = (float)((double)ht - 0.001);
            if ((double)t < 0.001) wgt = c3(0, 0, 0);
            if (t > kMaxFloat - 1) { wgt = c3(0, 0, 0); tri = 0; t = 0; }
            const V3 pos = ro + rd * t;
            V3 normal;
            C3 m_em, m_alb;   // the material's emission and albedo (materialDesc, f64)
            if (hslot != kNone) {   // (a checked hit: finite t, so tri is the winner)
                const float4 q2 = a.hrec[3 * (size_t)hslot + 2];
                const DMat* cm = a.mats + (int32_t)__float_as_uint(q2.w);
                normal = v3(q2.x, q2.y, q2.z);
                m_em = mat_emission(cm);
                m_alb = mat_albedo(cm);
                hslot = kNone;
            } else if (a.shade_m && (uint32_t)tri < a.num_tris) {
                const float4* rec = a.shade_m + 3 * (size_t)(uint32_t)tri;
                const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
                normal = v3(q0.x, q0.y, q0.z);
                m_em = c3(q0.w, q1.w, q2.x);
                m_alb = c3(q1.x, q1.y, q1.z);
            } else {
                const DMat* cm = a.mats + prim_mat(a, tri);
                normal = prim_normal(a, tri, pos);
                m_em = mat_emission(cm);
                m_alb = mat_albedo(cm);
            }
            if (m_em.r != 0) {
                SEC(SEC_EMIT);
                C3 acc = c3(0.0, 0.0, 0.0);
                if (!(fl & CF_ACC0)) {
                    const uint4 a01 = R.ld4(CW_ACC);
                    const uint2 a2 = R.ld2(CW_ACC + 4);
                    acc = c3(dbl(a01.x, a01.y), dbl(a01.z, a01.w), dbl(a2.x, a2.y));
                }
                fl &= ~CF_ACC0;
                acc = cadd(acc, cmul(wgt, m_em));
                R.st4(CW_ACC, dlo(acc.r), dhi(acc.r), dlo(acc.g), dhi(acc.g)); R.st2(CW_ACC + 4, dlo(acc.b), dhi(acc.b));
                wgt = c3(0, 0, 0);
            }
            // The two sampling branches (kernel.cu:470-497 light sample, 498-509 cosine) with their
            // common steps done once for the wave instead of once per branch: the draws (cosine:
            // u1, u2; light: area pick, u, v -- the same first two positions), the one sin/cos
            // (cosine theta, or a sphere light's phi), the normalisation and the f64 weight
            // update.  Per lane the operations and their order are those of cosine_ray() /
            // pick_light() + the reference's weight expressions.
            V3 ldir;
            const float u = rng_uniform(rng);
            const bool cosb = u < 0.5;
            const float r1 = rng_uniform(rng), r2 = rng_uniform(rng);
            float r3 = 0.0f;
            const DLight* L = nullptr;
            bool need_sc = cosb;
            float ang = r2;
            if (!cosb) {
                SEC(SEC_LIGHT);
                r3 = rng_uniform(rng);
                // (the records staged in the block's LDS when few; the pick reads them there)
                const DLight* const lt = (a.num_lights < kLdsLights)
                                             ? reinterpret_cast<const DLight*>(lprobe + 4 + kMaxProbeEmitters * 12)
                                             : a.lights;
                L = lt + light_scan(lt, a.num_lights, a.total_light_area * r1);
                if (L->pad != 0.0f) { need_sc = true; ang = r3; }   // sphere light: phi = 2*3.14159*v
            } else {
                SEC(SEC_COSINE);
            }
            float sn = 0.0f, cs = 0.0f;
            if (need_sc) det_sincos((float)(2 * 3.14159 * (double)ang), &sn, &cs);
            V3 vec;   // the direction before normalisation (light: dd = p1 - pos)
            if (cosb) {
                const float r = sqrtf(r1);
                const float x = r * cs, z = r * sn;
                const float y = sqrtf(__builtin_fmaxf(0.0f, 1.0f - r1));
                const V3 tg = get_tangent(normal);
                const V3 bt = cross(normal, tg);
                vec = normal * y + tg * x + bt * z;
            } else {
                V3 p1;
                if (L->pad != 0.0f) {
                    const float zz = 1.0f - 2.0f * r2;
                    const float rxy = sqrtf(__builtin_fmaxf(0.0f, 1.0f - zz * zz));
                    p1 = v3(L->v0[0], L->v0[1], L->v0[2]) + v3(rxy * cs, rxy * sn, zz) * L->a1[0];
                } else {
                    float lu = r2, lv = r3;
                    if ((double)(lu + lv) > 1.0) {
                        lu = (float)((double)lu + 2 * (0.5 - (double)lu));
                        lv = (float)((double)lv + 2 * (0.5 - (double)lv));
                    }
                    p1 = v3(L->v0[0], L->v0[1], L->v0[2]) + v3(L->a1[0], L->a1[1], L->a1[2]) * lu +
                         v3(L->a2[0], L->a2[1], L->a2[2]) * lv;
                }
                vec = p1 - pos;
            }
            ldir = normalized(vec);
            float f = (float)3.14159;
            if (!cosb) {
                const float cos_l = __builtin_fmaxf(0.0f, dot(ldir, normal));
                const float cos_o = __builtin_fmaxf(0.0f, dot(v3(0, -1, 0), ldir * -1));
                f = cos_l * cos_o / dot(vec, vec);   // G
                i = (i > D - 2) ? i : D - 2;
            }
            C3 bw = cmulf(cmulf(m_alb, (float)(1 / 3.14159)), f);   // brdf (kernel.cu:101-104) * f
            if (!cosb) bw = cmulf(bw, fresh(a.total_light_area));
            wgt = cmul(wgt, bw);
            ro = pos;
            rd = ldir;
            ++i;
        }
        // advance to the next trace this lane needs
        for (;;) {
            if (i >= D) {
                wave_count(lcnt + 2, lane);
                SEC(SEC_SAMPLE_END);
                // cells 7 (pixel, memo) and 8 (pinhole direction) with the accumulator and mean: the
                // next sample's start needs no fetch of its own
                const uint4 c7 = R.ld4(CW_PX), c8 = R.ld4(CW_CD);
                const uint32_t px = c7.x, py = c7.y;
                // acc and the running mean: cells 4..6 = acc.r, acc.g | acc.b, m0 | m1, m2
                uint4 a01 = make_uint4(0u, 0u, 0u, 0u);
                if (!(fl & CF_ACC0)) a01 = R.ld4(CW_ACC);
                const uint4 a2m0 = R.ld4(CW_ACC + 4);   // (acc.b, only when !CF_ACC0) and m0
                const C3 acc = (fl & CF_ACC0) ? c3(0.0, 0.0, 0.0)
                                              : c3(dbl(a01.x, a01.y), dbl(a01.z, a01.w), dbl(a2m0.x, a2m0.y));
                if (!(fl & CF_SPLIT) || (fl & CF_CHUNK0)) {
                    const uint4 m12 = R.ld4(CW_M + 2);
                    const C3 m = mean_step(n, dbl(a2m0.z, a2m0.w), dbl(m12.x, m12.y), dbl(m12.z, m12.w), acc);
                    const double m0 = m.r, m1 = m.g, m2 = m.b;
                    if ((uint32_t)n >= nend) {   // (a whole pixel's unit ends at spp)
                        if (fl & CF_CHUNK0) {
                            double* P = a.lbuf + (size_t)c8.w * 3;
                            P[0] = m0; P[1] = m1; P[2] = m2;
                        } else {   // (c8.w: an accumulating whole unit's slot)
                            finish_pixel<kAccum>(a, c8.w, px, py, m0, m1, m2, rng.v0, rng.v1, rng.v2, rng.v3, rng.v4, rng.d);
                        }
                        state = ST_IDLE;
                        break;
                    }
                    R.std_(CW_M, m0); R.st4(CW_M + 2, dlo(m1), dhi(m1), dlo(m2), dhi(m2));
                } else {
                    // split pixel: keep L_n, finalize_pixels forms the ordered mean
                    // (the slot is cell 8's last word, fetched with this sample's end: no dependent fetch
                    // before the stores)
                    // (an accumulating pass: rows count from the pass's first sample)
                    double* L = a.lbuf + ((size_t)((uint32_t)(n - 1) - (kAccum ? a.acc_n0 : 0u)) * a.ntail + c8.w) * 3;
                    L[0] = acc.r;
                    L[1] = acc.g;
                    L[2] = acc.b;
                    if ((uint32_t)n >= nend) {
                        if (kAccum && nend == a.acc_n0 + (uint32_t)a.spp)   // the pixel's last sample of the pass
                            store_stream(a.npix, a.acc_rng + a.nwhole + c8.w, rng.v0, rng.v1, rng.v2, rng.v3, rng.v4, rng.d);
                        state = ST_IDLE;
                        break;
                    }
                }
                ++n;
                again = start_sample(px, py, true, c7, c8);
                break;
            }
            // Last-bounce light probe.  The hit of bounce D-1 only decides the emission it adds
            // (weight * Le if its material has emission.r != 0, kernel.cu:453); its position, normal
            // and next direction are never used, and the draws that follow do not depend on it (u,
            // then 2 or 3).  a.emis holds every triangle whose material has emission.r != 0 (the
            // integrator's own test, not the caller's light list); each is tested exactly (the
            // walk's triIntersect bits):
            //  * no hit with 0 < t < MAX_FLOAT: the reference's winner is not emissive (or there is
            //    none), so the bounce adds 0 -- the path is dead: replay its draws, no trace at all;
            //  * otherwise the winner has t <= t_min (the emitter at t_min is a triangle the reference
            //    may test; if it does not, the final winner check sends the ray to the exact slow
            //    walk), so the walk starts with its bound at t_min instead of MAX_FLOAT.
            float bound = kMaxFloat;
            const uint32_t nem = lprobe[0];   // (the emitters are staged in the block's LDS)
            // (the wave-uniform terms as one scalar test, the per-lane terms as one mask: no short circuit)
            const bool probe_on = nem != 0u && !(a.flags & PT_FLAG_NO_DEAD_PATH_SKIP) && a.scene_fast != 0u;
            if (probe_on && ((int)(i == D - 1) & (int)!czero(wgt) & (int)ray_fast_m(ro, rd)) != 0) {
                SEC(SEC_PROBE);
                float bt = kMaxFloat;
                const float4* er = reinterpret_cast<const float4*>(lprobe + 4);
                for (uint32_t k = 0; k < nem; ++k, er += 3) {
                    const float t = tri_hit_pk(f2{ro.x, ro.y}, ro.z, f2{rd.x, rd.y}, rd.z, er[0], er[1], er[2].x);
                    if (0.0f < t && t < bt) bt = t;
                }
                if (bt == kMaxFloat) wgt = c3(0.0, 0.0, 0.0);   // adds nothing: dead from here
                else bound = __uint_as_float(__float_as_uint(bt) + 1u);   // the next float above t_min
            }
            if (!(a.flags & PT_FLAG_NO_DEAD_PATH_SKIP) && czero(wgt)) {   // dead path: replay the draws
                wave_count(lcnt + 1, lane);
                SEC(SEC_DEAD);
                const float u = rng_uniform(rng);
                if (u < 0.5) { rng_next(rng); rng_next(rng); }
                else { rng_next(rng); rng_next(rng); rng_next(rng); i = (i > D - 2) ? i : D - 2; }
                ++i;
                continue;
            }
            wave_count(lcnt + 1, lane);
            again = begin_trace(ro, rd, bound);
            break;
        }
      }
      if (iters != 0u) {
          if (__ballot(again) == 0ull) break;
          continue;
      }
    // refill: lanes whose unit is finished take the next units of this shard
    uint64_t idle = __ballot(state == ST_IDLE);
    if (idle) {
        SEC(SEC_REFILL);
        const uint32_t u = take_unit<kCount>(a, lane, idle, state == ST_IDLE, lprobe, done_rel);
        if (state == ST_IDLE) {
            if (u >= a.nunits) {
                if (a.lane_times) a.lane_times[R.voff >> 4] = wall_clock64();
                state = ST_DONE;
            } else {
                // the unit as init_pixel_states prepared it (pixel, sample range, curand_init's
                // state fast-forwarded to the range, the pinhole camera ray)
                const size_t N = a.nunits;
                const uint32_t pxy = a.pix_states[UW_PXY * N + u];
                if (pxy != kNoPixel) {
                    const uint32_t px = pxy & 0xffffu, py = pxy >> 16;
                    const uint32_t n0 = a.pix_states[UW_N0 * N + u];
                    rng.v0 = a.pix_states[u];
                    rng.v1 = a.pix_states[N + u];
                    rng.v2 = a.pix_states[2 * N + u];
                    rng.v3 = a.pix_states[3 * N + u];
                    rng.v4 = a.pix_states[4 * N + u];
                    rng.d = a.pix_states[5 * N + u];
                    nend = a.pix_states[UW_NEND * N + u];
                    n = (int)(n0 & (kAccum ? kAccumMaxSamples : 0x7fffffffu));
                    // the pixel's first unit (of the pass): sample 1, or the unit word's flag
                    const bool first = kAccum ? (n0 & kUnitFirst) != 0u : n == 1;
                    const bool split = u >= a.nwhole;
                    fl = (n0 >> 31) ? CF_LENS : CF_CAMC;
                    uint4 c8 = make_uint4(0u, 0u, 0u, 0u);
                    if (!(fl & CF_LENS)) {
                        c8 = make_uint4(a.pix_states[UW_CD * N + u], a.pix_states[(UW_CD + 1) * N + u],
                                        a.pix_states[(UW_CD + 2) * N + u], a.pix_states[UW_TQ * N + u]);
                        R.st4(CW_CD, c8.x, c8.y, c8.z, c8.w);
                    }
                    if (split) fl |= first ? CF_SPLIT | CF_CHUNK0 : CF_SPLIT;
#ifdef PT_DEBUG_CHECKS
                    // finalize_pixels continues a CF_CHUNK0 slot's mean from sample chunk_first(1): the unit must end there
                    if (split && first &&
                        nend != (kAccum ? a.acc_n0 : 0u) + chunk_first(a, 1u, slot_chunks(a, a.pix_states[UW_TQ * N + u])))
                        __builtin_trap();
#endif
                    if (split && !(fl & CF_LENS) && !(a.flags & PT_FLAG_NO_PRIMARY_CACHE))
                        fl |= first ? CF_OWNER : CF_SHARE;   // (chunk 0 starts the pixel: sample 1 of a plain render)
                    R.st2(CW_PX, px, py);
                    if ((split || kAccum) && (fl & CF_LENS)) R.st(CW_Q, a.pix_states[UW_TQ * N + u]);
                    if (kAccum && (!split || first)) {
                        // the unit keeps the running mean: it continues the slot's stored one
                        const size_t P = a.npix;
                        const double* am = a.acc_mean + (split ? a.nwhole : 0u) + a.pix_states[UW_TQ * N + u];
                        const double s0 = am[0], s1 = am[P], s2 = am[2 * P];
                        R.std_(CW_M, s0); R.st4(CW_M + 2, dlo(s1), dhi(s1), dlo(s2), dhi(s2));
                    } else {
                        R.st2(CW_M, 0u, 0u); R.st4(CW_M + 2, 0u, 0u, 0u, 0u);
                    }
                    // (a new unit: no memo yet; its pinhole direction and slot are in c8 -- a lens
                    // unit reads neither, and its slot from the record)
                    again = start_sample(px, py, !(fl & CF_LENS), make_uint4(0u, 0u, 0u, 0u), c8);
                }
            }
        }
    }
      if (__ballot(again) == 0ull) break;
    }

    if (a.root_first && state == ST_TRACE && w.node == 0u) {
        bool more = walk4_root<kCount>(w, S, kCullRel, a.node_mask, cnt);
        // (up to root_first visits: the next node too while it is staged in LDS and no leaf is queued)
        for (uint32_t k = 1; more && k < a.root_first && w.node < S.ntop && !leaf4_pending(w); ++k)
            more = walk4_root<kCount>(w, S, kCullRel, a.node_mask, cnt);
        if (!more) state = (w.best_t == kMaxFloat) ? ST_SHADE : ST_SLOW;
    }
    SEC(SEC_RECORD);
    R.st4(CW_N, (uint32_t)n, (uint32_t)i, fl, rng.d);
    R.st4(CW_RNG_V0, rng.v0, rng.v1, rng.v2, rng.v3);
    R.st4(CW_WGT, dlo(wgt.r), dhi(wgt.r), dlo(wgt.g), dhi(wgt.g));
    R.st4(CW_WGT + 4, dlo(wgt.b), dhi(wgt.b), rng.v4, nend);
}


// ------------------------------------------------------------------ wavefront kernel, integrator 1
// radianceAlongSingleStep (kernel.cu:217-415) on the same state machine.  A sample is a fixed data
// flow of traces: T1 the light subpath's bounce from the area-sampled light vertex x0 (kernel.cu:263-
// 287), T2 the camera ray (the pixel's memo when the camera has no lens, :289-305), T3 the camera's
// cosine bounce (:306-350), then one visibility ray x_i -> x_j for each connection (i in {0,1}, j in
// {2,3}, :353-412) whose weight exceeds 0.01.  None of its XORWOW draws depends on a trace (lens 2,
// light pick 3, rand_ray 2, cosine 2), so all of them are drawn when the sample starts.  The record
// keeps the path vertices; the connection weights are recomputed from them in the sample's last pass,
// in the reference's order, with the visibility bits the shadow walks left (the weights' arithmetic
// is identical both times, so the set of connections that trace cannot differ).
// Cells are grouped by the pass that reads them, so that a pass touches few cells (a wave's access to
// one word of a cell spans the same 1 KiB as the whole cell): every pass reads cell 0 only, the
// sample's last pass cells 10-12.
enum : int {
    HW_N = 0, HW_SF, HW_RNG_D, HW_CU1,        // cell 0: sample, stage | flags << 16, XORWOW d, the pending
                                              //         visibility ray's length
    HW_RNG_V0 = 4,                            // cell 1: v0..v3
    HW_RNG_V4 = 8, HW_NEND, HW_DU1, HW_DU2,   // cell 2: v4, unit end, the cosine draws of T3
    HW_X0 = 12, HW_MAT0 = 15,                 // cell 3: light vertex x0 (offset along its normal), material
    HW_N0 = 16, HW_IP1 = 19,                  // cell 4: its normal, ip[1]
    HW_X1 = 20, HW_MAT1 = 23,                 // cell 5: light bounce hit x1, material
    HW_N1 = 24,                               // cell 6: its normal
    HW_X3 = 28, HW_MAT3 = 31,                 // cell 7: camera hit x3, material
    HW_N3 = 32,                               // cell 8: its normal
    HW_X2 = 36,                               // cell 9: camera bounce hit x2
    HW_GC = 40,                               // cell 10: G of the four connections (written with T3's end)
    HW_FA = 44,                               // cell 11: G1, G3, ip[1], ip[2] (T3's end)
    HW_FB = 48,                               // cell 12: the four materials (T3's end)
    HW_M = 52,                                // cells 13, 14.lo: running mean m0..m2 (f64)
    HW_PXY = 60, HW_Q, HW_MTRI, HW_MT,        // cell 15: pixel (x | y << 16), split slot, primary memo (tri, t)
    HW_CD = 64,                               // cell 16: camera direction (pinhole: the unit's; lens: the sample's)
    HW_CO = 68,                               // cell 17: camera origin of a lens sample
    kHeadWords = 72
};
// stage word: bits 0-1 the pending trace, 2-3 the connection whose visibility ray it is (k = 2i + j-2),
// 4-7 visibility bits, 8-11 the connections that need a ray
enum : uint32_t { HS_T1 = 0, HS_T2 = 1, HS_T3 = 2, HS_SH = 3 };
constexpr int kHeadLdsLightBytes = (int)kLdsLights * 16;   // per staged light: its normal and material

// The geometric factors of one HEAD sample's connections (kernel.cu:353-412): G1 = geo_term of the
// light subpath edge x1-x0, G3 = of the camera edge x3-x2, Gc[k] = the connection term of (i, j),
// k = 2i + j-2 -- the float parts of the weights, computed once from the vertices (x[4], nrm[4] as
// radianceAlongSingleStep holds them); the f64 chain (head_weights) needs only these.
struct HeadGeo {
    float G1, G3, Gc[4];
};
__device__ __forceinline__ void head_geometry(const V3 (&x)[4], const V3 (&nrm)[4], HeadGeo& g)
{
    g.G1 = geo_term(x[1], x[0], nrm[1], nrm[0]);
    g.G3 = geo_term(x[3], x[2], nrm[3], nrm[2]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 2; j < 4; ++j) {
            const V3 seg = x[j] - x[i];
            const V3 ray = normalized(seg);
            float G = __builtin_fmaxf(0.0f, dot(ray, nrm[j]) * dot(ray * -1, nrm[i])) / dot(seg, seg);
            if (G != G) G = 0;
            g.Gc[2 * i + (j - 2)] = G;
        }
    }
}
// The four connections' weights in the reference's order and arithmetic: w = le*ip0, times
// (albedo_k/pi, G, ip_k) for k = 1..i and k = j+1..3, times (albedo_j/pi, Gc, ip_j); a connection whose
// weight max exceeds 0.01 traces (its bit in *need) and counts only if visible (bit in vis); the
// radiance adds w*V and the camera hit's emission per connection.  mat[4] and ip[0..2] as the
// reference's arrays (ip[3] = 1).
__device__ __forceinline__ C3 head_weights(const Args& a, const int32_t (&mat)[4], const float (&ip)[3], const HeadGeo& g,
                                           uint32_t vis, uint32_t* need)
{
    const C3 le = mat_emission(a.mats + mat[0]);
    const C3 e3 = mat_emission(a.mats + mat[3]);
    const C3 A1 = cdivf(mat_albedo(a.mats + mat[1]), 3.14159f);
    const C3 A2 = cdivf(mat_albedo(a.mats + mat[2]), 3.14159f);
    const C3 A3 = cdivf(mat_albedo(a.mats + mat[3]), 3.14159f);
    C3 accum = c3(0, 0, 0);
    uint32_t nd = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 2; j < 4; ++j) {
            C3 w = cmulf(le, ip[0]);
            if (i == 1) w = cmulf(cmulf(cmul(w, A1), g.G1), ip[1]);      // k = 1
            if (j == 2) w = cmulf(cmulf(cmul(w, A3), g.G3), 1.0f);       // k = 3 (ip[3] = 1)
            const int k = 2 * i + (j - 2);
            w = cmulf(cmulf(cmul(w, (j == 2) ? A2 : A3), g.Gc[k]), (j == 2) ? ip[2] : 1.0f);
            const float m = (float)fmax(w.r, fmax(w.g, w.b));
            float V = 0;
            if ((double)m > 0.01) {
                nd |= 1u << k;
                if (vis & (1u << k)) V = 1;
            }
            w = cmulf(w, V);
            accum = cadd(accum, w);
            accum = cadd(accum, e3);
        }
    }
    if (need) *need = nd;
    return accum;
}

__device__ __forceinline__ V3 u3f(uint4 q) { return v3(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z)); }

// The visibility ray of connection k (kernel.cu:397-405: from x_i along normalized(x_j - x_i); visible
// iff the hit's |t - len| <= 0.01) -- the expressions of head_connections, so the same bits.
__device__ __forceinline__ void head_vis_ray(V3 xi, V3 xj, V3* ro, V3* rd, float* len)
{
    const V3 seg = xj - xi;
    *len = length(seg);
    *ro = xi;
    *rd = normalized(seg);
}
// A visibility walk only needs hits up to len + 0.01: every t >= RN(len + 0.02) has |t - len| > 0.016
// (len < MAX_FLOAT, so ulp(len) <= 2^-7), so the walk is bounded there and finding no hit below the
// bound means "not visible" -- exactly as the reference's closest hit, wherever it lies beyond, does.
__device__ __forceinline__ float head_vis_bound(float len)
{
    const float b = len + 0.02f;
    return (b < kMaxFloat) ? b : kMaxFloat;
}
// ... and any hit with t <= RN(len - 0.03) decides "not visible" at once: then len - t >= 0.026 (exact, or
// far larger), so |t - len| > 0.01 for it and for the closest hit, which is no farther (the walk stops
// there; the winner check still confirms it is a triangle the reference tests).
__device__ __forceinline__ float head_vis_occluded(float len)
{
    return (len > 0.04f) ? len - 0.03f : -1.0f;
}

// (kJit: a jittered render, as shade_lane's: instances of their own)
// (kRays: a render along the caller's rays, instances of their own too.  A unit is a pinhole unit whose camera vertex
// is the ray's origin: written to HW_CO once, when the unit is taken, beside the direction in HW_CD, and read from
// there by every sample's camera stage -- so the memo path is the pinhole unit's.)
// (kPts: an irradiance render, instances of their own as well.  A unit is a lens unit; a sample's first two draws are
// cosine_ray's over the pixel's normal, and the ray goes to HW_CO / HW_CD at once, where the camera stage reads a
// lens sample's ray.  The memo paths are compiled out.)
template <bool kCount, bool kAccum, bool kJit = false, bool kRays = false, bool kPts = false>
__device__ __forceinline__ void shade_lane_head(const ColdRec& R, int lane, uint32_t& state, V3& ro, V3& rd,
                                                int32_t& htri, float& ht, W4& w, const Stack4& S,
                                                unsigned long long* lcnt, const uint32_t* lprobe, uint32_t* done_rel,
                                                Counters& cnt)
{
    const Args& a = kernel_args_opaque();
    SEC(SEC_PASS);
    // (the XORWOW words v0..v3 are read and written only where a sample starts -- the only place a
    // sample draws -- so they are not live across the pass: the shading code then fits 96 VGPRs)
    const uint4 k0 = R.ld4(HW_N);
    if (state == ST_CHECK) {
        SEC(SEC_CHECK);
        state = check_winner(a, htri, ro, rd) ? ST_SHADE : ST_SLOW;
    }
    int n = (int)k0.x;
    uint32_t stage = k0.y & 0xffffu, fl = k0.y >> 16;
    Rng rng;
    rng.d = k0.z;
    // (likewise v4, the unit end and the cosine draws: each read where it is used, written where it
    // changes; only cell 0 -- n, stage, flags, XORWOW d -- is live across the pass)
    float cu1 = __uint_as_float(k0.w);   // the pending visibility ray's length (its check below)
    // (the staged light records and, behind them, each one's normal and material)
    const DLight* const llt = reinterpret_cast<const DLight*>(lprobe + 4 + kMaxProbeEmitters * 12);
    const float4* const lnm = reinterpret_cast<const float4*>(lprobe + 4 + kMaxProbeEmitters * 12 + kLdsLights * 12);

    // begin a trace of (ro, rd) below `bound`; true = the lane continues shading at once (no triangles, a
    // root miss -- the hit is a miss --, or a ray outside the Markstein preconditions: the exact slow walk)
    auto begin_trace = [&](float bound, float occ) -> bool {
        wave_count(lcnt + 0, lane);
        SEC(SEC_BEGIN);
        if (a.num_tris == 0) { htri = -1; ht = kMaxFloat; state = ST_SHADE; return true; }
        if (!((a.scene_fast != 0u) && ray_fast(ro, rd))) { state = ST_SLOW; return true; }
        if (!walk4_begin(w, ro, rd, a.acc_root, a.cull_abs)) { htri = -1; ht = kMaxFloat; state = ST_SHADE; return true; }
        w.best_t = bound;
        w.occ = occ;
        state = ST_TRACE;
        return false;
    };
    // start sample n: all of its draws, the light vertex, the camera ray of a lens sample; trace T1
    auto start_sample = [&](uint32_t px, uint32_t py, bool have_rng) -> bool {
        SEC(SEC_START);
        if (!have_rng) {
            const uint4 k1 = R.ld4(HW_RNG_V0);
            rng.v0 = k1.x; rng.v1 = k1.y; rng.v2 = k1.z; rng.v3 = k1.w;
            rng.v4 = R.ld(HW_RNG_V4);
        }
        const bool lens = kPts || (!kRays && (fl & CF_LENS) != 0u);
        float lu1 = 0.0f, lu2 = 0.0f;
        float jx = 0.0f, jy = 0.0f;
        bool pair = !kPts && lens;   // the sample draws a lens pair
        if (kPts) {   // this sample's ray: the pair (cosine_ray draws it) comes before every other draw
            const V3 co = ray_origin(a, px, py);
            const V3 cd = cosine_ray(ray_direction(a, px, py), rng);
            R.st4(HW_CD, __float_as_uint(cd.x), __float_as_uint(cd.y), __float_as_uint(cd.z), 0u);
            R.st4(HW_CO, __float_as_uint(co.x), __float_as_uint(co.y), __float_as_uint(co.z), 0u);
        }
        if (kJit) {   // the sample's film point: its first two draws (every unit of a jittered render has CF_LENS)
            const float ua = rng_uniform(rng), ub = rng_uniform(rng);
            jitter_offset(fresh(a.flags), ua, ub, &jx, &jy);
            pair = lens_pixel(a, px, py);
        }
        if (pair) { lu1 = rng_uniform(rng); lu2 = rng_uniform(rng); }   // drawPixel's cameraRay (kernel.cu:547)
        // light vertex: the area-CDF pick + uniform point (pick_light, kernel.cu:231-262)
        const bool staged = a.num_lights < kLdsLights;
        const DLight* const lt = staged ? llt : a.lights;
        const uint32_t sel = light_scan(lt, a.num_lights, a.total_light_area * rng_uniform(rng));
        float u = rng_uniform(rng);
        float v = rng_uniform(rng);
        const DLight* L = lt + sel;
        V3 p, n0;
        int32_t m0;
        if (L->pad != 0.0f) {   // sphere light (d8)
            p = light_point_sphere(*L, u, v);
            n0 = prim_normal(a, L->tri, p);
            m0 = prim_mat(a, L->tri);
        } else {
            if ((double)(u + v) > 1.0) {
                u = (float)((double)u + 2 * (0.5 - (double)u));
                v = (float)((double)v + 2 * (0.5 - (double)v));
            }
            p = v3(L->v0[0], L->v0[1], L->v0[2]) + v3(L->a1[0], L->a1[1], L->a1[2]) * u + v3(L->a2[0], L->a2[1], L->a2[2]) * v;
            if (staged) {
                const float4 q = lnm[sel];
                n0 = v3(q.x, q.y, q.z);
                m0 = (int32_t)__float_as_uint(q.w);
            } else {
                n0 = ld_norm(a.shade, L->tri);
                m0 = ld_mat(a.shade, L->tri);
            }
        }
        ro = p + n0 * 0.001f;                 // x[0] (kernel.cu:259)
        rd = rand_ray(n0, rng);               // the light bounce (kernel.cu:264)
        const float du1 = rng_uniform(rng);   // cosine_ray's draws for T3 (kernel.cu:307)
        const float du2 = rng_uniform(rng);
        R.st(HW_RNG_V4, rng.v4);
        R.st2(HW_DU1, __float_as_uint(du1), __float_as_uint(du2));
        R.st4(HW_RNG_V0, rng.v0, rng.v1, rng.v2, rng.v3);
        R.st4(HW_X0, __float_as_uint(ro.x), __float_as_uint(ro.y), __float_as_uint(ro.z), (uint32_t)m0);
        R.st4(HW_N0, __float_as_uint(n0.x), __float_as_uint(n0.y), __float_as_uint(n0.z), 0u);
        if (!kPts && lens) {   // this sample's camera ray (its draws came first)
            V3 co, cd;
            if (kJit) camera_ray_jitter(a, px, py, jx, jy, pair, lu1, lu2, &co, &cd);
            else if (a.oriented) camera_ray_view(a, px, py, true, lu1, lu2, &co, &cd);
            else camera_ray(a.cam, px, py, true, lu1, lu2, &co, &cd);
            R.st4(HW_CD, __float_as_uint(cd.x), __float_as_uint(cd.y), __float_as_uint(cd.z), 0u);
            R.st4(HW_CO, __float_as_uint(co.x), __float_as_uint(co.y), __float_as_uint(co.z), 0u);
        }
        stage = HS_T1;
        wave_count(lcnt + 1, lane);
        return begin_trace(kMaxFloat, -1.0f);
    };
    // T2: the camera ray -- the memo of a pinhole pixel, or a trace
    auto camera_stage = [&]() -> bool {
        stage = HS_T2;
        wave_count(lcnt + 1, lane);
        const uint4 cd = R.ld4(HW_CD);
        rd = v3(__uint_as_float(cd.x), __uint_as_float(cd.y), __uint_as_float(cd.z));
        const bool lens = kPts || (!kRays && (fl & CF_LENS) != 0u);
        if (kRays || lens) {
            const uint4 co = R.ld4(HW_CO);
            ro = v3(__uint_as_float(co.x), __uint_as_float(co.y), __uint_as_float(co.z));
        } else {
            ro = v3(0.0f, 0.0f, 0.0f) + v3(fresh(a.cam.pos[0]), fresh(a.cam.pos[1]), fresh(a.cam.pos[2]));
        }
        if (!kPts && (fl & CF_HAVE)) {
            SEC(SEC_MEMO);
            const uint2 mm = R.ld2(HW_MTRI);
            htri = (int32_t)mm.x; ht = __uint_as_float(mm.y);
            fl = (fl & ~CF_PRIMARY) | CF_MEMO; state = ST_SHADE;
            return true;
        }
        if (!kPts && (fl & CF_SHARE)) {
            const uint32_t q = R.ld(HW_Q);
            const uint64_t mv = __hip_atomic_load(reinterpret_cast<uint64_t*>(a.pmemo) + q, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
            if ((uint32_t)mv != 0u) {
                htri = (int32_t)((uint32_t)mv - 2u);
                ht = __uint_as_float((uint32_t)(mv >> 32));
                fl = (fl | CF_PRIMARY | CF_MEMO) & ~CF_SHARE;
                state = ST_SHADE;
                return true;
            }
        }
        fl = (!(a.flags & PT_FLAG_NO_PRIMARY_CACHE) && !lens) ? (fl | CF_PRIMARY) : (fl & ~CF_PRIMARY);
        return begin_trace(kMaxFloat, -1.0f);
    };
    // begin the visibility ray of connection k
    auto vis_stage = [&](uint32_t k, V3 xi, V3 xj) -> bool {
        float len;
        head_vis_ray(xi, xj, &ro, &rd, &len);
        cu1 = len;   // (stored with cell 0 at the pass's end; its walk may end in this pass: a root miss)
        stage = (stage & ~0xfu) | HS_SH | (k << 2);
        wave_count(lcnt + 1, lane);
        return begin_trace(head_vis_bound(len), head_vis_occluded(len));
    };
    auto ldv = [&](int k) -> V3 { return u3f(R.ld4(k)); };
    bool again = (state == ST_SHADE || state == ST_SLOW);
    for (uint32_t iters = 0; iters < a.wf_iters; ++iters) {
      if (again) {
        again = false;
        if (state == ST_SLOW) {
            wave_count(lcnt + 3, lane);
            SEC(SEC_SLOW);
            trace_slow(ro, rd, a.root, a.nodes, a.tris_leaf, S.spill(), S.stride, a.cull_rel, a.cull_abs,
                       &htri, &ht, kCount ? a.tri_counts : nullptr);
        }
        state = ST_SHADE;
        take_hit(a, R, HW_MTRI, HW_Q, fl, ro, rd, htri, ht);
        for (;;) {   // consume the hit; advance until the lane needs a trace or its unit is done
            SEC(SEC_BOUNCE);
            bool sample_done = false;
            C3 acc = c3(0, 0, 0);
            if ((stage & 3u) == HS_T1) {
                // light bounce hit x[1] (kernel.cu:266-287)
                int32_t tri = htri;
                float t = (float)((double)ht - 0.001);
                if (t > kMaxFloat - 1) { tri = 0; t = 0; }
                const V3 pos = ro + rd * t;
                const V3 n2 = prim_normal(a, tri, pos);
                const float G = __builtin_fabsf(dot(n2, rd)) / __builtin_fmaxf(0.001f, t * t);
                const float ip1 = (float)(2 * 3.14159 / (double)G);
                R.st4(HW_X1, __float_as_uint(pos.x), __float_as_uint(pos.y), __float_as_uint(pos.z), (uint32_t)prim_mat(a, tri));
                R.st(HW_IP1, __float_as_uint(ip1));
                R.st4(HW_N1, __float_as_uint(n2.x), __float_as_uint(n2.y), __float_as_uint(n2.z), 0u);
                if (camera_stage()) {
                    if (state == ST_SLOW) { again = true; break; }
                    take_hit(a, R, HW_MTRI, HW_Q, fl, ro, rd, htri, ht);
                    continue;   // the camera hit is at hand (memo or a root miss)
                }
                break;
            } else if ((stage & 3u) == HS_T2) {
                // camera hit x[3] (kernel.cu:289-305)
                int32_t tri = htri;
                float t = (float)((double)ht - 0.001);
                if (t > kMaxFloat - 1) { tri = 0; t = 0; }
                const V3 x3 = ro + rd * t;
                const V3 n3 = prim_normal(a, tri, x3);
                R.st4(HW_X3, __float_as_uint(x3.x), __float_as_uint(x3.y), __float_as_uint(x3.z), (uint32_t)prim_mat(a, tri));
                R.st4(HW_N3, __float_as_uint(n3.x), __float_as_uint(n3.y), __float_as_uint(n3.z), 0u);
                // the camera bounce: cosine_ray (kernel.cu:78-99) with the draws taken at the start
                SEC(SEC_COSINE);
                const uint2 cc = R.ld2(HW_DU1);
                const float du1 = __uint_as_float(cc.x), du2 = __uint_as_float(cc.y);
                const float r = sqrtf(du1);
                const float theta = (float)(2 * 3.14159 * (double)du2);
                float sn, cs;
                det_sincos(theta, &sn, &cs);
                const float y = sqrtf(__builtin_fmaxf(0.0f, 1.0f - du1));
                ro = x3;
                rd = to_frame(n3, r * cs, y, r * sn);
                stage = HS_T3;
                wave_count(lcnt + 1, lane);
                if (begin_trace(kMaxFloat, -1.0f)) {
                    if (state == ST_SLOW) { again = true; break; }
                    take_hit(a, R, HW_MTRI, HW_Q, fl, ro, rd, htri, ht);
                    continue;
                }
                break;
            } else if ((stage & 3u) == HS_T3) {
                // camera bounce hit x[2] (kernel.cu:324-350; decision d2: a miss is triangle 0, t 0)
                int32_t tri = htri;
                float t = (float)((double)ht - 0.001);
                if (t > kMaxFloat - 1 || tri < 0) { tri = 0; t = 0; }
                const uint4 c3v = R.ld4(HW_X0), c4 = R.ld4(HW_N0), c5 = R.ld4(HW_X1), c6 = R.ld4(HW_N1),
                            c7 = R.ld4(HW_X3), c8 = R.ld4(HW_N3);
                V3 x[4], nrm[4];
                x[0] = u3f(c3v); nrm[0] = u3f(c4); x[1] = u3f(c5); nrm[1] = u3f(c6); x[3] = u3f(c7); nrm[3] = u3f(c8);
                x[2] = ro + rd * t;
                nrm[2] = prim_normal(a, tri, x[2]);
                float G = __builtin_fabsf(dot(nrm[3], rd) * dot(nrm[2], rd)) / (t * t);
                if (G == 0) G = 1;
                if (G != G) G = 1;
                const int32_t mat[4] = {(int32_t)c3v.w, (int32_t)c5.w, prim_mat(a, tri), (int32_t)c7.w};
                const float ip[3] = {fresh(a.total_light_area), __uint_as_float(c4.w), (float)(3.14159 / (double)G)};
                HeadGeo g;
                head_geometry(x, nrm, g);
                R.st4(HW_X2, __float_as_uint(x[2].x), __float_as_uint(x[2].y), __float_as_uint(x[2].z), 0u);
                R.st4(HW_GC, __float_as_uint(g.Gc[0]), __float_as_uint(g.Gc[1]), __float_as_uint(g.Gc[2]), __float_as_uint(g.Gc[3]));
                R.st4(HW_FA, __float_as_uint(g.G1), __float_as_uint(g.G3), __float_as_uint(ip[1]), __float_as_uint(ip[2]));
                R.st4(HW_FB, (uint32_t)mat[0], (uint32_t)mat[1], (uint32_t)mat[2], (uint32_t)mat[3]);
                uint32_t need = 0;
                acc = head_weights(a, mat, ip, g, 0u, &need);
                if (need == 0u) {
                    sample_done = true;   // no connection needs a visibility ray: acc is the sample's radiance
                } else {
                    stage = (need << 8);
                    const uint32_t k = (uint32_t)__builtin_ctz(need);
                    // (the endpoints re-read from the record: the vertices need not stay live across the weights)
                    asm volatile("" ::: "memory");
                    if (vis_stage(k, ldv((k >> 1) ? HW_X1 : HW_X0), ldv((k & 1u) ? HW_X3 : HW_X2))) {
                        if (state == ST_SLOW) { again = true; break; }
                        take_hit(a, R, HW_MTRI, HW_Q, fl, ro, rd, htri, ht);
                        continue;
                    }
                    break;
                }
            } else {
                // visibility ray of connection k (kernel.cu:397-405)
                const uint32_t k = (stage >> 2) & 3u, need = (stage >> 8) & 15u;
                if ((double)__builtin_fabsf(ht - cu1) <= 0.01) stage |= 1u << (4 + k);
                const uint32_t rest = need & ~((2u << k) - 1u);
                if (rest != 0u) {
                    const uint32_t k2 = (uint32_t)__builtin_ctz(rest);
                    const V3 xi = ldv((k2 >> 1) ? HW_X1 : HW_X0), xj = ldv((k2 & 1u) ? HW_X3 : HW_X2);
                    if (vis_stage(k2, xi, xj)) {
                        if (state == ST_SLOW) { again = true; break; }
                        take_hit(a, R, HW_MTRI, HW_Q, fl, ro, rd, htri, ht);
                        continue;
                    }
                    break;
                }
                // the sample's last pass: the weights again, now with the visibility bits
                HeadGeo g;
                const uint4 gc = R.ld4(HW_GC), fa = R.ld4(HW_FA), fb = R.ld4(HW_FB);

                g.Gc[0] = __uint_as_float(gc.x); g.Gc[1] = __uint_as_float(gc.y); g.Gc[2] = __uint_as_float(gc.z);
                g.Gc[3] = __uint_as_float(gc.w);
                g.G1 = __uint_as_float(fa.x);
                g.G3 = __uint_as_float(fa.y);
                const int32_t mat[4] = {(int32_t)fb.x, (int32_t)fb.y, (int32_t)fb.z, (int32_t)fb.w};
                const float ip[3] = {fresh(a.total_light_area), __uint_as_float(fa.z), __uint_as_float(fa.w)};
                acc = head_weights(a, mat, ip, g, (stage >> 4) & 15u, nullptr);
                sample_done = true;
            }
            if (!sample_done) break;
            // sample n's end: the running mean (kernel.cu:551-552), or the split pixel's per-sample slot
            wave_count(lcnt + 2, lane);
            SEC(SEC_SAMPLE_END);
            const uint4 c13 = R.ld4(HW_PXY);
            // the next sample's XORWOW words and the unit end, fetched with the sample's end
            const uint4 r1 = R.ld4(HW_RNG_V0), r2 = R.ld4(HW_RNG_V4);
            const uint32_t px = c13.x & 0xffffu, py = c13.x >> 16;
            if (!(fl & CF_SPLIT)) {
                const uint4 m01 = R.ld4(HW_M);
                const uint2 m2 = R.ld2(HW_M + 4);
                const C3 m = mean_step(n, dbl(m01.x, m01.y), dbl(m01.z, m01.w), dbl(m2.x, m2.y), acc);
                const double m0 = m.r, mm1 = m.g, mm2 = m.b;
                if (kAccum ? (uint32_t)n >= r2.y : n >= a.spp) {   // (the unit's end: a plain whole pixel's is spp)
                    // (c13.y: an accumulating whole unit's slot)
                    finish_pixel<kAccum>(a, c13.y, px, py, m0, mm1, mm2, r1.x, r1.y, r1.z, r1.w, r2.x, rng.d);
                    state = ST_IDLE;
                    break;
                }
                R.st4(HW_M, dlo(m0), dhi(m0), dlo(mm1), dhi(mm1));
                R.st2(HW_M + 4, dlo(mm2), dhi(mm2));
            } else {
                // (an accumulating pass: rows count from the pass's first sample)
                double* Lb = a.lbuf + ((size_t)((uint32_t)(n - 1) - (kAccum ? a.acc_n0 : 0u)) * a.ntail + c13.y) * 3;
                Lb[0] = acc.r;
                Lb[1] = acc.g;
                Lb[2] = acc.b;
                if ((uint32_t)n >= r2.y) {
                    if (kAccum && r2.y == a.acc_n0 + (uint32_t)a.spp)   // the pixel's last sample of the pass
                        store_stream(a.npix, a.acc_rng + a.nwhole + c13.y, r1.x, r1.y, r1.z, r1.w, r2.x, rng.d);
                    state = ST_IDLE;
                    break;
                }
            }
            ++n;
            rng.v0 = r1.x; rng.v1 = r1.y; rng.v2 = r1.z; rng.v3 = r1.w; rng.v4 = r2.x;
            again = start_sample(px, py, true);
            break;
        }
      }
      if (iters != 0u) {
          if (__ballot(again) == 0ull) break;
          continue;
      }
      // refill: lanes whose unit is finished take the next units of this shard
      uint64_t idle = __ballot(state == ST_IDLE);
      if (idle) {
          SEC(SEC_REFILL);
          const uint32_t u = take_unit<kCount>(a, lane, idle, state == ST_IDLE, lprobe, done_rel);
          if (state == ST_IDLE) {
              if (u >= a.nunits) {
                  if (a.lane_times) a.lane_times[R.voff >> 4] = wall_clock64();
                  state = ST_DONE;
              } else {
                  const size_t N = a.nunits;
                  const uint32_t pxy = a.pix_states[UW_PXY * N + u];
                  if (pxy != kNoPixel) {
                      const uint32_t n0 = a.pix_states[UW_N0 * N + u];
                      rng.v0 = a.pix_states[u];
                      rng.v1 = a.pix_states[N + u];
                      rng.v2 = a.pix_states[2 * N + u];
                      rng.v3 = a.pix_states[3 * N + u];
                      rng.v4 = a.pix_states[4 * N + u];
                      rng.d = a.pix_states[5 * N + u];
                      R.st(HW_NEND, a.pix_states[UW_NEND * N + u]);
                      n = (int)(n0 & (kAccum ? kAccumMaxSamples : 0x7fffffffu));
                      const bool first = kAccum ? (n0 & kUnitFirst) != 0u : n == 1;   // the pixel's first unit (of the pass)
                      const bool split = u >= a.nwhole;
                      fl = (n0 >> 31) ? CF_LENS : CF_CAMC;
                      if (!(fl & CF_LENS))
                          R.st4(HW_CD, a.pix_states[UW_CD * N + u], a.pix_states[(UW_CD + 1) * N + u],
                                a.pix_states[(UW_CD + 2) * N + u], 0u);
                      if (kRays) {   // the unit's camera vertex: the ray's origin, once
                          const V3 co = ray_origin(a, pxy & 0xffffu, pxy >> 16);
                          R.st4(HW_CO, __float_as_uint(co.x), __float_as_uint(co.y), __float_as_uint(co.z), 0u);
                      }
                      if (split) fl |= CF_SPLIT;
                      if (split && !(fl & CF_LENS) && !(a.flags & PT_FLAG_NO_PRIMARY_CACHE))
                          fl |= first ? CF_OWNER : CF_SHARE;
                      R.st4(HW_PXY, pxy, (split || kAccum) ? a.pix_states[UW_TQ * N + u] : 0u, 0u, 0u);
                      if (kAccum && !split) {   // a whole pixel continues its slot's stored mean
                          const size_t P = a.npix;
                          const double* am = a.acc_mean + a.pix_states[UW_TQ * N + u];
                          const double s0 = am[0], s1 = am[P], s2 = am[2 * P];
                          R.st4(HW_M, dlo(s0), dhi(s0), dlo(s1), dhi(s1)); R.st2(HW_M + 4, dlo(s2), dhi(s2));
                      } else {
                          R.st4(HW_M, 0u, 0u, 0u, 0u); R.st2(HW_M + 4, 0u, 0u);
                      }
                      again = start_sample(pxy & 0xffffu, pxy >> 16, true);
                  }
              }
          }
      }
      if (__ballot(again) == 0ull) break;
    }
    if (a.root_first && state == ST_TRACE && w.node == 0u) {
        bool more = walk4_root<kCount>(w, S, kCullRel, a.node_mask, cnt);
        for (uint32_t k = 1; more && k < a.root_first && w.node < S.ntop && !leaf4_pending(w); ++k)
            more = walk4_root<kCount>(w, S, kCullRel, a.node_mask, cnt);
        if (!more) {   // nothing below the bound: a miss
            w.best_t = kMaxFloat;
            state = ST_SHADE;
        }
    }
    SEC(SEC_RECORD);
    R.st4(HW_N, (uint32_t)n, stage | (fl << 16), rng.d, __float_as_uint(cu1));
}

// The wavefront kernel's body, shared by both integrators (kHead: integrator 1, shade_lane_head).
// kLdsWalk: walk steps read the staged top from LDS (integrator 1 always; integrator 0 when the LDS
// top holds the whole tree) instead of issuing every node's loads to memory.
template <bool kCount, bool kHead, bool kLdsWalk = kHead, bool kAccum = false, bool kView = false, bool kJit = false,
          bool kRays = false, bool kPts = false>
__device__ __forceinline__ void wf_main(const Args& a)
{
    extern __shared__ uint32_t lds_wf[];
    // after the four waves' rings (kWaveLdsWords each): the block counters (traced, reference,
    // samples, slow walks)
    unsigned long long* lcnt = reinterpret_cast<unsigned long long*>(lds_wf + 4 * kWaveLdsWords);
    // 4 counters + the section counts + the walk-length histogram (counting variant)
    if (threadIdx.x < 4 + kSections / 2 + kHist / 2) lcnt[threadIdx.x] = 0ull;
    uint32_t* const lhist = reinterpret_cast<uint32_t*>(lcnt + 4) + kSections;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    Counters cnt;
    if (kCount) cnt.tri_counts = a.tri_counts;
    if (kCount && threadIdx.x == 0) atomicMin(a.counters + CNT_T_START, (unsigned long long)wall_clock64());   // first start
    uint32_t walk_slots = 0, shade_slots = 0;   // counting variant: SIMD lane-slot usage
    uint32_t trace_slots = 0, steps = 0;        // counting variant: lanes tracing per iteration; steps of this walk
    uint32_t start_wait = 0;                    // counting variant: lanes without a ray when a walk phase starts
    uint32_t itc[6] = {0, 0, 0, 0, 0, 0};       // counting variant: walk-iteration classes (counters[14..19])
    unsigned long long walk_clk = 0, shade_clk = 0;   // counting variant: wave-clock per phase
    uint32_t done_rel[2] = {0, 0};                    // counting variant: ticks from the queue's drain / the
                                                      // kernel's start to this lane's end

    // hot state: what the walk phase needs
    uint32_t state = ST_IDLE;
    V3 ro = v3(0, 0, 0), rd = v3(0, 0, 1);
    W4 w;
    int32_t& htri = reinterpret_cast<int32_t&>(w.best_slot);   // the pending hit lives in the walk state
    float& ht = w.best_t;                                        // (a finished walk leaves it there)
    htri = -1;
    ht = kMaxFloat;
    Stack4 S;
    S.ring = lds_wf + (threadIdx.x >> 6) * kWaveLdsWords + lane;
    S.stride = a.spill_stride;
    constexpr uint32_t kRecWords = kHead ? (uint32_t)kHeadWords : (uint32_t)kColdWords;
    const ColdRec R{__builtin_amdgcn_make_buffer_rsrc(a.cold, 0, (int)(kRecWords * a.cold_stride * 4u), 0x00020000),
                    (uint32_t)(blockIdx.x * blockDim.x + threadIdx.x) * 16u, a.cold_stride * 16u};
    S.spill_base = a.spill;   // spill column of lane g at byte offset 4g = R.voff / 4
    S.lane_off = &R.voff;
    S.off_mask = ~0u;
    S.off_shift = 2;
    // the light probe's emitters (count, then records), then the top of the BVH4 (kTopNodeBytes per node)
    uint32_t* const lprobe = reinterpret_cast<uint32_t*>(lcnt + 4 + (kSections + kHist) / 2);
    if (threadIdx.x == 0) { lprobe[0] = a.num_emis; lprobe[1] = 0u; }   // ([1]: the refill's exhausted unit counters)
    if (a.num_lights < kLdsLights)
        for (uint32_t k = threadIdx.x; k < (a.num_lights + 1) * 3; k += blockDim.x)
            reinterpret_cast<float4*>(lprobe + 4 + kMaxProbeEmitters * 12)[k] = reinterpret_cast<const float4*>(a.lights)[k];
    for (uint32_t k = threadIdx.x; k < a.num_emis * 3; k += blockDim.x)
        reinterpret_cast<float4*>(lprobe + 4)[k] = reinterpret_cast<const float4*>(a.emis)[k];
    if (kHead && a.num_lights < kLdsLights) {   // integrator 1: each staged light's normal and material
        float4* const lnm = reinterpret_cast<float4*>(lprobe + 4 + kMaxProbeEmitters * 12 + kLdsLights * 12);
        for (uint32_t k = threadIdx.x; k <= a.num_lights; k += blockDim.x) {
            const DLight& L = a.lights[k];
            float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (L.pad == 0.0f) {
                const DShade& sh = a.shade[L.tri];
                q = make_float4(sh.nx, sh.ny, sh.nz, __uint_as_float((uint32_t)sh.mat));
            }
            lnm[k] = q;
        }
    }
    float4* const ltop = reinterpret_cast<float4*>(reinterpret_cast<char*>(lprobe) + kProbeLdsBytes +
                                                   (kHead ? kHeadLdsLightBytes : 0));
    for (uint32_t k = threadIdx.x; k < a.top_nodes * (kTopNodeBytes / 16); k += blockDim.x) {
        const uint32_t nd = k / (kTopNodeBytes / 16), q = k - nd * (kTopNodeBytes / 16);
        ltop[k] = reinterpret_cast<const float4*>(a.nodes4 + nd)[q];
    }
    S.top = reinterpret_cast<const char*>(ltop);
    S.ntop = a.top_nodes;
    __syncthreads();
    const uint32_t nlanes = gridDim.x * blockDim.x, wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (a.lane_times && lane == 0) a.lane_times[nlanes + wave_id] = wall_clock64();

    for (;;) {
        // ---------------------------------------------------------------- walk
        // walk phases issue ahead of other waves' shading passes (wave priority 1 vs 0): a walk
        // step's node fetch goes out sooner, so more of its round trip overlaps the shading VALU
        // (C3 +2.7%, 1/8 shard +1.0%, same box; priorities 2 and 3 the same, shading first -0.7%)
        __builtin_amdgcn_s_setprio(1);
        unsigned long long clk0 = 0;
        if (kCount) clk0 = clock64();
        const uint64_t live = __ballot(state != ST_DONE);   // (no lane becomes DONE while walking)
        if (kCount) start_wait += (uint32_t)__popcll(live & ~__ballot(state == ST_TRACE));
        // (the threshold as an opaque scalar: left a kernel argument, it was reloaded and waited for at
        // the head of every step)
        uint32_t thr;
        asm volatile("s_mov_b32 %0, %1" : "=s"(thr) : "s"(a.wf_threshold));
        for (;;) {
            const uint64_t tracing = __ballot(state == ST_TRACE);
            if (tracing == 0ull) break;
            if ((uint32_t)__popcll(live & ~tracing) >= thr) break;   // lanes waiting to shade
            if (kCount) {
                ++walk_slots;
                if (state == ST_TRACE) ++trace_slots;
                // wave iterations by the number of lanes needing a global node fetch (0, 1-4, 5-8,
                // more), with no pending leaf in the wave, and with neither
                const bool vis = state == ST_TRACE && w.node != kNone && w.lsp <= kLeafRing - 1;
                const uint32_t deep = (uint32_t)__popcll(__ballot(vis && w.node >= S.ntop));
                const bool noleaf = __ballot(state == ST_TRACE && leaf4_pending(w)) == 0ull;
                ++itc[deep == 0u ? 0 : deep <= 4u ? 1 : deep <= 8u ? 2 : 3];
                if (noleaf) ++itc[4];
                if (noleaf && deep == 0u) ++itc[5];
            }
            if (state == ST_TRACE) {
                // (the culling factor as the literal it always is: a kernel argument here was a scalar
                // load and wait on every step's chain, the compiler rematerialising it for want of SGPRs)
                const bool more = walk4_step<kCount, true, NoSetup, kHead, !kLdsWalk>(
                    w, ro, rd, a.nodes4, a.acc_tris, S, kCullRel, a.cull_abs, a.node_mask, cnt);
                if (kCount) ++steps;
                if (kCount && !more) {   // walk length histogram, log2 buckets
                    atomicAdd(lhist + min(31 - __clz((int)steps), kHist - 1), 1u);
                    steps = 0;
                }
                if (!more) state = ST_WALKED;
            }
        }
        __builtin_amdgcn_s_setprio(0);
        // the winner's check against the reference BVH runs in the shading phase
        // (htri, ht) == (w.best_slot, w.best_t): the hit is already in place
        // (no winner: a miss -- or, for a bounded last-bounce walk, never expected: exact slow walk)
        if (state == ST_WALKED) {
            if (kHead) {   // integrator 1: no hit below the bound is a miss (a visibility walk's "not visible")
                if (w.best_slot != kNone) state = ST_CHECK;
                else { w.best_t = kMaxFloat; state = ST_SHADE; }
            } else {
                state = (w.best_slot != kNone) ? ST_CHECK : (w.best_t == kMaxFloat) ? ST_SHADE : ST_SLOW;
            }
        }

        if (kCount) {
            const unsigned long long c = clock64();
            walk_clk += c - clk0;
            clk0 = c;
        }
        // ---------------------------------------------------------------- shade + refill
        // Only the per-bounce part of the shading state is held in registers here (sample
        // index, bounce, flags, RNG, path weight); accumulator, running mean, pixel and memo
        // words are read and written in the record where they are used.
        if (kCount) ++shade_slots;
        // (the lane id is recomputed for the shading pass: one VGPR less live across the walk loop)
        if (state != ST_TRACE && state != ST_DONE) {
            if (kHead) shade_lane_head<kCount, kAccum, kJit, kRays, kPts>(R, (int)__lane_id(), state, ro, rd, htri, ht, w, S, lcnt, lprobe, done_rel, cnt);
            else shade_lane<kCount, kAccum, kView, kJit, kRays, kPts>(a, R, (int)__lane_id(), state, ro, rd, htri, ht, w, S, lcnt, lprobe, done_rel, cnt);
        }
        if (kCount) shade_clk += clock64() - clk0;
        if (__ballot(state != ST_DONE) == 0ull) break;
    }
    if (a.lane_times && lane == 0) a.lane_times[nlanes + nlanes / 64 + wave_id] = wall_clock64();
    if (kCount) {
        if (lane == 0) { atomicAdd(a.counters + CNT_WALK_CYCLES, walk_clk); atomicAdd(a.counters + CNT_SHADE_CYCLES, shade_clk); }
        if (lane == 0) {   // wave exit times (wall clock): last, the sum for the mean, and after the drain
            const unsigned long long t = wall_clock64();
            atomicMax(a.counters + CNT_T_LAST_EXIT, t);
            atomicAdd(a.counters + CNT_T_EXIT_SUM, t);
            atomicAdd(a.counters + CNT_WAVES, 1ull);
            const unsigned long long d0 = __hip_atomic_load(a.counters + CNT_T_DRAINED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicAdd(a.counters + CNT_WAVE_BINS + tail_bin(t - min(t, d0)), 1ull);
        }
        // lane ends after the drain (log2 bins: one atomic per occupied bin and wave), and their sum
        // since the kernel's start (the tail's idle lane-time = lanes x last exit - that sum)
        const uint32_t bin = tail_bin(done_rel[0]);
        for (uint32_t k = 0; k < (uint32_t)kTailBins; ++k) {
            const uint64_t m = __ballot(bin == k);
            if (m && lane == 0) atomicAdd(a.counters + CNT_LANE_BINS + k, (unsigned long long)__popcll(m));
        }
        const unsigned long long dsum = wave_sum(done_rel[1]);
        if (lane == 0) atomicAdd(a.counters + CNT_LANE_END_SUM, dsum);
        const unsigned long long c2 = wave_sum(cnt.nodes), c3v = wave_sum(cnt.tris), c5 = wave_sum(walk_slots);
        const unsigned long long c13 = wave_sum(cnt.top), c25 = wave_sum(cnt.spills);
        const unsigned long long c6 = wave_sum(cnt.leaf_steps), c7 = wave_sum(shade_slots);
        const unsigned long long c11 = wave_sum(trace_slots);
        if (lane == 0) {
            atomicAdd(a.counters + CNT_NODES, c2); atomicAdd(a.counters + CNT_TRIS, c3v); atomicAdd(a.counters + CNT_WALK_SLOTS, c5);
            atomicAdd(a.counters + CNT_LEAF_STEPS, c6); atomicAdd(a.counters + CNT_SHADE_SLOTS, c7); atomicAdd(a.counters + CNT_TRACE_SLOTS, c11);
            atomicAdd(a.counters + CNT_START_WAIT, (unsigned long long)start_wait);
            atomicAdd(a.counters + CNT_TOP_VISITS, c13);
            atomicAdd(a.counters + CNT_SPILL, c25);
            for (int k = 0; k < 6; ++k) atomicAdd(a.counters + CNT_ITERS + k, (unsigned long long)itc[k]);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // (lcnt is the block's own LDS table -- 0 traced, 1 reference, 2 samples, 3 fallbacks, as shade_lane's
        // wave_count(lcnt + k) fills it -- not Args::counters: its indices are not CNT_*)
        atomicAdd(a.counters + CNT_TRACED, lcnt[0]);
        atomicAdd(a.counters + CNT_REFERENCE, lcnt[1]);
        atomicAdd(a.counters + CNT_SAMPLES, lcnt[2]);
        if (lcnt[3]) atomicAdd(a.counters + CNT_FALLBACKS, lcnt[3]);
    }
    if (kCount && threadIdx.x < kSections + kHist) {   // section counts, then the histogram
        const uint32_t v = reinterpret_cast<const uint32_t*>(lcnt + 4)[threadIdx.x];
        if (v) atomicAdd(a.counters + CNT_SECTIONS + threadIdx.x, (unsigned long long)v);
    }
}

template <bool kCount, int kMinWaves, bool kLdsWalk = false>
__global__ __launch_bounds__(256, kMinWaves) void render_unidir_wf(Args a)
{
    wf_main<kCount, false, kLdsWalk>(a);
}

// integrator 1 (radianceAlongSingleStep, kernel.cu:217-415) on the wavefront state machine
template <bool kCount, int kMinWaves>
__global__ __launch_bounds__(256, kMinWaves) void render_head_wf(Args a)
{
    wf_main<kCount, true>(a);
}

// The accumulating instances (pt_accum_add; kAccum): default occupancy, no counting -- kernels of their own
// names, so the plain kernels keep theirs (profiles and tools refer to them).
template <bool kLdsWalk>
__global__ __launch_bounds__(256, 5) void render_unidir_accum_wf(Args a)
{
    wf_main<false, false, kLdsWalk, true>(a);
}
__global__ __launch_bounds__(256, 5) void render_head_accum_wf(Args a)
{
    wf_main<false, true, true, true>(a);
}

// Integrator 0 through an oriented camera (Args::oriented; kView): twins of render_unidir_wf and
// render_unidir_accum_wf, after them, so that a render without a view runs the kernels it always ran.  (Integrator
// 1's kernels take the view under a uniform branch: their register budget did not move)
template <bool kCount, int kMinWaves, bool kLdsWalk = false>
__global__ __launch_bounds__(256, kMinWaves) void render_unidir_view_wf(Args a)
{
    wf_main<kCount, false, kLdsWalk, false, true>(a);
}
template <bool kLdsWalk>
__global__ __launch_bounds__(256, 5) void render_unidir_accum_view_wf(Args a)
{
    wf_main<false, false, kLdsWalk, true, true>(a);
}

// ------------------------------------------------------------------ output step
// kernel.cu:763-778 / color.h:59-71 on the GPU: code = (int)(pow(c/(c+1), (float)(1/2.2))*255)
// per channel, read off a table of the 255 boundaries the HOST's libm puts between codes
// (pt::tonemap_thresholds), so the codes equal pt_tonemap_u8 exactly.
__global__ __launch_bounds__(256) void tonemap_codes(const float* __restrict__ rgb, size_t n,
                                                     const float* __restrict__ thr, int32_t* __restrict__ out)
{
    __shared__ float t[256];
    t[threadIdx.x] = thr[threadIdx.x];
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float c = rgb[i];
        int32_t code;
        if (!(c == c) || c == INFINITY) {
            code = INT32_MIN;                // c/(c+1) is NaN: (int)NaN on x86
        } else if (c < 0.0f) {
            code = INT32_MAX;                // never produced by the integrator; redone on the host
        } else {
            int lo = 0, hi = 255;            // largest k with t[k] <= c (t[0] = 0)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (t[mid] <= c) lo = mid; else hi = mid - 1;
            }
            code = lo;
        }
        out[i] = code;
    }
}

// ------------------------------------------------------------------ batched trace()
// pt_trace: the reference's trace() (kernel.cu:112-161) for a batch of rays, one lane per ray,
// on the same walk the wavefront kernel uses (BVH4 + winner check + exact slow path), or on the
// reference BVH with the reference's own stack walk (kRef).  A caller's rays need not be the
// integrator's: those outside ray_regular() take the reference's walk too (pt_device.h).
template <bool kRef, bool kCount>
__global__ __launch_bounds__(256) void trace_rays(Args a, const float* __restrict__ rays, uint32_t n,
                                                  int32_t* __restrict__ tri_out, float* __restrict__ t_out)
{
    extern __shared__ uint32_t lds_tr[];
    const int lane = threadIdx.x & 63;
    Counters cnt;
    if (kCount) cnt.tri_counts = a.tri_counts;
    Stack4 S;
    // per wave: the reference walk's stack (stack_words) or the BVH4 rings (kWaveLdsWords)
    uint32_t* const wave_lds = lds_tr + (threadIdx.x >> 6) * a.stack_words;
    S.ring = wave_lds + lane;
    S.stride = a.spill_stride;
    const uint32_t lane_off = (blockIdx.x * blockDim.x + threadIdx.x) * 4u;
    S.spill_base = a.spill;
    S.lane_off = &lane_off;
    S.off_mask = ~0u;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const V3 o = v3(rays[6 * r], rays[6 * r + 1], rays[6 * r + 2]);
        const V3 d = v3(rays[6 * r + 3], rays[6 * r + 4], rays[6 * r + 5]);
        int32_t htri = -1;
        float ht = kMaxFloat;
        if (a.num_tris == 0) {
            // spheres only
        } else if (kRef) {
            const Hit h = trace_reference<kCount>(o, d, a.rnodes, a.tris_orig, wave_lds, lane, cnt);
            htri = h.tri; ht = h.t;
        } else if (!ray_regular(o, d, a.origin_max)) {
            // a far origin or a long direction: the reference's walk, its stack in this lane's spill column
            atomicAdd(a.counters + CNT_FALLBACKS, 1ull);
            const Hit h = trace_reference<kCount>(o, d, a.rnodes, a.tris_orig, S.spill(), 0, cnt, (int)S.stride);
            htri = h.tri; ht = h.t;
        } else if (!((a.scene_fast != 0u) && ray_fast(o, d))) {
            atomicAdd(a.counters + CNT_FALLBACKS, 1ull);
            trace_slow(o, d, a.root, a.nodes, a.tris_leaf, S.spill(), S.stride, a.cull_rel, a.cull_abs, &htri, &ht,
                       cnt.tri_counts);
        } else {
            W4 w;
            if (walk4_begin(w, o, d, a.acc_root, a.cull_abs)) {
                while (walk4_step<kCount>(w, o, d, a.nodes4, a.acc_tris, S, a.cull_rel, a.cull_abs, a.node_mask, cnt)) {
                }
                ht = w.best_t;
                bool ok = true;
                if (w.best_slot != kNone) {
                    const float4 C = a.acc_tris[w.best_slot].c;
                    htri = (int32_t)__float_as_uint(C.y);
                    ok = ref_tested(__float_as_uint(C.w), o, d, a.rnodes, a.rparent);
                }
                if (!ok) {
                    atomicAdd(a.counters + CNT_FALLBACKS, 1ull);
                    trace_slow(o, d, a.root, a.nodes, a.tris_leaf, S.spill(), S.stride, a.cull_rel, a.cull_abs,
                               &htri, &ht, cnt.tri_counts);
                }
            }
        }
        if (a.num_spheres) apply_spheres(a, o, d, &htri, &ht);
        tri_out[r] = htri;
        t_out[r] = ht;
    }
    if (kCount) {
        const unsigned long long sp = wave_sum(cnt.spills);
        if (lane == 0 && sp) atomicAdd(a.counters + CNT_SPILL, sp);
    }
}

// ------------------------------------------------------------------ primary-hit features
// pt_render_features: the camera ray of every pixel of the shard (pinhole: no lens draws), traced as
// trace_rays<false, false> traces a ray, then the hit's material and normal as one 48-B pt_feature.
// One lane per work slot, in the wavefront kernels' slot order (unit_pixel: a wave = one 8x8 block, so
// its rays are coherent); slots outside the image write nothing.
// (kView: the oriented pinhole ray; primary_features_view is the kernel of a render with a view)
// (kJit: the guide buffers of a jittered render, primary_features_jitter: the ray through the footprint's centre,
// jx = jy = 0.5, box and tent alike, so that they sit under the image they guide)
// (kRays: the guide buffers of a ray render, primary_features_rays: the pixel's ray as it stands in RayArgs::rays -- no
// normalisation, no 0 + o -- so depth is closestT along the given d and an irregular ray takes the reference's walk)
template <bool kView, bool kJit = false, bool kRays = false>
__device__ __forceinline__ void primary_features_body(const Args& a, float4* __restrict__ out)
{
    extern __shared__ uint32_t lds_tr[];
    const int lane = threadIdx.x & 63;
    Counters cnt;
    Stack4 S;
    uint32_t* const wave_lds = lds_tr + (threadIdx.x >> 6) * a.stack_words;
    S.ring = wave_lds + lane;
    S.stride = a.spill_stride;
    const uint32_t lane_off = (blockIdx.x * blockDim.x + threadIdx.x) * 4u;
    S.spill_base = a.spill;
    S.lane_off = &lane_off;
    S.off_mask = ~0u;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < a.npix; q += gridDim.x * blockDim.x) {
        uint32_t px, py;
        if (!unit_pixel(a, q, &px, &py)) continue;
        V3 o, d;
        if (kRays) { o = ray_origin(a, px, py); d = ray_direction(a, px, py); }
        else if (kJit) camera_ray_jitter<false>(a, px, py, 0.5f, 0.5f, false, 0.0f, 0.0f, &o, &d);
        else if (kView) camera_ray_view<false>(a, px, py, false, 0.0f, 0.0f, &o, &d);
        else camera_ray<false>(a.cam, px, py, false, 0.0f, 0.0f, &o, &d);
        int32_t htri = -1;
        float ht = kMaxFloat;
        if (a.num_tris == 0) {
            // spheres only
        } else if (!ray_regular(o, d, a.origin_max)) {   // (a far camera, as trace_rays<false, *> traces its rays)
            const Hit h = trace_reference<false>(o, d, a.rnodes, a.tris_orig, S.spill(), 0, cnt, (int)S.stride);
            htri = h.tri; ht = h.t;
        } else if (!((a.scene_fast != 0u) && ray_fast(o, d))) {
            trace_slow(o, d, a.root, a.nodes, a.tris_leaf, S.spill(), S.stride, a.cull_rel, a.cull_abs, &htri, &ht,
                       cnt.tri_counts);
        } else {
            W4 w;
            if (walk4_begin(w, o, d, a.acc_root, a.cull_abs)) {
                while (walk4_step<false>(w, o, d, a.nodes4, a.acc_tris, S, a.cull_rel, a.cull_abs, a.node_mask, cnt)) {
                }
                ht = w.best_t;
                bool ok = true;
                if (w.best_slot != kNone) {
                    const float4 C = a.acc_tris[w.best_slot].c;
                    htri = (int32_t)__float_as_uint(C.y);
                    ok = ref_tested(__float_as_uint(C.w), o, d, a.rnodes, a.rparent);
                }
                if (!ok)
                    trace_slow(o, d, a.root, a.nodes, a.tris_leaf, S.spill(), S.stride, a.cull_rel, a.cull_abs,
                               &htri, &ht, cnt.tri_counts);
            }
        }
        if (a.num_spheres) apply_spheres(a, o, d, &htri, &ht);
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, ht);                       // albedo, depth
        float4 r1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));       // normal, prim
        float4 r2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                     // position, reserved
        if (htri >= 0) {
            const V3 p = o + d * ht;
            const V3 n = prim_normal(a, htri, p);
            const DMat* m = a.mats + prim_mat(a, htri);
            const int32_t prim = htri | ((m->emission[0] != 0.0) ? (int32_t)PT_FEATURE_EMISSIVE : 0);
            r0 = make_float4((float)m->albedo[0], (float)m->albedo[1], (float)m->albedo[2], ht);
            r1 = make_float4(n.x, n.y, n.z, __int_as_float(prim));
            r2 = make_float4(p.x, p.y, p.z, 0.0f);
        }
        float4* rec = out + out_pixel(a, px, py) * 3;
        rec[0] = r0; rec[1] = r1; rec[2] = r2;
    }
}
__global__ __launch_bounds__(256) void primary_features(Args a, float4* __restrict__ out)
{
    primary_features_body<false>(a, out);
}
__global__ __launch_bounds__(256) void primary_features_view(Args a, float4* __restrict__ out)
{
    primary_features_body<true>(a, out);
}

// ------------------------------------------------------------------ sub-pixel jitter (PT_FLAG_JITTER)
// The kernels of a jittered render: twins of the set-up kernels, of every wavefront instance of both integrators and
// of the features kernel (render_tiles_jitter stands with render_tiles), defined and first used after every existing
// instance, so that a render without the flag runs the kernels it always ran, compiled as they always were
// (DESIGN.md 3.15).  One set serves both cameras: the view is a wave-uniform branch inside them.
__global__ __launch_bounds__(256) void init_pixel_states_jitter(Args a, uint32_t* __restrict__ st)
{
    init_pixel_states_body<true>(a, st);
}
__global__ __launch_bounds__(256) void init_active_states_jitter(Args a, uint32_t* __restrict__ st, const uint32_t* __restrict__ list)
{
    init_active_states_body<true>(a, st, list);
}
template <bool kCount, int kMinWaves, bool kLdsWalk = false>
__global__ __launch_bounds__(256, kMinWaves) void render_unidir_jitter_wf(Args a)
{
    wf_main<kCount, false, kLdsWalk, false, false, true>(a);
}
template <bool kLdsWalk>
__global__ __launch_bounds__(256, 5) void render_unidir_accum_jitter_wf(Args a)
{
    wf_main<false, false, kLdsWalk, true, false, true>(a);
}
template <bool kCount, int kMinWaves>
__global__ __launch_bounds__(256, kMinWaves) void render_head_jitter_wf(Args a)
{
    wf_main<kCount, true, true, false, false, true>(a);
}
__global__ __launch_bounds__(256, 5) void render_head_accum_jitter_wf(Args a)
{
    wf_main<false, true, true, true, false, true>(a);
}
__global__ __launch_bounds__(256) void primary_features_jitter(Args a, float4* __restrict__ out)
{
    primary_features_body<false, true>(a, out);
}

// ------------------------------------------------------------------ ray queries on device buffers
// pt_trace_device / pt_occluded*: a caller's rays, classified ray by ray as trace_rays<false, *> classifies them (the
// BVH4 walk plus winner check, trace_slow, or the reference's walk for a ray outside ray_regular), on a persistent
// grid.  A wave owns the 64 ray indices a grid-stride loop would give it, chunk after chunk; a lane that ends its ray
// takes the chunk's next index (one ballot of the idle lanes, base plus rank each; no atomic) once `refill_at` lanes
// of the wave are idle, instead of waiting for the wave's slowest ray.  refill_at == 64 is trace_rays' lock-step
// loop.  (A global ray counter, per refill or per 1024 indices, was measured and lost: DESIGN.md 3.17, 8.)  Which
// lane traces a ray never changes what the ray computes.  Defined after every other kernel, which therefore compile
// as they did.
// kOccluded: occ[r] = (tri >= 0 && t < tmax[r]) of that trace, without computing the closest hit: the walk starts
// with best_t = min(tmax, MAX_FLOAT), so its strict acceptance 0 < t < best_t is the condition, and it ends at the
// first accepted hit.  That hit counts only if the reference would have tested it (ref_tested); otherwise the exact
// slow walk's closest hit is compared.  Spheres are tested only if no triangle decided.
enum : uint32_t { QS_IDLE = 0, QS_WALK, QS_WALKED };
template <bool kOccluded>
__global__ __launch_bounds__(256) void query_rays(Args a, const float* __restrict__ rays, const float* __restrict__ tmax,
                                                  uint32_t n, uint32_t refill_at,
                                                  int32_t* __restrict__ tri_out, float* __restrict__ t_out,
                                                  uint8_t* __restrict__ occ_out)
{
    extern __shared__ uint32_t lds_tr[];
    const int lane = threadIdx.x & 63;
    Counters cnt;
    Stack4 S;
    S.ring = lds_tr + (threadIdx.x >> 6) * kWaveLdsWords + lane;
    S.stride = a.spill_stride;
    const uint32_t lane_off = (blockIdx.x * blockDim.x + threadIdx.x) * 4u;
    S.spill_base = a.spill;
    S.lane_off = &lane_off;
    S.off_mask = ~0u;
    uint32_t state = QS_IDLE;
    uint32_t r = 0;
    V3 o = v3(0, 0, 0), d = v3(0, 0, 1);
    float tm = kMaxFloat;   // kOccluded: min(tmax, MAX_FLOAT) of the lane's ray
    W4 w;
    walk4_reset(w);
    // (wave-uniform) the wave's chunk of ray indices, and whether the rays have run out
    uint32_t chunk_next = 0, chunk_end = 0;
    uint32_t stride_base = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64u;   // the chunk after this one
    bool drained = false;
    // the end of a ray whose triangles gave (htri, ht): the spheres, the result
    auto finish = [&](int32_t htri, float ht) {
        if (kOccluded) {
            bool occ = htri >= 0 && ht < tm;
            if (!occ)
                for (uint32_t k = 0; k < a.num_spheres; ++k) {
                    const float t = sphere_t(o, d, a.spheres[k]);
                    if (0.0f < t && t < tm) { occ = true; break; }
                }
            occ_out[r] = occ ? 1 : 0;
        } else {
            if (a.num_spheres) apply_spheres(a, o, d, &htri, &ht);
            tri_out[r] = htri;
            t_out[r] = ht;
        }
        state = QS_IDLE;
    };
    for (;;) {
        // ---- the lanes whose walk ended: the winner check (or the exact slow walk), the result
        if (state == QS_WALKED) {
            int32_t htri = -1;
            float ht = kMaxFloat;
            if (w.best_slot != kNone) {
                const float4 C = a.acc_tris[w.best_slot].c;
                htri = (int32_t)__float_as_uint(C.y);
                ht = w.best_t;
                if (!ref_tested(__float_as_uint(C.w), o, d, a.rnodes, a.rparent))
                    trace_slow(o, d, a.root, a.nodes, a.tris_leaf, S.spill(), S.stride, a.cull_rel, a.cull_abs, &htri, &ht);
            }
            finish(htri, ht);
        }
        // ---- refill: the idle lanes take the chunk's next indices (those it cannot serve wait for the next chunk)
        const uint64_t idle = __ballot(state == QS_IDLE);
        if (idle != 0ull && !drained) {
            if (chunk_next == chunk_end) {
                chunk_next = stride_base;   // (n <= 2^29 per launch: no index wraps)
                chunk_end = chunk_next + 64u;
                stride_base += gridDim.x * blockDim.x;
                if (chunk_next >= n) { drained = true; chunk_end = chunk_next; }
                else if (chunk_end > n) chunk_end = n;
            }
            const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            const uint32_t take = min((uint32_t)__popcll(idle), chunk_end - chunk_next);
            if (state == QS_IDLE && rank < take) {
                r = chunk_next + rank;
                const float* p = rays + (size_t)r * 6;
                o = v3(p[0], p[1], p[2]);
                d = v3(p[3], p[4], p[5]);
                bool live = true;
                if (kOccluded) {
                    const float tx = tmax ? tmax[r] : kMaxFloat;
                    live = tx > 0.0f;   // (false for NaN, +-0 and negative bounds: nothing lies before them)
                    tm = __builtin_fminf(tx, kMaxFloat);
                }
                int32_t htri = -1;
                float ht = kMaxFloat;
                if (!live) {
                    occ_out[r] = 0;
                } else if (a.num_tris == 0) {
                    finish(htri, ht);
                } else if (!ray_regular(o, d, a.origin_max)) {
                    // a far origin or a long direction: the reference's walk, its stack in this lane's spill column
                    const Hit h = trace_reference<false>(o, d, a.rnodes, a.tris_orig, S.spill(), 0, cnt, (int)S.stride);
                    finish(h.tri, h.t);
                } else if (!((a.scene_fast != 0u) && ray_fast(o, d))) {
                    trace_slow(o, d, a.root, a.nodes, a.tris_leaf, S.spill(), S.stride, a.cull_rel, a.cull_abs, &htri, &ht);
                    finish(htri, ht);
                } else if (walk4_begin(w, o, d, a.acc_root, a.cull_abs)) {
                    if (kOccluded) w.best_t = tm;   // the walk's bound: only hits with 0 < t < tm are accepted
                    state = QS_WALK;
                } else {
                    finish(htri, ht);
                }
            }
            chunk_next += take;
        }
        // ---- walk: one BVH4 step per walking lane, until refill_at lanes are idle again
        if (__ballot(state == QS_WALK) == 0ull) {
            if (drained) break;   // (no lane walks and none can begin: all are idle)
            continue;
        }
        for (;;) {
            if (state == QS_WALK) {
                bool more = walk4_step<false>(w, o, d, a.nodes4, a.acc_tris, S, a.cull_rel, a.cull_abs, a.node_mask, cnt);
                if (kOccluded && w.best_slot != kNone) more = false;   // any accepted hit decides
                if (!more) state = QS_WALKED;
            }
            const uint64_t walking = __ballot(state == QS_WALK);
            if (walking == 0ull) break;
            if (!drained && 64u - (uint32_t)__popcll(walking) >= refill_at) break;
        }
    }
}

// ------------------------------------------------------------------ renders along caller-supplied rays
// pt_render_rays*: the kernels of a render whose rays come from RayArgs::rays (kRays) -- the set-up kernel, the two
// integrators' wavefront kernels at the default occupancy (integrator 0's with its LDS-walk twin) and the tile kernel
// -- defined and first used after every other kernel, which therefore compile as they did.
__global__ __launch_bounds__(256) void init_pixel_states_rays(RayArgs a, uint32_t* __restrict__ st)
{
    init_pixel_states_body<false, true>(a, st);
}
template <bool kLdsWalk>
__global__ __launch_bounds__(256, 5) void render_unidir_rays_wf(RayArgs a)
{
    wf_main<false, false, kLdsWalk, false, false, false, true>(a);
}
__global__ __launch_bounds__(256, 5) void render_head_rays_wf(RayArgs a)
{
    wf_main<false, true, true, false, false, false, true>(a);
}
template <int kIntegrator, bool kRefWalk, bool kCount>
__global__ __launch_bounds__(64) void render_tiles_rays(RayArgs a)
{
    render_tiles_body<kIntegrator, kRefWalk, kCount, false, false, true>(a);
}

// ------------------------------------------------------------------ accumulators and features over caller-supplied rays
// pt_accum_create_rays* / pt_render_features_rays*: the accumulating twins of the two ray-source wavefront kernels, the
// set-up of an adaptive pass over a ray accumulator and the features kernel with a ray source -- again defined and
// first used after every other kernel, which therefore compile as they did.  The unfrozen
// accumulating pass is set up by init_pixel_states_rays, whose body honours Args::accum.
template <bool kLdsWalk>
__global__ __launch_bounds__(256, 5) void render_unidir_accum_rays_wf(RayArgs a)
{
    wf_main<false, false, kLdsWalk, true, false, false, true>(a);
}
__global__ __launch_bounds__(256, 5) void render_head_accum_rays_wf(RayArgs a)
{
    wf_main<false, true, true, true, false, false, true>(a);
}

__global__ __launch_bounds__(256) void init_active_states_rays(RayArgs a, uint32_t* __restrict__ st, const uint32_t* __restrict__ list)
{
    init_active_states_body<false, true>(a, st, list);
}
__global__ __launch_bounds__(256) void primary_features_rays(RayArgs a, float4* __restrict__ out)
{
    primary_features_body<false, false, true>(a, out);
}

// ------------------------------------------------------------------ irradiance renders at caller-supplied points
// pt_render_irradiance*: the kernels of a render whose every sample leaves its pixel's point along a cosine-weighted
// direction about the point's normal (kPts; RayArgs::rays names the point buffer) -- the set-up kernel, the two
// integrators' wavefront kernels at the default occupancy and the tile kernel -- defined and first used after every
// other kernel once more, which therefore compile as they did.
__global__ __launch_bounds__(256) void init_pixel_states_points(RayArgs a, uint32_t* __restrict__ st)
{
    init_pixel_states_body<false, false, true>(a, st);
}
template <bool kLdsWalk>
__global__ __launch_bounds__(256, 5) void render_unidir_points_wf(RayArgs a)
{
    wf_main<false, false, kLdsWalk, false, false, false, false, true>(a);
}
__global__ __launch_bounds__(256, 5) void render_head_points_wf(RayArgs a)
{
    wf_main<false, true, true, false, false, false, false, true>(a);
}
template <int kIntegrator, bool kRefWalk, bool kCount>
__global__ __launch_bounds__(64) void render_tiles_points(RayArgs a)
{
    render_tiles_body<kIntegrator, kRefWalk, kCount, false, false, false, true>(a);
}

// ------------------------------------------------------------------ accumulators over caller-supplied points
// pt_accum_create_points*: the accumulating twins of the two point-source wavefront kernels and the set-up of an
// adaptive pass over a point accumulator -- defined and first used after every other kernel yet again, which
// therefore compile as they did.  The unfrozen accumulating pass is set up by
// init_pixel_states_points, whose body honours Args::accum: the stream continues from acc_rng, the sample numbers
// from acc_n0, a whole-pixel unit carries its slot, and a split unit's replay skips the sample's pair as a lens
// unit's does.
template <bool kLdsWalk>
__global__ __launch_bounds__(256, 5) void render_unidir_accum_points_wf(RayArgs a)
{
    wf_main<false, false, kLdsWalk, true, false, false, false, true>(a);
}
__global__ __launch_bounds__(256, 5) void render_head_accum_points_wf(RayArgs a)
{
    wf_main<false, true, true, true, false, false, false, true>(a);
}

__global__ __launch_bounds__(256) void init_active_states_points(RayArgs a, uint32_t* __restrict__ st, const uint32_t* __restrict__ list)
{
    init_active_states_body<false, false, true>(a, st, list);
}

}  // namespace

#include "pt_render_host.h"
