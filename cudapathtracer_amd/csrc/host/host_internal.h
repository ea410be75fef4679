// host_internal.h -- shared declarations of the host surface (plain C++17, no HIP).
#pragma once

#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pt/pt.h"

static_assert(sizeof(pt_vec3) == 12, "vec3 is 12 B (vec3.h:4-7)");
static_assert(sizeof(pt_triangle) == 28, "triangle is 28 B (modelLoader.h:14-19)");
static_assert(sizeof(pt_material) == 48, "materialDesc is 48 B (modelLoader.h:21-25)");
static_assert(sizeof(pt_sphere) == 64, "sphere.h sphere is 64 B");
static_assert(sizeof(pt_bvh_node) == 32, "BVH_array_node is 32 B (BVH.h:111-115)");
static_assert(sizeof(pt_camera) == 32, "camera is 32 B (camera.h:26-34)");
static_assert(sizeof(pt_view) == 44, "pt_view is 44 B (11 floats, no padding)");

namespace pt {

// Thread-local error channel behind pt_last_error().
int fail(int code, const char* fmt, ...);
void clear_error();

// The condition a pt_view must meet (pt.h: finite, film > 0, orthonormal to 1e-3 in double); PT_E_INVALID under
// `who`'s name otherwise (scene.cpp).
int validate_view(const char* who, const pt_view* v);

// The jitter bits of pt_params.flags (pt.h): PT_FLAG_JITTER_TENT only together with PT_FLAG_JITTER; PT_E_INVALID under
// `who`'s name otherwise (scene.cpp).
int validate_jitter_flags(const char* who, uint32_t flags);

// The HIP device ordinal a render context lives on (pt_render_host.h; used by pt_multi.cpp).
int ctx_device(const pt_ctx* c);

// 64-bit FNV-1a over a byte range, chained through `h` (pt_accel_digest, the scene digest of pt_create).
constexpr uint64_t kFnvBasis = 1469598103934665603ull;
inline uint64_t fnv1a(const void* p, size_t n, uint64_t h = kFnvBasis)
{
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= c[i]; h *= 1099511628211ull; }
    return h;
}

// ---- accumulating passes: what pt_accum.cpp (the pt_accum_* entry points) needs of a render context
// (pt_render_host.h).  The state is device memory of the context's device, in the shard's work-slot order:
// rng[k * slots + q] (k = v0..v4, d) and mean[k * slots + q] (k = r, g, b) of slot q.
struct AccumPass {
    uint32_t n0;      // samples every pixel (an adaptive pass: every active pixel) has before this pass
    uint32_t* rng;
    double* mean;
    // an adaptive pass (pt_accum.cpp, once a pixel is frozen): only the work slots active[0..nactive-1] (device,
    // ascending) are sampled, one whole-pixel unit each; null: every pixel of the shard, as planned by plan_units
    const uint32_t* active = nullptr;
    uint32_t nactive = 0;
    // a pass of a ray accumulator (pt_accum_create_rays*): its own copy of the rays (device, width * height * 6 floats,
    // every one regular), indexed in the accumulator's pixel order; cam is then the stand-in of accum_check_rays
    const float* rays = nullptr;
    // a pass of a point accumulator (pt_accum_create_points*): rays holds its own copy of the points {p, n}, every one
    // regular, and every sample leaves its pixel's point along a cosine-weighted direction (pt_render_irradiance's loop)
    bool points = false;
};
// Validates (params, cam) as pt_render_device_async does and refuses every mode without an accumulating
// kernel (render_tiles, the counting variants, non-default occupancy).
// (view: the accumulator's pt_view, or null for the reference camera)
int accum_check(const pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view);
// The same for an accumulator over a ray buffer (pt_accum_create_rays*): the flags a ray render and an accumulator
// both take, the parameters, the kernels.  *stand_in: the camera the passes are enqueued with -- at the origin, it
// carries the image size alone.  (points: an accumulator over a point buffer, pt_accum_create_points* -- the same
// checks under its own name)
int accum_check_rays(const pt_ctx* c, const pt_params* p, pt_camera* stand_in, bool points = false);
// Classifies the accumulator's own ray copy (device, width * height rays) and refuses it unless every ray is regular:
// an invalid ray with its lowest pixel named, irregular rays with their count.  Blocking.
// (points: the copy holds points {p, n}, classified as pt_render_irradiance classifies them)
int accum_classify_rays(pt_ctx* c, const pt_params* p, const float* d_rays, void* stream, bool points = false);
// p->spp more samples of every pixel (of every active pixel), blocking; d_out (device, W*H*3) may be null.
int accum_pass(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, const AccumPass& acc, float* d_out,
               void* stream, pt_stats* stats);
// Work slot q of the shard -> scanline pixel id y*W + x, or 0xffffffff for a slot outside the image.
int shard_slots(const pt_params* p, std::vector<uint32_t>* pix);
// The FNV-1a digest of the scene arrays the context was created from, and their primitive counts.
void ctx_scene_id(const pt_ctx* c, uint64_t* digest, uint32_t* num_tris, uint32_t* num_spheres);
int ctx_in_flight(const pt_ctx* c);
uint32_t accum_max_samples();

// ---- what the noise estimator (pt_noise.hip) needs of an accumulator (pt_accum.cpp): read-only, except the
// slot that names the accumulator's one live estimator (null: none)
struct AccumView {
    pt_ctx* ctx;
    const pt_params* params;
    const double* mean;                      // device, mean[k * slots + q]
    const std::vector<uint32_t>* slot_pix;   // work slot -> scanline pixel id, 0xffffffff outside the image
    int64_t samples;
    pt_noise** noise;
    // adaptive sampling: null until the accumulator has a frozen pixel; then per work slot the sample count the
    // pixel was frozen at, kSlotActive for a pixel still sampled (its count is `samples`), 0 outside the image
    const uint32_t* frozen_at;               // device
    uint64_t pixels;                         // work slots inside the image
};
AccumView accum_view(pt_accum* acc);
constexpr uint32_t kSlotActive = 0xffffffffu;
// The frozen_at plane for a device sweep that freezes pixels (pt_noise_freeze), allocated on first use; the sweep
// reports how many pixels it froze with accum_frozen (which drops the accumulator's active list).
int accum_freeze_plane(pt_accum* acc, uint32_t** plane);
void accum_frozen(pt_accum* acc, uint64_t newly_frozen);
// ---- the active list (pt_adaptive.hip): ordered compaction of the slots with frozen_at == kSlotActive into
// list[0..*count-1] (ascending), on the device; block_tot: scratch of adaptive_scan_words(slots) words.
// Blocking: only *count comes back.
size_t adaptive_scan_words(size_t slots);
int adaptive_compact(const uint32_t* frozen_at, size_t slots, uint32_t* list, uint32_t* block_tot, void* stream,
                     uint32_t* count);

// ---- the denoiser (pt_denoise.hip) keeps its device scratch in the render context (pt_render_host.h), which
// frees it in pt_destroy
struct DenoiseScratch {
    void* mem = nullptr;
    size_t bytes = 0;
};
DenoiseScratch* ctx_denoise_scratch(pt_ctx* c);
int ctx_num_cus(const pt_ctx* c);

// ---- the classes of a ray buffer (pt_rays.hip): d_rays[0..n) on the current device, 8-byte aligned, against
// origin_max = 64 scene extents; d_words: four device words the context keeps.  Blocking: *out is final on return.
// points: the records are the points {p, n} of an irradiance render, classified by pt.h's point classes.
int classify_ray_buffer(const float* d_rays, uint32_t n, float origin_max, int num_cus, uint32_t* d_words, void* stream,
                  pt_ray_classes* out, bool points = false);

// PT_TIMING=1: the host wall time of each stage of a checkpoint / session save or load on stderr, "who: stage ms"
// (every stage ends in a blocking call; the measurements of DESIGN.md 8).
struct StageTimer {
    const char* who;
    bool on = getenv("PT_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char* what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "%s: %-18s %9.3f ms\n", who, what, std::chrono::duration<double, std::milli>(now - t0).count());
        t0 = now;
    }
};

// ---- session files (pt_session.cpp: the pt_session_* entry points and the file; pt_session.hip: the pack / unpack
// kernels).  What they need of an accumulator (pt_accum.cpp), an estimator (pt_noise.hip) and the context.
struct SessionAccum {
    pt_ctx* ctx;
    const pt_params* params;
    const pt_camera* cam;
    const pt_view* view;           // null: the reference camera (a version-2 file)
    int64_t samples;
    size_t slots;
    uint64_t pixels;               // work slots inside the image
    uint32_t* rng;                 // device, rng[k * slots + q]
    double* mean;                  // device, mean[k * slots + q]
    uint32_t* frozen_at;           // device; null unless a pixel was ever frozen
    const uint32_t* slot_pix;      // device: work slot -> scanline pixel id, 0xffffffff outside the image
    pt_noise* noise;               // the live estimator, or null
};
// (uploads the slot -> pixel map on first use)
int accum_session(pt_accum* acc, SessionAccum* out);
// A new accumulator at `samples` whose planes session_unpack fills; counts: with the frozen_at plane, in the state
// pt_accum_freeze leaves (a pixel is frozen, the active list invalid).  Null with *code set on failure.
pt_accum* accum_session_new(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, int64_t samples, bool counts,
                            int* code);
struct SessionNoise {
    double* state;                 // device: prev[3], mu, m2 planes of slots doubles
    uint32_t* pix;                 // device: W_q, b_q planes of slots words; null unless they carry the state
    int64_t n0;
    double W;
    int32_t batches;
};
void noise_session(pt_noise* noise, SessionNoise* out);
// A new estimator attached to `acc` with the given window (not a fresh one) whose planes session_unpack fills;
// per_pixel: with live W_q / b_q planes.
pt_noise* noise_session_new(pt_accum* acc, int64_t n0, double W, int32_t batches, bool per_pixel, int* code);
// The staging of a session save / load: one device buffer and its pinned host twin, `bytes` each, grown on demand
// inside the context and freed by pt_destroy.
struct SessionScratch {
    void* dev = nullptr;
    void* host = nullptr;
    size_t bytes = 0;
};
SessionScratch* ctx_session_scratch(pt_ctx* c);
// Where a staging buffer holds what: the frozen / illegal counters first, then each section of the file at a
// 256-byte boundary (a section's offset is 0 when the file has none).
constexpr int kSessionSumCopies = 32;    // copies of the counters; block b adds into copy b % kSessionSumCopies
constexpr int kSessionSumWords = 2;      // frozen pixels, illegal section-B words
struct SessionLayout {
    size_t a = 0, b = 0, c = 0, d = 0;   // byte offsets of sections A..D
    size_t bytes = 0;
};
constexpr size_t kSessionSumBytes = (size_t)kSessionSumCopies * kSessionSumWords * sizeof(unsigned long long);
// The planes a kernel packs from / unpacks into (null: the file has no such section) and the staging.
struct SessionPlanes {
    uint32_t* rng;
    double* mean;
    uint32_t* frozen_at;
    double* nstate;
    uint32_t* npix;
    const uint32_t* slot_pix;
    unsigned char* stage;          // device staging, laid out by `at`
    SessionLayout at;
    size_t slots;
    size_t image_pixels;           // W*H
    uint32_t samples;
};
// Enqueue on `stream` (nothing is launched for 0 slots).  session_pack: the planes into the staging's sections, and
// the frozen pixels into its counters.  session_unpack: the sections into the planes, slots outside the image as
// a new accumulator / estimator has them, and the frozen pixels and illegal section-B words into the counters.
int session_pack(pt_ctx* c, const SessionPlanes& pl, void* stream);
int session_unpack(pt_ctx* c, const SessionPlanes& pl, void* stream);

// ---- OBJ/MTL ingest with tinyobj 0.9.13 semantics (tiny_obj_loader.cc) ------------------
// Only what loadOBJ (modelLoader.h:125-210) consumes is kept: positions, per-triangle
// indices, per-triangle material ids, material diffuse/emission.  Vertex dedupe keys still
// include the vt/vn indices, since they decide how many positions a shape gets.
struct ObjMaterial {
    std::string name;
    float diffuse[3];
    float emission[3];
};
struct ObjShape {
    std::string name;
    std::vector<float> positions;       // xyz per deduplicated vertex
    std::vector<uint32_t> indices;      // 3 per triangle
    std::vector<int> material_ids;      // 1 per triangle
};
struct ObjResult {
    std::vector<ObjShape> shapes;
    std::vector<ObjMaterial> materials;
    std::string message;                // tinyobj's returned error/warning string
    bool fatal = false;                 // file could not be opened / malformed index
};
ObjResult read_obj(const std::string& path, const std::string& mtl_basepath);

// Greedy decimal parser of tinyobj's tryParseDouble (tiny_obj_loader.cc:127-241).
bool parse_real(const char* s, const char* end, double* out);

// ---- scene (the reference's globals, modelLoader.h:43-47) -------------------------------
struct HostScene {
    std::vector<pt_vec3> verts;
    std::vector<pt_triangle> tris;
    std::vector<pt_material> mats;
    std::vector<uint32_t> lights;
    float total_light_area = 0.0f;
    std::vector<pt_bvh_node> bvh;
    int32_t bvh_depth = 0;
    std::vector<pt_sphere> spheres;
    std::string warning;
};

// Area of an emissive sphere light: 4*3.14159*r^2 evaluated in float, left to right.
inline float sphere_area(float r) { return 4.0f * 3.14159f * r * r; }

// Deterministic float sin/cos shared with the kernels (defined in hip/pt_render_host.h over pt_device.h's det_sincos).
void sincos_det(float theta, float* s, float* c);
bool tonemap_thresholds(float t[256]);
// host threads for the parallel builders: PT_HOST_THREADS, else OMP_NUM_THREADS, else the
// hardware concurrency, capped at 16
unsigned host_threads();
bool morton_size_ok(int w, int h);   // square power-of-two image (the reference's Morton imgBuff)
// Device -> host copy of a finished image through a pinned staging buffer (*pinned, grown as needed,
// owned by the caller's context / group; freed with free_pinned): one DMA on `stream` (a
// hipStream_t), then host_threads() threads copy the staging buffer into dst -- a pageable
// destination's first-touch page faults spread over the threads instead of serialising the DMA.
int copy_to_host(void* dst, const void* src_dev, size_t bytes, void* stream, void** pinned, size_t* pinned_bytes);
void free_pinned(void* pinned);

// ---- render-path acceleration structure (accel_build.cpp) --------------------------------
struct AccelNode {
    float box[2][6];       // child boxes (lo xyz, hi xyz), inflated by `margin`
    uint32_t child[2];     // inner node index, or a leaf: PT_BVH_LEAF_FLAG | (count - 1) << 29 | first slot
};
// a leaf of the render-path BVH holds 1..kAccelLeafMax triangles at consecutive leaf slots
constexpr uint32_t kAccelLeafMax = 2;
inline uint32_t accel_leaf_count(uint32_t ref) { return ((ref >> 29) & 3u) + 1u; }
inline uint32_t accel_leaf_slot(uint32_t ref) { return ref & 0x1fffffffu; }
struct AccelBvh {
    std::vector<AccelNode> nodes;        // node 0 = root
    std::vector<uint32_t> leaf_order;    // triangle id of each leaf slot
    float root_box[6];
    int depth = 0;
    float margin = 0.0f;
};
int build_accel(const pt_scene& sc, AccelBvh* out);
// SAH cost of the binary tree: the sum of its inner-node surface areas
double accel_sah_cost(const AccelBvh& acc);

// 4-wide collapse of the binary SAH BVH: each node holds up to 4 children (largest-area
// expansion, at most kAccel4LeafTris triangles in its leaf children), empty slots are
// kAccel4Empty; leaves keep their binary-BVH refs (count and first leaf slot).
constexpr uint32_t kAccel4Empty = 0xffffffffu;
constexpr uint32_t kAccel4LeafTris = 8;    // at most this many triangles in a node's leaf children (kLeafBits)
struct Accel4Node {
    float lo[3][4], hi[3][4];   // [axis][child]
    uint32_t child[4];          // inner node index, PT_BVH_LEAF_FLAG | slot, or kAccel4Empty
};
struct Accel4 {
    std::vector<Accel4Node> nodes;       // node 0 = root
    int depth = 0;
};
int collapse_accel4(const AccelBvh& bin, Accel4* out);
// c_node x inner-node surfaces + c_tri x leaf surfaces x triangles, over the root's (diagnostic)
double accel4_cost(const Accel4& t, const float* root_box, double cn, double ct);
// every node and leaf slot reached once, <= kAccel4LeafTris leaf triangles per node, nested boxes
int validate_accel4(const AccelBvh& bin, const Accel4& t);

// ---- BVH (BVH.h) ------------------------------------------------------------------------
int build_bvh(const std::vector<pt_vec3>& verts, const std::vector<pt_triangle>& tris,
              std::vector<pt_bvh_node>* out, int32_t* depth);

}  // namespace pt

struct pt_host_scene {
    pt::HostScene s;
};
