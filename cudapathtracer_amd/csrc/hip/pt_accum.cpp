// pt_accum.cpp -- resumable sample accumulation (include/pt/pt.h, pt_accum_*): the reference's progressive
// loop (kernel.cu:702-737: one drawPixel launch per sample over randState_device and imgBuffer_device,
// kernel.cu:527-553) as passes of the wavefront kernels over a per-pixel state kept on the device, and that
// state's checkpoint file.  Host code over the HIP runtime (no kernels): the passes themselves are
// pt::accum_pass (pt_render_host.h).
// Adaptive sampling (pt_accum_freeze, pt_noise_freeze): a frozen pixel is never sampled again.  Its slot of the
// frozen_at plane holds the sample count it stopped at; the other pixels all have `samples`.  Once a pixel is
// frozen a pass runs over the active list (pt_adaptive.hip), rebuilt only when the frozen set changed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../host/host_internal.h"
#include "pt_hip_util.h"

namespace {

// The checkpoint header (documented in pt.h); every field little-endian at a fixed offset.
constexpr char kMagic[8] = {'P', 'T', 'A', 'C', 'C', 'U', 'M', '\0'};
constexpr uint32_t kVersion = 1;
constexpr size_t kRecordBytes = 48;
struct Header {
    char magic[8];
    uint32_t version;
    uint32_t header_bytes;
    pt_params params;        // 56 B: spp = 0, the 4 bytes of tail padding 0
    pt_camera cam;           // 32 B
    int64_t samples;
    uint64_t scene_digest;
    uint32_t num_tris, num_spheres;
};
static_assert(sizeof(pt_params) == 56, "pt_params is 56 B in the checkpoint header");
static_assert(sizeof(Header) == 128, "checkpoint header is 128 B");
struct Record {
    uint32_t rng[6];   // v0..v4, d
    double mean[3];
};
static_assert(sizeof(Record) == kRecordBytes, "checkpoint record is 48 B");

bool little_endian()
{
    const uint32_t one = 1;
    unsigned char b;
    memcpy(&b, &one, 1);
    return b == 1;
}

// Reads and validates the header of `path`; *file_bytes = the file's size.
int read_header(const char* what, const char* path, Header* h, FILE** keep)
{
    if (!little_endian()) return pt::fail(PT_E_INVALID, "%s: checkpoint files are little-endian; this host is not", what);
    FILE* f = fopen(path, "rb");
    if (!f) return pt::fail(PT_E_IO, "%s: cannot open %s", what, path);
    auto bail = [&](int code) { fclose(f); return code; };
    if (fread(h, 1, sizeof(Header), f) != sizeof(Header))
        return bail(pt::fail(PT_E_IO, "%s: %s is shorter than the %zu-byte header", what, path, sizeof(Header)));
    if (memcmp(h->magic, kMagic, 8) != 0) return bail(pt::fail(PT_E_INVALID, "%s: %s is not a checkpoint file (bad magic)", what, path));
    if (h->version != kVersion)
        return bail(pt::fail(PT_E_INVALID, "%s: %s has format version %u, this build reads %u", what, path, h->version, kVersion));
    if (h->header_bytes != sizeof(Header))
        return bail(pt::fail(PT_E_INVALID, "%s: %s has a %u-byte header, expected %zu", what, path, h->header_bytes, sizeof(Header)));
    const pt_params& p = h->params;
    if (p.width <= 0 || p.height <= 0 || p.width > 65535 || p.height > 65535 || h->samples < 0 ||
        h->samples > (int64_t)pt::accum_max_samples())
        return bail(pt::fail(PT_E_INVALID, "%s: %s: image %dx%d with %lld samples is out of range", what, path, p.width, p.height,
                             (long long)h->samples));
    if (fseek(f, 0, SEEK_END) != 0) return bail(pt::fail(PT_E_IO, "%s: cannot seek in %s", what, path));
    const long long size = ftell(f);
    const long long want = (long long)sizeof(Header) + (long long)p.width * p.height * (long long)kRecordBytes;
    if (size < want)
        return bail(pt::fail(PT_E_IO, "%s: %s is truncated: %lld bytes, %dx%d records need %lld", what, path, size, p.width, p.height, want));
    if (size > want)
        return bail(pt::fail(PT_E_INVALID, "%s: %s has %lld bytes, %dx%d records make %lld", what, path, size, p.width, p.height, want));
    if (keep) {
        if (fseek(f, (long)sizeof(Header), SEEK_SET) != 0) return bail(pt::fail(PT_E_IO, "%s: cannot seek in %s", what, path));
        *keep = f;
    } else {
        fclose(f);
    }
    return PT_OK;
}

}  // namespace

struct pt_accum {
    pt_ctx* ctx = nullptr;
    pt_params params;
    pt_camera cam;
    pt_view view;                     // the oriented camera, kept for life like cam (has_view)
    bool has_view = false;
    int64_t samples = 0;
    std::vector<uint32_t> slot_pix;   // work slot -> scanline pixel id (0xffffffff: outside the image)
    uint32_t* d_rng = nullptr;        // 6 words per slot, word-major
    double* d_mean = nullptr;         // 3 doubles per slot, channel-major
    pt_noise* noise = nullptr;        // the live estimator attached to this accumulator (pt_noise.hip), if any
    // adaptive sampling, allocated on first use (an accumulator that never freezes a pixel has none of it)
    uint64_t pixels = 0;              // work slots inside the image
    uint32_t* d_frozen_at = nullptr;  // per slot: pt::kSlotActive, or the count the pixel was frozen at (0 outside the image)
    uint32_t* d_list = nullptr;       // the active slots, ascending (slots() entries)
    uint32_t* d_scan = nullptr;       // the compaction's block totals
    bool any_frozen = false;          // a pixel was frozen: passes run over the list from now on
    bool list_valid = false;
    uint32_t nactive = 0;             // entries of d_list (list_valid)
    uint32_t* d_slot_pix = nullptr;   // slot_pix on the device, uploaded when a session file first needs it (pt_session.hip)
    float* d_rays = nullptr;          // a ray accumulator's own copy of its rays (width * height * 6 floats), kept for life
    bool points = false;              // d_rays holds points {p, n}: a point accumulator (pt_accum_create_points*)
    size_t slots() const { return slot_pix.size(); }
};

pt::AccumView pt::accum_view(pt_accum* a)
{
    return pt::AccumView{a->ctx, &a->params, a->d_mean, &a->slot_pix, a->samples, &a->noise,
                         a->any_frozen ? a->d_frozen_at : nullptr, a->pixels};
}

namespace {

// The adaptive planes, allocated on first use: every pixel active, slots outside the image frozen at 0.
int adaptive_alloc(pt_accum* a)
{
    if (a->d_frozen_at) return PT_OK;
    const size_t n = a->slots() ? a->slots() : 1;
    std::vector<uint32_t> init(n, 0u);
    for (size_t q = 0; q < a->slots(); ++q)
        if (a->slot_pix[q] != 0xffffffffu) init[q] = pt::kSlotActive;
    HIP_TRY(hipSetDevice(pt::ctx_device(a->ctx)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&a->d_frozen_at), n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&a->d_list), n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&a->d_scan), pt::adaptive_scan_words(n) * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(a->d_frozen_at, init.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    a->list_valid = false;
    return PT_OK;
}

// The active list of the frozen set as it stands (rebuilt only after a freeze).
int active_list(pt_accum* a, void* stream)
{
    if (int rc = adaptive_alloc(a)) return rc;
    if (a->list_valid) return PT_OK;
    HIP_TRY(hipSetDevice(pt::ctx_device(a->ctx)));
    if (int rc = pt::adaptive_compact(a->d_frozen_at, a->slots(), a->d_list, a->d_scan, stream, &a->nactive)) return rc;
    a->list_valid = true;
    return PT_OK;
}

// Every slot's sample count (0 outside the image).
int fetch_counts(pt_accum* a, std::vector<uint32_t>* cnt)
{
    const size_t n = a->slots();
    cnt->assign(n, 0u);
    if (a->d_frozen_at && n) {
        HIP_TRY(hipSetDevice(pt::ctx_device(a->ctx)));
        HIP_TRY(hipMemcpy(cnt->data(), a->d_frozen_at, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    for (size_t q = 0; q < n; ++q) {
        if (a->slot_pix[q] == 0xffffffffu) (*cnt)[q] = 0u;
        else if (!a->d_frozen_at || (*cnt)[q] == pt::kSlotActive) (*cnt)[q] = (uint32_t)a->samples;
    }
    return PT_OK;
}

// The index of scanline pixel `pix` in the accumulator's pixel order.
size_t order_index(const pt_accum* a, uint32_t pix)
{
    const uint32_t w = (uint32_t)a->params.width;
    return a->params.pixel_order == PT_ORDER_MORTON ? (size_t)pt_morton_pxl_to_i(pix % w, pix / w) : (size_t)pix;
}

}  // namespace

int pt::accum_freeze_plane(pt_accum* a, uint32_t** plane)
{
    if (int rc = adaptive_alloc(a)) return rc;
    *plane = a->d_frozen_at;
    return PT_OK;
}

void pt::accum_frozen(pt_accum* a, uint64_t newly_frozen)
{
    if (!newly_frozen) return;
    a->any_frozen = true;
    a->list_valid = false;
}

namespace {
pt_accum* make_accum(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, int* code);
}

int pt::accum_session(pt_accum* a, pt::SessionAccum* out)
{
    if (!a->d_slot_pix) {
        const size_t n = a->slots() ? a->slots() : 1;
        HIP_TRY(hipSetDevice(pt::ctx_device(a->ctx)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&a->d_slot_pix), n * sizeof(uint32_t)));
        if (a->slots()) HIP_TRY(hipMemcpy(a->d_slot_pix, a->slot_pix.data(), a->slots() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    *out = pt::SessionAccum{a->ctx, &a->params, &a->cam, a->has_view ? &a->view : nullptr, a->samples, a->slots(), a->pixels, a->d_rng, a->d_mean,
                            a->any_frozen ? a->d_frozen_at : nullptr, a->d_slot_pix, a->noise};
    return PT_OK;
}

pt_accum* pt::accum_session_new(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, int64_t samples,
                                bool counts, int* code)
{
    pt_accum* a = make_accum(c, p, cam, view, code);
    if (!a) return nullptr;
    a->samples = samples;
    if (counts) {
        *code = adaptive_alloc(a);
        if (*code != PT_OK) { pt_accum_destroy(a); return nullptr; }
        a->any_frozen = true;
        a->list_valid = false;
    }
    return a;
}

namespace {

// The accumulator of (c, p, cam, view) with zeroed state (0 samples), or null with the error recorded.
pt_accum* make_accum(pt_ctx* c, const pt_params* p, const pt_camera* cam, const pt_view* view, int* code)
{
    *code = pt::accum_check(c, p, cam, view);
    if (*code != PT_OK) return nullptr;
    pt_accum* a = new (std::nothrow) pt_accum();
    if (!a) { *code = pt::fail(PT_E_OOM, "pt_accum_create: out of host memory"); return nullptr; }
    a->ctx = c;
    memset(&a->params, 0, sizeof(a->params));   // (padding too: the header is written from it)
    a->params.width = p->width; a->params.height = p->height; a->params.spp = 0; a->params.bounces = p->bounces;
    a->params.integrator = p->integrator; a->params.flags = p->flags; a->params.seed = p->seed;
    a->params.shard_index = p->shard_index; a->params.shard_count = p->shard_count; a->params.pixel_order = p->pixel_order;
    a->params.tile_w = p->tile_w; a->params.tile_h = p->tile_h;
    a->cam = *cam;
    memset(&a->view, 0, sizeof(a->view));
    if (view) { a->view = *view; a->has_view = true; }
    pt::shard_slots(&a->params, &a->slot_pix);
    for (const uint32_t pix : a->slot_pix) a->pixels += pix != 0xffffffffu;
    auto alloc = [&]() -> int {
        HIP_TRY(hipSetDevice(pt::ctx_device(c)));
        const size_t n = a->slots() ? a->slots() : 1;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&a->d_rng), n * 6 * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&a->d_mean), n * 3 * sizeof(double)));
        HIP_TRY(hipMemset(a->d_rng, 0, n * 6 * sizeof(uint32_t)));
        HIP_TRY(hipMemset(a->d_mean, 0, n * 3 * sizeof(double)));
        HIP_TRY(hipDeviceSynchronize());
        return PT_OK;
    };
    *code = alloc();
    if (*code != PT_OK) { pt_accum_destroy(a); return nullptr; }
    return a;
}

// The state as scanline records (pixels outside the shard: all zero).
int fetch_records(pt_accum* a, std::vector<Record>* rec)
{
    const size_t n = a->slots();
    std::vector<uint32_t> rng(n * 6);
    std::vector<double> mean(n * 3);
    HIP_TRY(hipSetDevice(pt::ctx_device(a->ctx)));
    if (n) {
        HIP_TRY(hipMemcpy(rng.data(), a->d_rng, n * 6 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(mean.data(), a->d_mean, n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    }
    Record zero;
    memset(&zero, 0, sizeof(zero));
    rec->assign((size_t)a->params.width * a->params.height, zero);
    if (a->samples == 0) return PT_OK;
    for (size_t q = 0; q < n; ++q) {
        const uint32_t pix = a->slot_pix[q];
        if (pix == 0xffffffffu) continue;
        Record& r = (*rec)[pix];
        for (int k = 0; k < 6; ++k) r.rng[k] = rng[(size_t)k * n + q];
        for (int k = 0; k < 3; ++k) r.mean[k] = mean[(size_t)k * n + q];
    }
    return PT_OK;
}

}  // namespace

extern "C" {

pt_accum* pt_accum_create_view(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, const pt_view* view, int* err)
{
    pt::clear_error();
    int code;
    pt_accum* a = nullptr;
    if (!ctx || !params || !cam) code = pt::fail(PT_E_INVALID, "pt_accum_create: null argument");
    else a = make_accum(ctx, params, cam, view, &code);
    if (err) *err = code;
    return a;
}

pt_accum* pt_accum_create(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, int* err)
{
    return pt_accum_create_view(ctx, params, cam, nullptr, err);
}

// The accumulator of (c, p) over a copy of the width * height rays at `rays` (host memory, or device memory read on
// `stream`), or null with the error recorded: the checks in pt.h's order, the copy, then the copy's classes.
// (points: the records are points {p, n} and the accumulator is a point accumulator, pt_accum_create_points*)
static pt_accum* make_accum_rays(pt_ctx* c, const pt_params* p, const float* rays, bool host, void* stream, int* code,
                                 bool points = false)
{
    const char* who = points ? "pt_accum_create_points" : "pt_accum_create_rays";
    if (pt::ctx_in_flight(c) > 0) {
        *code = pt::fail(PT_E_INVALID, "%s: %d asynchronous renders in flight (pt_render_wait first)", who, pt::ctx_in_flight(c));
        return nullptr;
    }
    pt_camera cam;
    *code = pt::accum_check_rays(c, p, &cam, points);
    if (*code != PT_OK) return nullptr;
    if (!host && reinterpret_cast<uintptr_t>(rays) % 8 != 0) {
        *code = pt::fail(PT_E_INVALID, "%s: the %s buffer must be 8-byte aligned", who, points ? "point" : "ray");
        return nullptr;
    }
    pt_accum* a = make_accum(c, p, &cam, nullptr, code);
    if (!a) return nullptr;
    a->points = points;
    auto copy = [&]() -> int {
        const size_t bytes = (size_t)p->width * (size_t)p->height * 6 * sizeof(float);
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&a->d_rays), bytes));
        if (host) {
            HIP_TRY(hipMemcpy(a->d_rays, rays, bytes, hipMemcpyHostToDevice));
        } else {
            HIP_TRY(hipMemcpyAsync(a->d_rays, rays, bytes, hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream)));
        }
        // (its own copy is what gets classified: what the passes read is what was checked)
        return pt::accum_classify_rays(c, p, a->d_rays, host ? nullptr : stream, points);
    };
    *code = copy();
    if (*code != PT_OK) { pt_accum_destroy(a); return nullptr; }
    return a;
}

pt_accum* pt_accum_create_rays_device(pt_ctx* ctx, const pt_params* params, const float* d_rays, void* stream, int* err)
{
    pt::clear_error();
    int code;
    pt_accum* a = nullptr;
    if (!ctx || !params || !d_rays) code = pt::fail(PT_E_INVALID, "pt_accum_create_rays: null argument");
    else a = make_accum_rays(ctx, params, d_rays, false, stream, &code);
    if (err) *err = code;
    return a;
}

pt_accum* pt_accum_create_rays(pt_ctx* ctx, const pt_params* params, const float* rays, int* err)
{
    pt::clear_error();
    int code;
    pt_accum* a = nullptr;
    if (!ctx || !params || !rays) code = pt::fail(PT_E_INVALID, "pt_accum_create_rays: null argument");
    else a = make_accum_rays(ctx, params, rays, true, nullptr, &code);
    if (err) *err = code;
    return a;
}

int pt_accum_has_rays(const pt_accum* acc) { return (acc && acc->d_rays && !acc->points) ? 1 : 0; }

pt_accum* pt_accum_create_points_device(pt_ctx* ctx, const pt_params* params, const float* d_points, void* stream, int* err)
{
    pt::clear_error();
    int code;
    pt_accum* a = nullptr;
    if (!ctx || !params || !d_points) code = pt::fail(PT_E_INVALID, "pt_accum_create_points: null argument");
    else a = make_accum_rays(ctx, params, d_points, false, stream, &code, true);
    if (err) *err = code;
    return a;
}

pt_accum* pt_accum_create_points(pt_ctx* ctx, const pt_params* params, const float* points, int* err)
{
    pt::clear_error();
    int code;
    pt_accum* a = nullptr;
    if (!ctx || !params || !points) code = pt::fail(PT_E_INVALID, "pt_accum_create_points: null argument");
    else a = make_accum_rays(ctx, params, points, true, nullptr, &code, true);
    if (err) *err = code;
    return a;
}

int pt_accum_has_points(const pt_accum* acc) { return (acc && acc->d_rays && acc->points) ? 1 : 0; }

int pt_accum_view(const pt_accum* acc, pt_view* out, int* has_view)
{
    pt::clear_error();
    if (!acc) return pt::fail(PT_E_INVALID, "pt_accum_view: null accumulator");
    if (has_view) *has_view = acc->has_view ? 1 : 0;
    if (out && acc->has_view) *out = acc->view;
    return PT_OK;
}

int pt_accum_add(pt_accum* acc, int32_t spp, float* d_out, void* stream, pt_stats* stats)
{
    pt::clear_error();
    if (!acc) return pt::fail(PT_E_INVALID, "pt_accum_add: null accumulator");
    if (spp < 0) return pt::fail(PT_E_INVALID, "pt_accum_add: spp < 0");
    if (pt::ctx_in_flight(acc->ctx) > 0)
        return pt::fail(PT_E_INVALID, "pt_accum_add: %d asynchronous renders in flight (pt_render_wait first)",
                        pt::ctx_in_flight(acc->ctx));
    if (acc->samples + (int64_t)spp > (int64_t)pt::accum_max_samples())
        return pt::fail(PT_E_INVALID, "pt_accum_add: %lld + %d samples exceed what a unit word carries (%u; bit 31 of a "
                        "unit's first sample number is the lens flag, bit 30 marks the pixel's first unit of a pass)",
                        (long long)acc->samples, spp, pt::accum_max_samples());
    if (spp == 0) {
        if (stats) memset(stats, 0, sizeof(*stats));
        return PT_OK;
    }
    pt_params p = acc->params;
    p.spp = spp;
    pt::AccumPass pass{(uint32_t)acc->samples, acc->d_rng, acc->d_mean};
    pass.rays = acc->d_rays;
    pass.points = acc->points;
    if (acc->any_frozen) {   // an adaptive pass: the active pixels only
        if (int rc = active_list(acc, stream)) return rc;
        if (acc->nactive == 0) {   // every pixel frozen: nothing to sample, the count stays
            if (stats) memset(stats, 0, sizeof(*stats));
            return PT_OK;
        }
        pass.active = acc->d_list;
        pass.nactive = acc->nactive;
    }
    if (int rc = pt::accum_pass(acc->ctx, &p, &acc->cam, acc->has_view ? &acc->view : nullptr, pass, d_out, stream, stats)) return rc;
    acc->samples += spp;
    return PT_OK;
}

int64_t pt_accum_samples(const pt_accum* acc) { return acc ? acc->samples : 0; }

int pt_accum_add_until(pt_accum* acc, pt_noise* noise, const pt_converge_params* cp, float* d_out, void* stream,
                       pt_converge_result* result)
{
    pt::clear_error();
    if (!acc || !noise || !cp || !result) return pt::fail(PT_E_INVALID, "pt_accum_add_until: null argument");
    if (acc->noise != noise) return pt::fail(PT_E_INVALID, "pt_accum_add_until: the estimator belongs to another accumulator");
    if (cp->pass_spp < 1) return pt::fail(PT_E_INVALID, "pt_accum_add_until: pass_spp %d < 1", cp->pass_spp);
    if (!(cp->quantile > 0.0f && cp->quantile <= 1.0f)) return pt::fail(PT_E_INVALID, "pt_accum_add_until: quantile must be in (0, 1]");
    if (cp->min_batches < 2) return pt::fail(PT_E_INVALID, "pt_accum_add_until: min_batches %d < 2", cp->min_batches);
    if (cp->max_samples < 0 || (int64_t)cp->max_samples > (int64_t)pt::accum_max_samples())
        return pt::fail(PT_E_INVALID, "pt_accum_add_until: max_samples %d outside 0..%u", cp->max_samples, pt::accum_max_samples());
    memset(result, 0, sizeof(*result));
    while (acc->samples < (int64_t)cp->max_samples) {
        const int64_t left = (int64_t)cp->max_samples - acc->samples;
        if (int rc = pt_accum_add(acc, left < cp->pass_spp ? (int32_t)left : cp->pass_spp, d_out, stream, nullptr)) return rc;
        if (int rc = pt_noise_update(noise, &cp->noise, stream, &result->last)) return rc;
        ++result->passes;
        const pt_noise_summary& s = result->last;
        if (s.batches >= cp->min_batches && s.converged >= (uint64_t)ceil((double)cp->quantile * (double)s.pixels)) {
            result->stopped_converged = 1;
            return PT_OK;
        }
    }
    if (result->passes == 0) return pt_noise_update(noise, &cp->noise, stream, &result->last);
    return PT_OK;
}

int pt_accum_freeze(pt_accum* acc, const uint8_t* mask)
{
    pt::clear_error();
    if (!acc || !mask) return pt::fail(PT_E_INVALID, "pt_accum_freeze: null argument");
    if (pt::ctx_in_flight(acc->ctx) > 0)
        return pt::fail(PT_E_INVALID, "pt_accum_freeze: %d asynchronous renders in flight (pt_render_wait first)",
                        pt::ctx_in_flight(acc->ctx));
    const size_t n = acc->slots();
    bool any = false;
    for (size_t q = 0; q < n && !any; ++q)
        any = acc->slot_pix[q] != 0xffffffffu && mask[order_index(acc, acc->slot_pix[q])] != 0;
    if (!any) return PT_OK;   // (nothing of this shard named: the accumulator stays as it is)
    if (int rc = adaptive_alloc(acc)) return rc;
    std::vector<uint32_t> at(n);
    HIP_TRY(hipSetDevice(pt::ctx_device(acc->ctx)));
    HIP_TRY(hipMemcpy(at.data(), acc->d_frozen_at, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t newly = 0;
    for (size_t q = 0; q < n; ++q) {
        if (acc->slot_pix[q] == 0xffffffffu || at[q] != pt::kSlotActive || !mask[order_index(acc, acc->slot_pix[q])]) continue;
        at[q] = (uint32_t)acc->samples;
        ++newly;
    }
    if (!newly) return PT_OK;
    HIP_TRY(hipMemcpy(acc->d_frozen_at, at.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    pt::accum_frozen(acc, newly);
    return PT_OK;
}

int pt_accum_counts(pt_accum* acc, uint32_t* out)
{
    pt::clear_error();
    if (!acc || !out) return pt::fail(PT_E_INVALID, "pt_accum_counts: null argument");
    std::vector<uint32_t> cnt;
    if (int rc = fetch_counts(acc, &cnt)) return rc;
    memset(out, 0, (size_t)acc->params.width * (size_t)acc->params.height * sizeof(uint32_t));
    for (size_t q = 0; q < acc->slots(); ++q)
        if (acc->slot_pix[q] != 0xffffffffu) out[order_index(acc, acc->slot_pix[q])] = cnt[q];
    return PT_OK;
}

int pt_accum_active(pt_accum* acc, uint32_t* out, uint32_t cap, uint64_t* n_out)
{
    pt::clear_error();
    if (!acc || !n_out) return pt::fail(PT_E_INVALID, "pt_accum_active: null argument");
    if (pt::ctx_in_flight(acc->ctx) > 0)
        return pt::fail(PT_E_INVALID, "pt_accum_active: %d asynchronous renders in flight (pt_render_wait first)",
                        pt::ctx_in_flight(acc->ctx));
    if (int rc = active_list(acc, nullptr)) return rc;
    *n_out = acc->nactive;
    if (!out) return PT_OK;
    if (cap < acc->nactive) return pt::fail(PT_E_INVALID, "pt_accum_active: buffer of %u entries too small for %u", cap, acc->nactive);
    std::vector<uint32_t> list(acc->nactive);
    if (acc->nactive) HIP_TRY(hipMemcpy(list.data(), acc->d_list, list.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t u = 0; u < list.size(); ++u) {
        if (list[u] >= acc->slots()) return pt::fail(PT_E_HIP, "pt_accum_active: the device list names slot %u of %zu", list[u], acc->slots());
        out[u] = acc->slot_pix[list[u]];
    }
    return PT_OK;
}

int pt_accum_add_adaptive(pt_accum* acc, pt_noise* noise, const pt_converge_params* cp, float* d_out, void* stream,
                          pt_adaptive_result* result)
{
    pt::clear_error();
    if (!acc || !noise || !cp || !result) return pt::fail(PT_E_INVALID, "pt_accum_add_adaptive: null argument");
    if (acc->noise != noise) return pt::fail(PT_E_INVALID, "pt_accum_add_adaptive: the estimator belongs to another accumulator");
    if (cp->pass_spp < 1) return pt::fail(PT_E_INVALID, "pt_accum_add_adaptive: pass_spp %d < 1", cp->pass_spp);
    if (!(cp->quantile > 0.0f && cp->quantile <= 1.0f)) return pt::fail(PT_E_INVALID, "pt_accum_add_adaptive: quantile must be in (0, 1]");
    if (cp->min_batches < 2) return pt::fail(PT_E_INVALID, "pt_accum_add_adaptive: min_batches %d < 2", cp->min_batches);
    if (cp->max_samples < 0 || (int64_t)cp->max_samples > (int64_t)pt::accum_max_samples())
        return pt::fail(PT_E_INVALID, "pt_accum_add_adaptive: max_samples %d outside 0..%u", cp->max_samples, pt::accum_max_samples());
    memset(result, 0, sizeof(*result));
    uint64_t active = acc->pixels;
    if (acc->any_frozen) {
        if (int rc = active_list(acc, stream)) return rc;
        active = acc->nactive;
    }
    while (acc->samples < (int64_t)cp->max_samples && active > 0) {
        const int64_t left = (int64_t)cp->max_samples - acc->samples;
        if (int rc = pt_accum_add(acc, left < cp->pass_spp ? (int32_t)left : cp->pass_spp, d_out, stream, nullptr)) return rc;
        if (int rc = pt_noise_update(noise, &cp->noise, stream, &result->last)) return rc;
        ++result->passes;
        const pt_noise_summary& s = result->last;
        if (s.batches < cp->min_batches) continue;
        uint64_t newly = 0;
        if (int rc = pt_noise_freeze(noise, &cp->noise, stream, &newly, &active)) return rc;
        if (active == 0 || s.converged >= (uint64_t)ceil((double)cp->quantile * (double)s.pixels)) {
            result->stopped_converged = 1;
            break;
        }
    }
    if (result->passes == 0) {
        if (int rc = pt_noise_update(noise, &cp->noise, stream, &result->last)) return rc;
        if (active == 0) result->stopped_converged = 1;
    }
    std::vector<uint32_t> cnt;
    if (int rc = fetch_counts(acc, &cnt)) return rc;
    result->active = active;
    for (const uint32_t c : cnt) result->samples_total += c;
    return PT_OK;
}

int pt_accum_read(pt_accum* acc, float* out_rgb, double* out_mean)
{
    pt::clear_error();
    if (!acc) return pt::fail(PT_E_INVALID, "pt_accum_read: null accumulator");
    std::vector<Record> rec;
    if (int rc = fetch_records(acc, &rec)) return rc;
    const uint32_t w = (uint32_t)acc->params.width, h = (uint32_t)acc->params.height;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const Record& r = rec[(size_t)y * w + x];
            const size_t o = (acc->params.pixel_order == PT_ORDER_MORTON) ? (size_t)pt_morton_pxl_to_i(x, y) : (size_t)y * w + x;
            for (int k = 0; k < 3; ++k) {
                if (out_mean) out_mean[o * 3 + k] = r.mean[k];
                if (out_rgb) out_rgb[o * 3 + k] = (float)r.mean[k];   // the render kernels' own conversion
            }
        }
    return PT_OK;
}

int pt_accum_save(pt_accum* acc, const char* path)
{
    pt::clear_error();
    if (!acc || !path) return pt::fail(PT_E_INVALID, "pt_accum_save: null argument");
    if (!little_endian()) return pt::fail(PT_E_INVALID, "pt_accum_save: checkpoint files are little-endian; this host is not");
    if (acc->d_rays && acc->points)
        return pt::fail(PT_E_INVALID, "pt_accum_save: the accumulator was built over a point buffer (pt_accum_create_points); a "
                        "checkpoint file holds a camera, not points");
    if (acc->d_rays)
        return pt::fail(PT_E_INVALID, "pt_accum_save: the accumulator was built over a ray buffer (pt_accum_create_rays); a "
                        "checkpoint file holds a camera, not rays");
    if (acc->has_view)
        return pt::fail(PT_E_INVALID, "pt_accum_save: the accumulator has a view (an oriented camera); checkpoint format version 1 "
                        "holds the 32-byte camera alone (pt_session_save writes a session file that holds the view)");
    if (acc->any_frozen) {
        std::vector<uint32_t> cnt;
        if (int rc = fetch_counts(acc, &cnt)) return rc;
        for (size_t q = 0; q < cnt.size(); ++q)
            if (acc->slot_pix[q] != 0xffffffffu && (int64_t)cnt[q] != acc->samples)
                return pt::fail(PT_E_INVALID, "pt_accum_save: the pixels' sample counts differ (frozen pixels stopped before %lld); "
                                "checkpoint format version 1 holds a single sample count", (long long)acc->samples);
    }
    pt::StageTimer timer{"pt_accum_save"};
    std::vector<Record> rec;
    if (int rc = fetch_records(acc, &rec)) return rc;
    timer.lap("state to host");
    Header h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, kMagic, 8);
    h.version = kVersion;
    h.header_bytes = (uint32_t)sizeof(Header);
    h.params = acc->params;
    h.cam = acc->cam;
    h.samples = acc->samples;
    pt::ctx_scene_id(acc->ctx, &h.scene_digest, &h.num_tris, &h.num_spheres);
    FILE* f = fopen(path, "wb");
    if (!f) return pt::fail(PT_E_IO, "pt_accum_save: cannot open %s for writing", path);
    const bool ok = fwrite(&h, 1, sizeof(h), f) == sizeof(h) && fwrite(rec.data(), sizeof(Record), rec.size(), f) == rec.size();
    if (fclose(f) != 0 || !ok) return pt::fail(PT_E_IO, "pt_accum_save: short write to %s", path);
    timer.lap("file write");
    return PT_OK;
}

pt_accum* pt_accum_load(pt_ctx* ctx, const char* path, int* err)
{
    pt::clear_error();
    auto bail = [&](int code) -> pt_accum* { if (err) *err = code; return nullptr; };
    if (!ctx || !path) return bail(pt::fail(PT_E_INVALID, "pt_accum_load: null argument"));
    pt::StageTimer timer{"pt_accum_load"};
    Header h;
    FILE* f = nullptr;
    if (int rc = read_header("pt_accum_load", path, &h, &f)) return bail(rc);
    std::vector<Record> rec((size_t)h.params.width * h.params.height);
    const bool got = fread(rec.data(), sizeof(Record), rec.size(), f) == rec.size();
    fclose(f);
    if (!got) return bail(pt::fail(PT_E_IO, "pt_accum_load: cannot read the records of %s", path));
    timer.lap("file read");
    uint64_t digest;
    uint32_t nt, ns;
    pt::ctx_scene_id(ctx, &digest, &nt, &ns);
    if (digest != h.scene_digest || nt != h.num_tris || ns != h.num_spheres)
        return bail(pt::fail(PT_E_SCENE, "pt_accum_load: %s was written for another scene (%u triangles, %u spheres, digest "
                             "%016llx; this context: %u, %u, %016llx)", path, h.num_tris, h.num_spheres,
                             (unsigned long long)h.scene_digest, nt, ns, (unsigned long long)digest));
    int code;
    pt_accum* a = make_accum(ctx, &h.params, &h.cam, nullptr, &code);
    if (!a) return bail(code);
    const size_t n = a->slots();
    std::vector<uint32_t> rng(n * 6, 0u);
    std::vector<double> mean(n * 3, 0.0);
    for (size_t q = 0; q < n; ++q) {
        const uint32_t pix = a->slot_pix[q];
        if (pix == 0xffffffffu) continue;
        for (int k = 0; k < 6; ++k) rng[(size_t)k * n + q] = rec[pix].rng[k];
        for (int k = 0; k < 3; ++k) mean[(size_t)k * n + q] = rec[pix].mean[k];
    }
    auto upload = [&]() -> int {
        if (!n) return PT_OK;
        HIP_TRY(hipMemcpy(a->d_rng, rng.data(), n * 6 * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(a->d_mean, mean.data(), n * 3 * sizeof(double), hipMemcpyHostToDevice));
        return PT_OK;
    };
    if (int rc = upload()) { pt_accum_destroy(a); return bail(rc); }
    a->samples = h.samples;
    timer.lap("host to state");
    if (err) *err = PT_OK;
    return a;
}

int pt_accum_file_info(const char* path, pt_params* params, pt_camera* cam, int64_t* samples, uint64_t* scene_digest)
{
    pt::clear_error();
    if (!path) return pt::fail(PT_E_INVALID, "pt_accum_file_info: null path");
    Header h;
    if (int rc = read_header("pt_accum_file_info", path, &h, nullptr)) return rc;
    if (params) *params = h.params;
    if (cam) *cam = h.cam;
    if (samples) *samples = h.samples;
    if (scene_digest) *scene_digest = h.scene_digest;
    return PT_OK;
}

void pt_accum_destroy(pt_accum* acc)
{
    if (!acc) return;
    (void)hipSetDevice(pt::ctx_device(acc->ctx));
    if (acc->d_rng) (void)hipFree(acc->d_rng);
    if (acc->d_mean) (void)hipFree(acc->d_mean);
    if (acc->d_frozen_at) (void)hipFree(acc->d_frozen_at);
    if (acc->d_list) (void)hipFree(acc->d_list);
    if (acc->d_scan) (void)hipFree(acc->d_scan);
    if (acc->d_slot_pix) (void)hipFree(acc->d_slot_pix);
    if (acc->d_rays) (void)hipFree(acc->d_rays);
    delete acc;
}

}  // extern "C"
