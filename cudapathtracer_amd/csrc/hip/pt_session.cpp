// pt_session.cpp -- session files (include/pt/pt.h, pt_session_*): the whole progressive state of one shard -- the
// accumulator, the per-pixel frozen-at counts and the attached noise estimator -- written to and read from one file,
// so that an adaptive or until-error render continues in another process exactly as if it had never stopped.
// Host code over the HIP runtime: the file's sections are laid out on the device by pt_session.hip's pack / unpack
// kernels and cross PCIe in one copy through a pinned staging buffer that the context owns; nothing here loops
// over pixels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../host/host_internal.h"
#include "pt_hip_util.h"

namespace {

// The session header (documented in pt.h); every field little-endian at a fixed offset.  Bytes 0..127 are the
// checkpoint header of format version 1.
constexpr char kMagic[8] = {'P', 'T', 'A', 'C', 'C', 'U', 'M', '\0'};
constexpr uint32_t kVersion = 2;        // without a view: byte for byte the format it always was
constexpr uint32_t kVersionView = 3;    // with a view: version 2's 192 bytes, then the 64-byte ViewTail
constexpr uint32_t kCounts = 0x1u, kNoise = 0x2u, kNoisePerPixel = 0x4u;
constexpr size_t kBytesA = 48, kBytesB = 4, kBytesC = 40, kBytesD = 8;
struct Header {
    char magic[8];
    uint32_t version;
    uint32_t header_bytes;
    pt_params params;        // 56 B: spp = 0, the 4 bytes of tail padding 0
    pt_camera cam;           // 32 B
    int64_t samples;
    uint64_t scene_digest;
    uint32_t num_tris, num_spheres;
    uint32_t flags;
    uint32_t zero0;
    int64_t noise_n0;
    double noise_W;
    int32_t noise_batches;
    uint32_t zero1;
    uint64_t frozen_pixels;
    unsigned char zero2[24];
};
// Format version 3's header is version 2's, then this: the file is recognised by its version and header size together.
struct ViewTail {
    pt_view view;            // 44 B at 192
    unsigned char zero[20];
};
static_assert(sizeof(ViewTail) == 64, "the view's part of a version-3 header is 64 B");
constexpr size_t kHeaderView = sizeof(Header) + sizeof(ViewTail);   // 256
static_assert(sizeof(pt_params) == 56, "pt_params is 56 B in the session header");
static_assert(sizeof(Header) == 192, "session header is 192 B");
static_assert(offsetof(Header, flags) == 128 && offsetof(Header, noise_n0) == 136 && offsetof(Header, noise_batches) == 152 &&
              offsetof(Header, frozen_pixels) == 160, "session header offsets");

bool little_endian()
{
    const uint32_t one = 1;
    unsigned char b;
    memcpy(&b, &one, 1);
    return b == 1;
}

size_t file_bytes(const Header& h)
{
    const size_t n = (size_t)h.params.width * (size_t)h.params.height;
    return (size_t)h.header_bytes + n * (kBytesA + ((h.flags & kCounts) ? kBytesB : 0) + ((h.flags & kNoise) ? kBytesC : 0) +
                                 ((h.flags & kNoisePerPixel) ? kBytesD : 0));
}

// Reads and validates the header of `path` and the file's size; *keep: the file, positioned at the sections.
// *has_view: the file is format version 3, and *view its (validated) view.
int read_header(const char* what, const char* path, Header* h, pt_view* view, bool* has_view, FILE** keep)
{
    *has_view = false;
    if (!little_endian()) return pt::fail(PT_E_INVALID, "%s: session files are little-endian; this host is not", what);
    FILE* f = fopen(path, "rb");
    if (!f) return pt::fail(PT_E_IO, "%s: cannot open %s", what, path);
    auto bail = [&](int code) { fclose(f); return code; };
    if (fread(h, 1, 16, f) != 16) return bail(pt::fail(PT_E_IO, "%s: %s is shorter than a header", what, path));
    if (memcmp(h->magic, kMagic, 8) != 0) return bail(pt::fail(PT_E_INVALID, "%s: %s is not a session file (bad magic)", what, path));
    if (h->version != kVersion && h->version != kVersionView)
        return bail(pt::fail(PT_E_INVALID, "%s: %s has format version %u, a session file has %u (or %u with a view)%s", what, path,
                             h->version, kVersion, kVersionView, h->version == 1 ? " (a version-1 checkpoint: pt_accum_load reads it)" : ""));
    const size_t header_want = h->version == kVersionView ? kHeaderView : sizeof(Header);
    if (h->header_bytes != header_want)
        return bail(pt::fail(PT_E_INVALID, "%s: %s has a %u-byte header, format version %u has %zu", what, path, h->header_bytes,
                             h->version, header_want));
    if (fread(reinterpret_cast<char*>(h) + 16, 1, sizeof(Header) - 16, f) != sizeof(Header) - 16)
        return bail(pt::fail(PT_E_IO, "%s: %s is shorter than the %zu-byte header", what, path, sizeof(Header)));
    if (h->version == kVersionView) {
        ViewTail t;
        if (fread(&t, 1, sizeof(t), f) != sizeof(t))
            return bail(pt::fail(PT_E_IO, "%s: %s is truncated inside the %zu-byte header (the view)", what, path, kHeaderView));
        for (const unsigned char z : t.zero)
            if (z) return bail(pt::fail(PT_E_INVALID, "%s: %s has a non-zero byte in the reserved bytes 236..255 of its header", what, path));
        const std::string who = std::string(what) + ": " + path;
        if (int rc = pt::validate_view(who.c_str(), &t.view)) return bail(rc);
        *view = t.view;
        *has_view = true;
    }
    const pt_params& p = h->params;
    if (p.width <= 0 || p.height <= 0 || p.width > 65535 || p.height > 65535 || h->samples < 0 ||
        h->samples > (int64_t)pt::accum_max_samples())
        return bail(pt::fail(PT_E_INVALID, "%s: %s: image %dx%d with %lld samples is out of range", what, path, p.width, p.height,
                             (long long)h->samples));
    if (h->flags & ~(kCounts | kNoise | kNoisePerPixel))
        return bail(pt::fail(PT_E_INVALID, "%s: %s has unknown flag bits (flags 0x%x)", what, path, h->flags));
    if ((h->flags & kNoisePerPixel) && !(h->flags & kNoise))
        return bail(pt::fail(PT_E_INVALID, "%s: %s has per-pixel estimator planes (flag 0x4) without an estimator (0x2)", what, path));
    // (an estimator's planes carry the state only once its accumulator has a frozen pixel: the per-pixel kernels
    // read the frozen-at plane)
    if ((h->flags & kNoisePerPixel) && !(h->flags & kCounts))
        return bail(pt::fail(PT_E_INVALID, "%s: %s has per-pixel estimator planes (flag 0x4) without frozen-at counts (0x1)", what, path));
    if (h->noise_batches < 0) return bail(pt::fail(PT_E_INVALID, "%s: %s: noise batches %d < 0", what, path, h->noise_batches));
    if (h->noise_n0 < 0 || h->noise_n0 > h->samples)
        return bail(pt::fail(PT_E_INVALID, "%s: %s: noise n0 %lld outside 0..%lld", what, path, (long long)h->noise_n0, (long long)h->samples));
    if (!(h->noise_W >= 0.0 && h->noise_W <= (double)h->samples))   // (the samples folded: NaN fails too)
        return bail(pt::fail(PT_E_INVALID, "%s: %s: noise W %g outside 0..%lld", what, path, h->noise_W, (long long)h->samples));
    const uint64_t npix = (uint64_t)p.width * (uint64_t)p.height;
    if (h->frozen_pixels > npix || (!(h->flags & kCounts) && h->frozen_pixels))
        return bail(pt::fail(PT_E_INVALID, "%s: %s: %llu frozen pixels disagree with the file's sections", what, path,
                             (unsigned long long)h->frozen_pixels));
    if (fseek(f, 0, SEEK_END) != 0) return bail(pt::fail(PT_E_IO, "%s: cannot seek in %s", what, path));
    const long long size = ftell(f), want = (long long)file_bytes(*h);
    if (size < want)
        return bail(pt::fail(PT_E_IO, "%s: %s is truncated: %lld bytes, its %dx%d sections need %lld", what, path, size, p.width, p.height, want));
    if (size > want)
        return bail(pt::fail(PT_E_INVALID, "%s: %s has %lld bytes, its %dx%d sections make %lld", what, path, size, p.width, p.height, want));
    if (keep) {
        if (fseek(f, (long)h->header_bytes, SEEK_SET) != 0) return bail(pt::fail(PT_E_IO, "%s: cannot seek in %s", what, path));
        *keep = f;
    } else {
        fclose(f);
    }
    return PT_OK;
}

// The staging's layout for an image of npix pixels with these sections.
pt::SessionLayout layout_of(size_t npix, bool b, bool c, bool d)
{
    pt::SessionLayout at;
    size_t end = pt::kSessionSumBytes;
    auto place = [&](bool have, size_t record) -> size_t {
        if (!have) return 0;
        const size_t off = (end + 255) & ~(size_t)255;
        end = off + npix * record;
        return off;
    };
    at.a = place(true, kBytesA);
    at.b = place(b, kBytesB);
    at.c = place(c, kBytesC);
    at.d = place(d, kBytesD);
    at.bytes = end;
    return at;
}

// The context's staging, at least `bytes` on both sides.
int grow(const char* who, pt::SessionScratch* S, size_t bytes)
{
    if (S->bytes >= bytes) return PT_OK;
    if (S->dev) (void)hipFree(S->dev);
    pt::free_pinned(S->host);
    S->dev = S->host = nullptr;
    S->bytes = 0;
    if (hipMalloc(&S->dev, bytes) != hipSuccess || hipHostMalloc(&S->host, bytes, hipHostMallocDefault) != hipSuccess) {
        if (S->dev) (void)hipFree(S->dev);
        S->dev = S->host = nullptr;
        (void)hipGetLastError();
        return pt::fail(PT_E_OOM, "%s: cannot allocate %zu bytes of staging (device + pinned host)", who, bytes);
    }
    S->bytes = bytes;
    return PT_OK;
}

void sum_counters(const void* host_stage, uint64_t* frozen, uint64_t* bad)
{
    const unsigned long long* part = static_cast<const unsigned long long*>(host_stage);
    *frozen = *bad = 0;
    for (int c = 0; c < pt::kSessionSumCopies; ++c) {
        *frozen += part[c * pt::kSessionSumWords];
        *bad += part[c * pt::kSessionSumWords + 1];
    }
}

}  // namespace

extern "C" {

int pt_session_save(pt_accum* acc, pt_noise* noise, const char* path)
{
    pt::clear_error();
    if (!acc || !path) return pt::fail(PT_E_INVALID, "pt_session_save: null argument");
    if (!little_endian()) return pt::fail(PT_E_INVALID, "pt_session_save: session files are little-endian; this host is not");
    if (pt_accum_has_rays(acc))
        return pt::fail(PT_E_INVALID, "pt_session_save: the accumulator was built over a ray buffer (pt_accum_create_rays); a "
                        "session file holds a camera, not rays");
    if (pt_accum_has_points(acc))
        return pt::fail(PT_E_INVALID, "pt_session_save: the accumulator was built over a point buffer (pt_accum_create_points); a "
                        "session file holds a camera, not points");
    pt::StageTimer timer{"pt_session_save"};
    const pt::AccumView view = pt::accum_view(acc);
    if (noise && noise != *view.noise) return pt::fail(PT_E_INVALID, "pt_session_save: the estimator is not this accumulator's live estimator");
    if (pt::ctx_in_flight(view.ctx) > 0)
        return pt::fail(PT_E_INVALID, "pt_session_save: %d asynchronous renders in flight (pt_render_wait first)", pt::ctx_in_flight(view.ctx));
    pt::SessionAccum sa;
    if (int rc = pt::accum_session(acc, &sa)) return rc;
    pt::SessionNoise sn{};
    if (noise) pt::noise_session(noise, &sn);
    Header h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, kMagic, 8);
    h.version = sa.view ? kVersionView : kVersion;
    h.header_bytes = (uint32_t)(sa.view ? kHeaderView : sizeof(Header));
    ViewTail tail;
    memset(&tail, 0, sizeof(tail));
    if (sa.view) tail.view = *sa.view;
    h.params = *sa.params;
    h.cam = *sa.cam;
    h.samples = sa.samples;
    pt::ctx_scene_id(sa.ctx, &h.scene_digest, &h.num_tris, &h.num_spheres);
    h.flags = (sa.frozen_at ? kCounts : 0u) | (noise ? kNoise : 0u) | (sn.pix ? kNoisePerPixel : 0u);
    if (noise) {
        h.noise_n0 = sn.n0;
        h.noise_W = sn.W;
        h.noise_batches = sn.batches;
    }
    const size_t npix = (size_t)sa.params->width * (size_t)sa.params->height;
    pt::SessionPlanes pl{};
    pl.rng = sa.rng; pl.mean = sa.mean; pl.frozen_at = sa.frozen_at; pl.nstate = sn.state; pl.npix = sn.pix;
    pl.slot_pix = sa.slot_pix;
    pl.at = layout_of(npix, sa.frozen_at != nullptr, noise != nullptr, sn.pix != nullptr);
    pl.slots = sa.slots; pl.image_pixels = npix; pl.samples = (uint32_t)sa.samples;
    HIP_TRY(hipSetDevice(pt::ctx_device(sa.ctx)));
    pt::SessionScratch* S = pt::ctx_session_scratch(sa.ctx);
    if (int rc = grow("pt_session_save", S, pl.at.bytes)) return rc;
    pl.stage = static_cast<unsigned char*>(S->dev);
    if (sa.slots) {
        // the counters, and every pixel of another shard when there are any: the kernel writes this shard's only
        HIP_TRY(hipMemsetAsync(S->dev, 0, sa.pixels == npix ? pt::kSessionSumBytes : pl.at.bytes, nullptr));
        if (int rc = pt::session_pack(sa.ctx, pl, nullptr)) return rc;
        HIP_TRY(hipMemcpyAsync(S->host, S->dev, pl.at.bytes, hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
    } else {
        memset(S->host, 0, pl.at.bytes);   // (a shard that owns no pixel: nothing is launched)
    }
    timer.lap("state to host");
    uint64_t bad = 0;
    sum_counters(S->host, &h.frozen_pixels, &bad);
    FILE* f = fopen(path, "wb");
    if (!f) return pt::fail(PT_E_IO, "pt_session_save: cannot open %s for writing", path);
    const char* host = static_cast<const char*>(S->host);
    bool ok = fwrite(&h, 1, sizeof(h), f) == sizeof(h) && (!sa.view || fwrite(&tail, 1, sizeof(tail), f) == sizeof(tail)) &&
              fwrite(host + pl.at.a, kBytesA, npix, f) == npix;
    if (ok && (h.flags & kCounts)) ok = fwrite(host + pl.at.b, kBytesB, npix, f) == npix;
    if (ok && (h.flags & kNoise)) ok = fwrite(host + pl.at.c, kBytesC, npix, f) == npix;
    if (ok && (h.flags & kNoisePerPixel)) ok = fwrite(host + pl.at.d, kBytesD, npix, f) == npix;
    if (fclose(f) != 0 || !ok) return pt::fail(PT_E_IO, "pt_session_save: short write to %s", path);
    timer.lap("file write");
    return PT_OK;
}

int pt_session_load(pt_ctx* ctx, const char* path, pt_accum** acc_out, pt_noise** noise_out, int* has_noise)
{
    pt::clear_error();
    if (acc_out) *acc_out = nullptr;
    if (noise_out) *noise_out = nullptr;
    if (has_noise) *has_noise = 0;
    if (!ctx || !path || !acc_out) return pt::fail(PT_E_INVALID, "pt_session_load: null argument");
    if (pt::ctx_in_flight(ctx) > 0)
        return pt::fail(PT_E_INVALID, "pt_session_load: %d asynchronous renders in flight (pt_render_wait first)", pt::ctx_in_flight(ctx));
    pt::StageTimer timer{"pt_session_load"};
    Header h;
    pt_view view;
    bool has_view = false;
    FILE* f = nullptr;
    if (int rc = read_header("pt_session_load", path, &h, &view, &has_view, &f)) return rc;
    auto bail = [&](int code) { fclose(f); return code; };
    uint64_t digest;
    uint32_t nt, ns;
    pt::ctx_scene_id(ctx, &digest, &nt, &ns);
    if (digest != h.scene_digest || nt != h.num_tris || ns != h.num_spheres)
        return bail(pt::fail(PT_E_SCENE, "pt_session_load: %s was written for another scene (%u triangles, %u spheres, digest "
                             "%016llx; this context: %u, %u, %016llx)", path, h.num_tris, h.num_spheres,
                             (unsigned long long)h.scene_digest, nt, ns, (unsigned long long)digest));
    const bool counts = (h.flags & kCounts) != 0;
    const bool take = (h.flags & kNoise) && noise_out;                   // (else the estimator's sections are skipped)
    const bool per_pixel = take && (h.flags & kNoisePerPixel);
    const size_t npix = (size_t)h.params.width * (size_t)h.params.height;
    pt::SessionPlanes pl{};
    pl.at = layout_of(npix, counts, take, per_pixel);
    if (hipSetDevice(pt::ctx_device(ctx)) != hipSuccess) return bail(pt::fail(PT_E_HIP, "pt_session_load: hipSetDevice failed"));
    pt::SessionScratch* S = pt::ctx_session_scratch(ctx);
    if (int rc = grow("pt_session_load", S, pl.at.bytes)) return bail(rc);
    char* host = static_cast<char*>(S->host);
    memset(host, 0, pt::kSessionSumBytes);
    bool got = fread(host + pl.at.a, kBytesA, npix, f) == npix;
    if (got && counts) got = fread(host + pl.at.b, kBytesB, npix, f) == npix;
    if (got && take) got = fread(host + pl.at.c, kBytesC, npix, f) == npix;
    if (got && per_pixel) got = fread(host + pl.at.d, kBytesD, npix, f) == npix;
    fclose(f);
    if (!got) return pt::fail(PT_E_IO, "pt_session_load: cannot read the sections of %s", path);
    timer.lap("file read");
    int code = PT_OK;
    // a refusal by the accumulator's or the estimator's own constructor, under this entry point's name
    auto renamed = [&](int rc) {
        const std::string why = pt_last_error();
        return pt::fail(rc, "pt_session_load: %s: %s", path, why.c_str());
    };
    pt_accum* acc = pt::accum_session_new(ctx, &h.params, &h.cam, has_view ? &view : nullptr, h.samples, counts, &code);
    if (!acc) return renamed(code);
    pt_noise* noise = nullptr;
    auto fill = [&]() -> int {
        pt::SessionAccum sa;
        if (int rc = pt::accum_session(acc, &sa)) return rc;
        pt::SessionNoise sn{};
        if (take) {
            noise = pt::noise_session_new(acc, h.noise_n0, h.noise_W, h.noise_batches, per_pixel, &code);
            if (!noise) return renamed(code);
            pt::noise_session(noise, &sn);
        }
        uint64_t frozen = 0, bad = 0;
        if (sa.slots) {
            pl.rng = sa.rng; pl.mean = sa.mean; pl.frozen_at = sa.frozen_at; pl.nstate = sn.state; pl.npix = sn.pix;
            pl.slot_pix = sa.slot_pix;
            pl.stage = static_cast<unsigned char*>(S->dev);
            pl.slots = sa.slots; pl.image_pixels = npix; pl.samples = (uint32_t)h.samples;
            HIP_TRY(hipMemcpyAsync(S->dev, S->host, pl.at.bytes, hipMemcpyHostToDevice, nullptr));
            if (int rc = pt::session_unpack(ctx, pl, nullptr)) return rc;
            HIP_TRY(hipMemcpyAsync(S->host, S->dev, pt::kSessionSumBytes, hipMemcpyDeviceToHost, nullptr));
            HIP_TRY(hipStreamSynchronize(nullptr));
            sum_counters(S->host, &frozen, &bad);
        }
        if (bad)
            return pt::fail(PT_E_INVALID, "pt_session_load: %s: %llu section-B words are neither 0xffffffff (active) nor a count <= %lld",
                            path, (unsigned long long)bad, (long long)h.samples);
        if (frozen != h.frozen_pixels)
            return pt::fail(PT_E_INVALID, "pt_session_load: %s: the header says %llu frozen pixels, section B holds %llu", path,
                            (unsigned long long)h.frozen_pixels, (unsigned long long)frozen);
        return PT_OK;
    };
    if (int rc = fill()) {
        pt_noise_destroy(noise);
        pt_accum_destroy(acc);
        return rc;
    }
    timer.lap("host to state");
    *acc_out = acc;
    if (noise_out) *noise_out = noise;
    if (has_noise) *has_noise = (h.flags & kNoise) ? 1 : 0;
    return PT_OK;
}

int pt_session_file_info(const char* path, pt_session_info* info)
{
    pt::clear_error();
    if (!path || !info) return pt::fail(PT_E_INVALID, "pt_session_file_info: null argument");
    Header h;
    pt_view view;
    bool has_view = false;
    if (int rc = read_header("pt_session_file_info", path, &h, &view, &has_view, nullptr)) return rc;
    memset(info, 0, sizeof(*info));
    info->params = h.params;
    info->cam = h.cam;
    info->samples = h.samples;
    info->scene_digest = h.scene_digest;
    info->flags = h.flags;
    info->noise_batches = h.noise_batches;
    info->noise_n0 = h.noise_n0;
    info->noise_W = h.noise_W;
    info->frozen_pixels = h.frozen_pixels;
    return PT_OK;
}

int pt_session_file_view(const char* path, pt_view* out, int* has_view_out)
{
    pt::clear_error();
    if (!path) return pt::fail(PT_E_INVALID, "pt_session_file_view: null path");
    Header h;
    pt_view view;
    bool has_view = false;
    if (int rc = read_header("pt_session_file_view", path, &h, &view, &has_view, nullptr)) return rc;
    if (has_view_out) *has_view_out = has_view ? 1 : 0;
    if (out && has_view) *out = view;
    return PT_OK;
}

}  // extern "C"
