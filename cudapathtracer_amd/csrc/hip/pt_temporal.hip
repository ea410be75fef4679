// pt_temporal.hip -- temporal reprojection (include/pt/pt.h, pt_temporal_*): a history of the image that follows a
// moving camera through the primary-hit feature buffers, for gfx950.  The arithmetic is the header's, operation by
// operation (f32, no contraction, IEEE division); tests/temporal_ref.py restates it in numpy and the kernel agrees
// with it in every bit.
//
// One kernel over two sets of planes, read one and write the other (scanline order, 56 B per pixel and set):
//   G0 = {P.xyz, prim}   G1 = {n.xyz, depth}   C = {r, g, b, n}   M = {m1, m2}
//   tp_push   one thread per pixel, consecutive lanes consecutive x: the pixel's own 60 B (12 B of `in`, 48 B of its
//             feature record as three 16-B loads) and its 72 B of stores (56 B of planes, 12 B of `out`, 4 B of `var`)
//             coalesce; it resolves the pixel order, projects position_p through the previous push's camera
//             (host/project_view.h, the function pt_project_view runs), gathers the four taps of the bilinear
//             footprint straight from the read planes (up to 4 x 56 B through L2 / TCP: for small camera moves they are
//             neighbours of the neighbouring lanes' taps), and folds the new frame in.  No atomics, no cross-lane
//             operations, no LDS, nothing of pt_render.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../host/host_internal.h"
#include "../host/project_view.h"
#include "pt_hip_util.h"

namespace {

static_assert(sizeof(pt_feature) == 48, "pt_feature is 48 B");

struct TpPlanes {
    float4* g0;
    float4* g1;
    float4* c;
    float2* m;
};

struct TpArgs {
    TpPlanes rd, wr;
    const float* in;
    const float4* feat;    // 3 per pixel
    float* out;
    float* var;            // may be null
    pt_camera prev_cam;
    pt_view prev_view;     // (the identity for a NULL view)
    float off_prev;
    float max_history;     // (float)max_history
    float normal_min, plane_tol;
    int32_t w, h;
    int32_t morton;
    int32_t first;         // the first push since create / reset: no pixel has a history
};

__device__ __forceinline__ uint32_t tp_morton(uint32_t x, uint32_t y)   // camera.h:66-75
{
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        r |= ((x >> b) & 1u) << (2 * b);
        r |= ((y >> b) & 1u) << (2 * b + 1);
    }
    return r;
}

__device__ __forceinline__ float tp_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// fx snapped to the nearest integer when it is within 1/64 pixel of it
__device__ __forceinline__ float tp_snap(float fx)
{
    const float r = floorf(fx + 0.5f);
    return (fabsf(fx - r) <= 0.015625f) ? r : fx;
}

__global__ __launch_bounds__(256) void tp_push(TpArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    const size_t s = a.morton ? (size_t)tp_morton((uint32_t)x, (uint32_t)y) : p;
    const float4 f0 = a.feat[s * 3], f1 = a.feat[s * 3 + 1], f2 = a.feat[s * 3 + 2];   // {albedo, depth} {n, prim} {P, -}
    const float in[3] = {a.in[s * 3], a.in[s * 3 + 1], a.in[s * 3 + 2]};
    const int32_t prim = __float_as_int(f1.w);
    const float depth = f0.w;

    float sx, sy;
    const bool front = pt::project_view(a.prev_cam, a.prev_view, f2.x, f2.y, f2.z, &sx, &sy);
    bool reset = a.first != 0 || prim < 0 || !front;
    const float fx = tp_snap(sx - a.off_prev), fy = tp_snap(sy - a.off_prev);
    reset = reset || !(fx > -1.0f && fx < (float)a.w) || !(fy > -1.0f && fy < (float)a.h);

    float ws = 0.0f, hc[3] = {0.0f, 0.0f, 0.0f}, hn = 0.0f, h1 = 0.0f, h2 = 0.0f;
    if (!reset) {   // fx in (-1, W), fy in (-1, H): the conversions below are in range
        const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
        const float tx = fx - (float)x0, ty = fy - (float)y0;
        const float lim = a.plane_tol * depth;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int xq = x0 + (t & 1), yq = y0 + (t >> 1);
            const float wx = (t & 1) ? tx : 1.0f - tx, wy = (t >> 1) ? ty : 1.0f - ty;
            const float w = wx * wy;
            if (xq < 0 || xq >= a.w || yq < 0 || yq >= a.h) continue;
            const size_t q = (size_t)yq * a.w + xq;
            // (all four loads before any test: the taps' 16 loads are in flight together)
            const float4 G0 = a.rd.g0[q];
            const float4 G1 = a.rd.g1[q];
            const float4 Cq = a.rd.c[q];
            const float2 Mq = a.rd.m[q];
            const float dn = (f1.x * G1.x + f1.y * G1.y) + f1.z * G1.z;
            const float e = (f1.x * (G0.x - f2.x) + f1.y * (G0.y - f2.y)) + f1.z * (G0.z - f2.z);
            if (__float_as_int(G0.w) < 0 || !(Cq.w > 0.0f) || !(dn >= a.normal_min) || !(fabsf(e) <= lim)) continue;
            ws = ws + w;
            hc[0] = hc[0] + w * Cq.x;
            hc[1] = hc[1] + w * Cq.y;
            hc[2] = hc[2] + w * Cq.z;
            hn = hn + w * Cq.w;
            h1 = h1 + w * Mq.x;
            h2 = h2 + w * Mq.y;
        }
    }
    if (ws > 0.0f && !reset) {
        hc[0] = hc[0] / ws; hc[1] = hc[1] / ws; hc[2] = hc[2] / ws;
        hn = hn / ws; h1 = h1 / ws; h2 = h2 / ws;
    } else {
        hc[0] = hc[1] = hc[2] = 0.0f;
        hn = h1 = h2 = 0.0f;
    }
    float n1 = hn + 1.0f;
    n1 = (n1 < a.max_history) ? n1 : a.max_history;
    const float al = 1.0f / n1;
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = hc[k] + (in[k] - hc[k]) * al;
    const float l = tp_luma(in[0], in[1], in[2]);
    const float m1 = h1 + (l - h1) * al;
    const float m2 = h2 + (l * l - h2) * al;
    if (a.var) {
        const float d = m2 - m1 * m1;
        a.var[s] = (n1 < 2.0f) ? INFINITY : ((d > 0.0f) ? d : 0.0f) / (n1 - 1.0f);
    }
    a.out[s * 3] = o[0];
    a.out[s * 3 + 1] = o[1];
    a.out[s * 3 + 2] = o[2];
    a.wr.g0[p] = make_float4(f2.x, f2.y, f2.z, f1.w);
    a.wr.g1[p] = make_float4(f1.x, f1.y, f1.z, depth);
    a.wr.c[p] = make_float4(o[0], o[1], o[2], n1);
    a.wr.m[p] = make_float2(m1, m2);
}

bool morton_ok(int w, int h) { return w == h && w > 0 && (w & (w - 1)) == 0; }

constexpr size_t kSetBytes = 3 * sizeof(float4) + sizeof(float2);   // 56 B per pixel and set

}  // namespace

struct pt_temporal {
    pt_ctx* ctx = nullptr;
    pt_temporal_params tp{};
    int w = 0, h = 0, order = PT_ORDER_SCANLINE;
    void* mem = nullptr;        // both sets of planes
    int cur = 0;                // the set the next push reads
    int frames = 0;
    pt_camera prev_cam{};
    pt_view prev_view{};
    float off_prev = 0.0f;
    // staging of the host variant, allocated on first use
    float* d_img = nullptr;
    pt_feature* d_feat = nullptr;
    float* d_var = nullptr;

    size_t pixels() const { return (size_t)w * (size_t)h; }
    TpPlanes set(int k) const
    {
        // the six 16-B planes of both sets first, then the two 8-B ones: every plane keeps its alignment for any W*H
        const size_t n = pixels();
        float4* const base = static_cast<float4*>(mem);
        TpPlanes pl;
        pl.g0 = base + (size_t)(3 * k) * n;
        pl.g1 = pl.g0 + n;
        pl.c = pl.g1 + n;
        pl.m = reinterpret_cast<float2*>(base + 6 * n) + (size_t)k * n;
        return pl;
    }
};

namespace {

int check_push(const char* who, const pt_temporal* t, const pt_camera* cam, const pt_view* view, const void* in, const void* feat,
               const void* out)
{
    if (!t || !cam || !in || !feat || !out) return pt::fail(PT_E_INVALID, "%s: null argument", who);
    if (view)
        if (int rc = pt::validate_view(who, view)) return rc;
    if (cam->pxl_width != t->w || cam->pxl_height != t->h)
        return pt::fail(PT_E_INVALID, "%s: the camera is %dx%d, the history %dx%d", who, cam->pxl_width, cam->pxl_height, t->w, t->h);
    if (!std::isfinite(cam->dist_from_film) || !(cam->dist_from_film > 0.0f))
        return pt::fail(PT_E_INVALID, "%s: dist_from_film must be finite and > 0", who);
    if (!std::isfinite(cam->focal_length) || !(cam->focal_length > 0.0f))
        return pt::fail(PT_E_INVALID, "%s: focal_length must be finite and > 0", who);
    if (pt::ctx_in_flight(t->ctx) > 0)
        return pt::fail(PT_E_INVALID, "%s: %d asynchronous renders in flight (pt_render_wait first)", who, pt::ctx_in_flight(t->ctx));
    return PT_OK;
}

// The push on device buffers, after the checks.
int push_device(pt_temporal* t, const pt_camera* cam, const pt_view* view, uint32_t flags, const float* d_in, const pt_feature* d_feat,
                float* d_out, float* d_var, void* stream_v)
{
    HIP_TRY(hipSetDevice(pt::ctx_device(t->ctx)));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    TpArgs a;
    a.rd = t->set(t->cur);
    a.wr = t->set(t->cur ^ 1);
    a.in = d_in;
    a.feat = reinterpret_cast<const float4*>(d_feat);
    a.out = d_out;
    a.var = d_var;
    a.prev_cam = t->prev_cam;
    a.prev_view = t->prev_view;
    a.off_prev = t->off_prev;
    a.max_history = (float)t->tp.max_history;
    a.normal_min = t->tp.normal_min;
    a.plane_tol = t->tp.plane_tol;
    a.w = t->w;
    a.h = t->h;
    a.morton = t->order == PT_ORDER_MORTON;
    a.first = t->frames == 0;
    const dim3 grid((unsigned)((t->w + 63) / 64), (unsigned)((t->h + 3) / 4));
    hipLaunchKernelGGL(tp_push, grid, dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    t->cur ^= 1;
    t->frames += 1;
    t->prev_cam = *cam;
    t->prev_view = view ? *view : pt::identity_view();
    t->off_prev = (flags & PT_FLAG_JITTER) ? 0.5f : 0.0f;
    return PT_OK;
}

}  // namespace

extern "C" {

void pt_temporal_defaults(pt_temporal_params* p)
{
    if (!p) return;
    p->max_history = 32;
    p->normal_min = 0.9f;
    p->plane_tol = 0.02f;
    p->flags = 0;
}

pt_temporal* pt_temporal_create(pt_ctx* c, const pt_temporal_params* tp, int w, int h, int order, int* err)
{
    pt::clear_error();
    pt_temporal* t = nullptr;
    auto make = [&]() -> int {
        const char* who = "pt_temporal_create";
        if (!tp) return pt::fail(PT_E_INVALID, "%s: null argument", who);
        if (tp->max_history < 1) return pt::fail(PT_E_INVALID, "%s: max_history %d must be >= 1", who, tp->max_history);
        if (!std::isfinite(tp->normal_min) || tp->normal_min < -1.0f || tp->normal_min > 1.0f)
            return pt::fail(PT_E_INVALID, "%s: normal_min must be finite and in [-1, 1]", who);
        if (!std::isfinite(tp->plane_tol) || !(tp->plane_tol > 0.0f)) return pt::fail(PT_E_INVALID, "%s: plane_tol must be finite and > 0", who);
        if (tp->flags != 0) return pt::fail(PT_E_INVALID, "%s: unknown flags 0x%x", who, tp->flags);
        if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return pt::fail(PT_E_INVALID, "%s: image size %dx%d out of range (1..65535)", who, w, h);
        if (order != PT_ORDER_SCANLINE && order != PT_ORDER_MORTON) return pt::fail(PT_E_INVALID, "%s: unknown pixel order %d", who, order);
        if (order == PT_ORDER_MORTON && !morton_ok(w, h))
            return pt::fail(PT_E_INVALID, "%s: Morton pixel order needs a square power-of-two image, not %dx%d", who, w, h);
        if (!c) return pt::fail(PT_E_INVALID, "%s: null context", who);
        if (pt::ctx_in_flight(c) > 0)
            return pt::fail(PT_E_INVALID, "%s: %d asynchronous renders in flight (pt_render_wait first)", who, pt::ctx_in_flight(c));
        t = new (std::nothrow) pt_temporal();
        if (!t) return pt::fail(PT_E_OOM, "%s: out of host memory", who);
        t->ctx = c;
        t->tp = *tp;
        t->w = w;
        t->h = h;
        t->order = order;
        t->prev_view = pt::identity_view();
        HIP_TRY(hipSetDevice(pt::ctx_device(c)));
        HIP_TRY(hipMalloc(&t->mem, 2 * t->pixels() * kSetBytes));
        HIP_TRY(hipMemset(t->mem, 0, 2 * t->pixels() * kSetBytes));
        HIP_TRY(hipDeviceSynchronize());
        return PT_OK;
    };
    const int code = make();
    if (code != PT_OK && t) {
        pt_temporal_destroy(t);
        t = nullptr;
    }
    if (err) *err = code;
    return t;
}

int pt_temporal_push_device(pt_temporal* t, const pt_camera* cam, const pt_view* view, uint32_t flags, const float* d_in,
                            const pt_feature* d_feat, float* d_out, float* d_var, void* stream)
{
    pt::clear_error();
    if (int rc = check_push("pt_temporal_push_device", t, cam, view, d_in, d_feat, d_out)) return rc;
    if (reinterpret_cast<uintptr_t>(d_feat) & 15u) return pt::fail(PT_E_INVALID, "pt_temporal_push_device: d_feat is not 16-byte aligned");
    return push_device(t, cam, view, flags, d_in, d_feat, d_out, d_var, stream);
}

int pt_temporal_push(pt_temporal* t, const pt_camera* cam, const pt_view* view, uint32_t flags, const float* in, const pt_feature* feat,
                     float* out, float* var)
{
    pt::clear_error();
    if (int rc = check_push("pt_temporal_push", t, cam, view, in, feat, out)) return rc;
    HIP_TRY(hipSetDevice(pt::ctx_device(t->ctx)));
    const size_t n = t->pixels();
    if (!t->d_img) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->d_img), n * 3 * sizeof(float)));
    if (!t->d_feat) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->d_feat), n * sizeof(pt_feature)));
    if (var && !t->d_var) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->d_var), n * sizeof(float)));
    HIP_TRY(hipMemcpy(t->d_img, in, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t->d_feat, feat, n * sizeof(pt_feature), hipMemcpyHostToDevice));
    if (int rc = push_device(t, cam, view, flags, t->d_img, t->d_feat, t->d_img, var ? t->d_var : nullptr, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, t->d_img, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (var) HIP_TRY(hipMemcpy(var, t->d_var, n * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_temporal_length(pt_temporal* t, float* n_out)
{
    pt::clear_error();
    if (!t || !n_out) return pt::fail(PT_E_INVALID, "pt_temporal_length: null argument");
    if (pt::ctx_in_flight(t->ctx) > 0)
        return pt::fail(PT_E_INVALID, "pt_temporal_length: %d asynchronous renders in flight (pt_render_wait first)", pt::ctx_in_flight(t->ctx));
    const size_t n = t->pixels();
    if (t->frames == 0) {
        memset(n_out, 0, n * sizeof(float));
        return PT_OK;
    }
    HIP_TRY(hipSetDevice(pt::ctx_device(t->ctx)));
    std::vector<float4> c(n);
    HIP_TRY(hipMemcpy(c.data(), t->set(t->cur).c, n * sizeof(float4), hipMemcpyDeviceToHost));
    for (int y = 0; y < t->h; ++y)
        for (int x = 0; x < t->w; ++x) {
            const size_t p = (size_t)y * t->w + x;
            n_out[t->order == PT_ORDER_MORTON ? (size_t)pt_morton_pxl_to_i((uint32_t)x, (uint32_t)y) : p] = c[p].w;
        }
    return PT_OK;
}

int pt_temporal_frames(const pt_temporal* t) { return t ? t->frames : 0; }

int pt_temporal_reset(pt_temporal* t)
{
    pt::clear_error();
    if (!t) return pt::fail(PT_E_INVALID, "pt_temporal_reset: null argument");
    t->frames = 0;
    return PT_OK;
}

void pt_temporal_destroy(pt_temporal* t)
{
    if (!t) return;
    (void)hipSetDevice(pt::ctx_device(t->ctx));
    if (t->mem) (void)hipFree(t->mem);
    if (t->d_img) (void)hipFree(t->d_img);
    if (t->d_feat) (void)hipFree(t->d_feat);
    if (t->d_var) (void)hipFree(t->d_var);
    delete t;
}

}  // extern "C"
