// pt_lightmap.hip -- lightmap finishing (include/pt/pt.h, pt_lightmap_*): the gutter fill that ends a bake and the
// lightmapped view that shows one on the geometry, for gfx950.  Both rules are the header's, operation by operation
// (the fill in integers; the view in f32, no contraction, IEEE division); tests/lightmap_ref.py restates them in numpy
// and the kernels agree with it in every bit.
//
// Two kernels, nothing of pt_render.hip (the view reads the scene's original-order triangle records where pt_create
// put them: pt_ctx.h, tris_orig):
//   lm_dilate  a block of 256 threads owns a tile of 64 x 32 texels.  Its waves stage the covered flags of the tile
//              and a halo of `radius` as one bit per texel: a wave loads 64 consecutive flags (one byte per lane, 64 B
//              coalesced), __ballot makes them a 64-bit word, lane 0 stores it -- two words per row (the tile's 64
//              columns; the 32 columns left of it and the 32 right of it, of which only the 2 * radius halo columns
//              are loaded), (32 + 2 * radius) rows, at most 1024 B of LDS, eight words' loads in flight per wave.  No
//              atomics.  A lane then owns column x of the tile and eight of its rows (wave + 4 * t): every lane of a
//              wave reads the same row words (an LDS broadcast), shifts its own 64-bit window out of them with the
//              centre at bit 32, and finds the nearest covered texel left and right of the centre with one clz and one
//              ctz.  Rows are visited in the order 0, -1, +1, -2, +2, ... and the search ends at the first |j| with j*j
//              above the best squared distance so far, so a texel next to a chart costs a few rows, not (2r+1)^2 taps.
//              The colours are gathered once, at the end: the lane's 24 loads together, then its stores.
//   lm_shade   one thread per feature record, no LDS: the record as three 16-B loads, the triangle record as three
//              16-B loads, six chart coordinates, four taps of three floats.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "../host/host_internal.h"
#include "pt_ctx.h"
#include "pt_hip_util.h"

namespace {

static_assert(sizeof(pt_feature) == 48, "pt_feature is 48 B");
static_assert(sizeof(pt_lightmap_params) == 16, "pt_lightmap_params is 16 B");

constexpr int kTileW = 64, kTileH = 32;
constexpr int kMaxRadius = 16;
constexpr int kRowsMax = kTileH + 2 * kMaxRadius;
constexpr int kStage = 8;   // flag words a wave loads before it waits for any

struct LmDilateArgs {
    const uint32_t* in;      // W*H*3 words (the floats' bits)
    const uint8_t* covered;
    uint32_t* out;
    int32_t* src;            // may be null
    int32_t w, h, radius;
};

// The 64 flags around column `lane` of the tile, the column itself at bit 32: bit k is column lane - 32 + k.
// R: the row's two words -- the tile's columns 0..63, then the halo: columns -32..-1 in its low half, 64..95 in its
// high half.
__device__ __forceinline__ unsigned long long lm_window(const unsigned long long* R, int lane)
{
    if (lane < 32) return ((R[1] & 0xffffffffull) >> lane) | (R[0] << (32 - lane));
    return (R[0] >> (lane - 32)) | (((R[1] >> 32) << 1) << (95 - lane));
}

__global__ __launch_bounds__(256) void lm_dilate(LmDilateArgs a)
{
    __shared__ unsigned long long bits[kRowsMax * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int r = a.radius;
    // ---- the flags, kStage words per wave and step: their loads are issued together, every one from inside the image
    // (a lane with nothing to load reads flag 0 and drops it), then the ballots.  Wave-uniform throughout.
    const int words = (kTileH + 2 * r) * 2;
    for (int k0 = wave * kStage; k0 < words; k0 += 4 * kStage) {
        uint8_t flag[kStage];
        bool want[kStage];
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int k = k0 + u, row = k >> 1;
            const int y = y0 - r + row;
            const int x = (k & 1) ? x0 + lane + (lane < 32 ? -32 : 32) : x0 + lane;
            want[u] = k < words && y >= 0 && y < a.h && x >= x0 - r && x < x0 + kTileW + r && x >= 0 && x < a.w;
            flag[u] = a.covered[want[u] ? (size_t)y * a.w + x : (size_t)0];
        }
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const unsigned long long m = __ballot(want[u] && flag[u] != 0);
            if (lane == 0 && k0 + u < words) bits[k0 + u] = m;
        }
    }
    __syncthreads();
    const int x = x0 + lane;
    if (x >= a.w) return;
    // ---- the search: where each of the lane's eight texels takes its colour from.  No memory but LDS.
    // the window's columns -r..r about the centre, and the half of it at and left of the centre
    const unsigned long long win = ((2ull << (2 * r)) - 1ull) << (32 - r), left = (2ull << 32) - 1ull;
    constexpr int kPer = kTileH / 4;
    uint32_t from[kPer];
    int32_t src[kPer];
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        const int ly = wave + 4 * t, y = y0 + ly;
        const int yc = y < a.h ? y : a.h - 1;                    // (a row below the image: loaded from the last row, never stored)
        from[t] = (uint32_t)yc * (uint32_t)a.w + (uint32_t)x;
        src[t] = (int32_t)from[t];
        if (y >= a.h || ((bits[(ly + r) * 2] >> lane) & 1ull)) continue;
        int best = INT_MAX, bi = 0, bj = 0;
        for (int k = 0; k <= r && k * k <= best; ++k) {
            for (int sgn = 0; sgn < (k ? 2 : 1); ++sgn) {
                const int j = sgn ? k : -k;
                const unsigned long long v = lm_window(bits + (ly + r + j) * 2, lane) & win;
                if (!v) continue;
                const unsigned long long vl = v & left, vr = v & ~left;
                const int da = vl ? __builtin_clzll(vl) - 31 : 64;   // the nearest at or left of the centre is da columns away
                const int db = vr ? __builtin_ctzll(vr) - 32 : 64;   // ... right of it, db columns
                const int i = (da <= db) ? -da : db;                 // (a tie goes to the smaller i)
                const int d2 = i * i + j * j;
                if (d2 < best || (d2 == best && j < bj)) { best = d2; bi = i; bj = j; }
            }
        }
        if (best != INT_MAX) {
            from[t] = (uint32_t)(y + bj) * (uint32_t)a.w + (uint32_t)(x + bi);
            src[t] = (int32_t)from[t];
        } else {
            src[t] = -1;
        }
    }
    // ---- the colours: all 24 loads, then the stores
    uint32_t c[kPer][3];
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        const size_t q = (size_t)from[t] * 3;
        c[t][0] = a.in[q];
        c[t][1] = a.in[q + 1];
        c[t][2] = a.in[q + 2];
    }
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        const int y = y0 + wave + 4 * t;
        if (y >= a.h) break;
        const size_t p = (size_t)y * a.w + x;
        a.out[p * 3] = c[t][0];
        a.out[p * 3 + 1] = c[t][1];
        a.out[p * 3 + 2] = c[t][2];
        if (a.src) a.src[p] = src[t];
    }
}

struct LmShadeArgs {
    const float4* feat;      // 3 per record
    const float4* tris;      // 3 per original triangle: {v0, e1.x} {e1.yz, e2.xy} {e2.z, ...}
    const float* tri_uv;     // 6 per original triangle
    const float* map;        // map_w * map_h * 3
    float* out;
    float fill[3];
    uint32_t n, num_tris, no_albedo;
    int32_t map_w, map_h;
};

__device__ __forceinline__ float lm_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ float lm_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // (a NaN stays)
__device__ __forceinline__ bool lm_finite(float v) { return fabsf(v) < INFINITY; }
__device__ __forceinline__ int lm_texel(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

__global__ __launch_bounds__(256) void lm_shade(LmShadeArgs a)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.n) return;
    const float4 f0 = a.feat[(size_t)p * 3], f1 = a.feat[(size_t)p * 3 + 1], f2 = a.feat[(size_t)p * 3 + 2];   // {albedo, depth} {n, prim} {P, -}
    const int32_t prim = __float_as_int(f1.w);
    float o[3] = {a.fill[0], a.fill[1], a.fill[2]};
    if (prim >= 0 && !(prim & PT_FEATURE_EMISSIVE) && (uint32_t)prim < a.num_tris) {
        const float* uv = a.tri_uv + (size_t)prim * 6;
        const float uax = uv[0], uay = uv[1], ubx = uv[2], uby = uv[3], ucx = uv[4], ucy = uv[5];
        const float4 ta = a.tris[(size_t)prim * 3], tb = a.tris[(size_t)prim * 3 + 1], tc = a.tris[(size_t)prim * 3 + 2];
        const float gx = f2.x - ta.x, gy = f2.y - ta.y, gz = f2.z - ta.z;
        const float d11 = lm_dot(ta.w, tb.x, tb.y, ta.w, tb.x, tb.y), d12 = lm_dot(ta.w, tb.x, tb.y, tb.z, tb.w, tc.x);
        const float d22 = lm_dot(tb.z, tb.w, tc.x, tb.z, tb.w, tc.x);
        const float g1 = lm_dot(gx, gy, gz, ta.w, tb.x, tb.y), g2 = lm_dot(gx, gy, gz, tb.z, tb.w, tc.x);
        const float det = d11 * d22 - d12 * d12;
        if (uax == uax && det != 0.0f && lm_finite(det)) {
            const float b1 = lm_clamp((d22 * g1 - d12 * g2) / det, 0.0f, 1.0f);
            const float b2 = lm_clamp((d11 * g2 - d12 * g1) / det, 0.0f, 1.0f);
            const float u = (uax + b1 * (ubx - uax)) + b2 * (ucx - uax);
            const float v = (uay + b1 * (uby - uay)) + b2 * (ucy - uay);
            const float s = u * (float)a.map_w - 0.5f, t = v * (float)a.map_h - 0.5f;
            if (lm_finite(s) && lm_finite(t)) {
                const float sc = lm_clamp(s, -1.0f, (float)a.map_w), tc2 = lm_clamp(t, -1.0f, (float)a.map_h);
                const float xf = floorf(sc), yf = floorf(tc2);
                const float fx = sc - xf, fy = tc2 - yf;
                const int xa = lm_texel((int)xf, a.map_w), xb = lm_texel((int)xf + 1, a.map_w);
                const int ya = lm_texel((int)yf, a.map_h), yb = lm_texel((int)yf + 1, a.map_h);
                const float* m00 = a.map + ((size_t)ya * a.map_w + xa) * 3;
                const float* m10 = a.map + ((size_t)ya * a.map_w + xb) * 3;
                const float* m01 = a.map + ((size_t)yb * a.map_w + xa) * 3;
                const float* m11 = a.map + ((size_t)yb * a.map_w + xb) * 3;
                const float alb[3] = {f0.x, f0.y, f0.z};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float l00 = m00[k], l10 = m10[k], l01 = m01[k], l11 = m11[k];
                    const float top = l00 + fx * (l10 - l00);
                    const float bot = l01 + fx * (l11 - l01);
                    const float val = top + fy * (bot - top);
                    o[k] = a.no_albedo ? val : alb[k] * val;
                }
            }
        }
    }
    a.out[(size_t)p * 3] = o[0];
    a.out[(size_t)p * 3 + 1] = o[1];
    a.out[(size_t)p * 3 + 2] = o[2];
}

int check_ctx(const char* who, pt_ctx* c)
{
    if (!c) return pt::fail(PT_E_INVALID, "%s: null ctx", who);
    if (pt::ctx_in_flight(c) > 0)
        return pt::fail(PT_E_INVALID, "%s: %d asynchronous renders in flight (pt_render_wait first)", who, pt::ctx_in_flight(c));
    return PT_OK;
}

bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

// What both dilate variants check of their arguments (the buffers' names are the variant's own); the context last, so
// that a bad size or radius is refused with or without a device.
int check_dilate(const char* who, pt_ctx* c, int w, int h, int radius, const void* in, const char* in_name, const void* covered,
                 const char* covered_name, const void* out, const char* out_name)
{
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return pt::fail(PT_E_INVALID, "%s: width x height %dx%d out of range (1..65535)", who, w, h);
    if ((int64_t)w * h > (int64_t)INT32_MAX)
        return pt::fail(PT_E_INVALID, "%s: width x height %dx%d has more than 2^31 - 1 texels (src is an int32)", who, w, h);
    if (radius < 0 || radius > kMaxRadius) return pt::fail(PT_E_INVALID, "%s: radius %d out of range (0..%d)", who, radius, kMaxRadius);
    if (!in) return pt::fail(PT_E_INVALID, "%s: null %s", who, in_name);
    if (!covered) return pt::fail(PT_E_INVALID, "%s: null %s", who, covered_name);
    if (!out) return pt::fail(PT_E_INVALID, "%s: null %s", who, out_name);
    return check_ctx(who, c);
}

int dilate_device(pt_ctx* c, int w, int h, int radius, const float* d_in, const uint8_t* d_covered, float* d_out, int32_t* d_src,
                  hipStream_t stream)
{
    LmDilateArgs a;
    a.in = reinterpret_cast<const uint32_t*>(d_in);
    a.covered = d_covered;
    a.out = reinterpret_cast<uint32_t*>(d_out);
    a.src = d_src;
    a.w = w;
    a.h = h;
    a.radius = radius;
    const dim3 grid((unsigned)((w + kTileW - 1) / kTileW), (unsigned)((h + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(lm_dilate, grid, dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}

int check_shade(const char* who, pt_ctx* c, const pt_lightmap_params* lp, uint32_t n, const void* feat, const char* feat_name,
                const void* tri_uv, const char* uv_name, const void* map, const char* map_name, int map_w, int map_h, const void* out,
                const char* out_name)
{
    if (!lp) return pt::fail(PT_E_INVALID, "%s: null params", who);
    if (lp->flags & ~(uint32_t)PT_LIGHTMAP_NO_ALBEDO) return pt::fail(PT_E_INVALID, "%s: unknown flags 0x%x", who, lp->flags);
    if (map_w <= 0 || map_h <= 0 || map_w > 65535 || map_h > 65535)
        return pt::fail(PT_E_INVALID, "%s: map_w x map_h %dx%d out of range (1..65535)", who, map_w, map_h);
    if (!map) return pt::fail(PT_E_INVALID, "%s: null %s", who, map_name);
    if (int rc = check_ctx(who, c)) return rc;
    if (!tri_uv && c->num_tris > 0) return pt::fail(PT_E_INVALID, "%s: null %s", who, uv_name);
    if (n > 0 && !feat) return pt::fail(PT_E_INVALID, "%s: null %s", who, feat_name);
    if (n > 0 && !out) return pt::fail(PT_E_INVALID, "%s: null %s", who, out_name);
    return PT_OK;
}

int shade_device(pt_ctx* c, const pt_lightmap_params* lp, uint32_t n, const pt_feature* d_feat, const float* d_tri_uv, const float* d_map,
                 int map_w, int map_h, float* d_out, hipStream_t stream)
{
    if (n == 0) return PT_OK;
    LmShadeArgs a;
    a.feat = reinterpret_cast<const float4*>(d_feat);
    a.tris = reinterpret_cast<const float4*>(c->tris_orig);
    a.tri_uv = d_tri_uv;
    a.map = d_map;
    a.out = d_out;
    memcpy(a.fill, lp->fill, sizeof(a.fill));
    a.n = n;
    a.num_tris = c->num_tris;
    a.no_albedo = (lp->flags & PT_LIGHTMAP_NO_ALBEDO) ? 1u : 0u;
    a.map_w = map_w;
    a.map_h = map_h;
    hipLaunchKernelGGL(lm_shade, dim3((n + 255u) / 256u), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_lightmap_dilate_device(pt_ctx* c, int w, int h, int radius, const float* d_in, const uint8_t* d_covered, float* d_out, int32_t* d_src,
                              void* stream)
{
    pt::clear_error();
    const char* who = "pt_lightmap_dilate_device";
    if (int rc = check_dilate(who, c, w, h, radius, d_in, "d_in", d_covered, "d_covered", d_out, "d_out")) return rc;
    if (!aligned(d_in, 4)) return pt::fail(PT_E_INVALID, "%s: d_in is not 4-byte aligned", who);
    if (!aligned(d_out, 4)) return pt::fail(PT_E_INVALID, "%s: d_out is not 4-byte aligned", who);
    if (!aligned(d_src, 4)) return pt::fail(PT_E_INVALID, "%s: d_src is not 4-byte aligned", who);
    HIP_TRY(hipSetDevice(c->device));
    return dilate_device(c, w, h, radius, d_in, d_covered, d_out, d_src, reinterpret_cast<hipStream_t>(stream));
}

int pt_lightmap_dilate(pt_ctx* c, int w, int h, int radius, const float* in, const uint8_t* covered, float* out, int32_t* src)
{
    pt::clear_error();
    if (int rc = check_dilate("pt_lightmap_dilate", c, w, h, radius, in, "in", covered, "covered", out, "out")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)w * (size_t)h;
    pt::ScopedDevice<float> d_img;
    pt::ScopedDevice<uint8_t> d_cov;
    pt::ScopedDevice<int32_t> d_src;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_img), n * 3 * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_cov), n));
    if (src) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_src), n * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(d_img, in, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_cov, covered, n, hipMemcpyHostToDevice));
    if (int rc = dilate_device(c, w, h, radius, d_img, d_cov, d_img, d_src, nullptr)) return rc;   // (in place: legal by the rule)
    HIP_TRY(hipMemcpy(out, d_img, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (src) HIP_TRY(hipMemcpy(src, d_src, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_lightmap_shade_device(pt_ctx* c, const pt_lightmap_params* lp, uint32_t n, const pt_feature* d_feat, const float* d_tri_uv,
                             const float* d_map, int map_w, int map_h, float* d_out, void* stream)
{
    pt::clear_error();
    const char* who = "pt_lightmap_shade_device";
    if (int rc = check_shade(who, c, lp, n, d_feat, "d_feat", d_tri_uv, "d_tri_uv", d_map, "d_map", map_w, map_h, d_out, "d_out")) return rc;
    if (!aligned(d_feat, 16)) return pt::fail(PT_E_INVALID, "%s: d_feat is not 16-byte aligned", who);
    if (!aligned(d_tri_uv, 4)) return pt::fail(PT_E_INVALID, "%s: d_tri_uv is not 4-byte aligned", who);
    if (!aligned(d_map, 4)) return pt::fail(PT_E_INVALID, "%s: d_map is not 4-byte aligned", who);
    if (!aligned(d_out, 4)) return pt::fail(PT_E_INVALID, "%s: d_out is not 4-byte aligned", who);
    HIP_TRY(hipSetDevice(c->device));
    return shade_device(c, lp, n, d_feat, d_tri_uv, d_map, map_w, map_h, d_out, reinterpret_cast<hipStream_t>(stream));
}

int pt_lightmap_shade(pt_ctx* c, const pt_lightmap_params* lp, uint32_t n, const pt_feature* feat, const float* tri_uv, const float* map,
                      int map_w, int map_h, float* out)
{
    pt::clear_error();
    if (int rc = check_shade("pt_lightmap_shade", c, lp, n, feat, "feat", tri_uv, "tri_uv", map, "map", map_w, map_h, out, "out")) return rc;
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t map_floats = (size_t)map_w * (size_t)map_h * 3, uv_floats = (size_t)c->num_tris * 6;
    pt::ScopedDevice<pt_feature> d_feat;
    pt::ScopedDevice<float> d_uv, d_map, d_out;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_feat), (size_t)n * sizeof(pt_feature)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_uv), (uv_floats ? uv_floats : 1) * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_map), map_floats * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_out), (size_t)n * 3 * sizeof(float)));
    HIP_TRY(hipMemcpy(d_feat, feat, (size_t)n * sizeof(pt_feature), hipMemcpyHostToDevice));
    if (uv_floats) HIP_TRY(hipMemcpy(d_uv, tri_uv, uv_floats * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_map, map, map_floats * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = shade_device(c, lp, n, d_feat, d_uv, d_map, map_w, map_h, d_out, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, d_out, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"
