// pt_denoise.hip -- the preview denoiser (include/pt/pt.h, pt_denoise*): a feature-guided, edge-avoiding
// a-trous filter over the fp32 mean image, for gfx950.  The arithmetic is the header's, operation by
// operation (f32, no contraction, IEEE division); tests/denoise_ref.py restates it in numpy and the
// kernels agree with it in every bit, whatever the tiling.
//
// Three kernels over an internal layout of four 16-B planes per pixel (scanline order, 64 B per pixel):
//   G0 = {P.xyz, s_p}   G1 = {n.xyz, skip}   C0 / C1 = {c.rgb, -} ping-pong
//   dn_prepass   (in, features) -> G0, G1, C0: resolves the pixel order, demodulates; skip = 1 marks a
//                pass-through pixel, whose C holds its input unchanged through every iteration
//   dn_iterate   one a-trous iteration C[src] -> C[dst].  kTiled: the 25 taps come from LDS.  A block owns
//                64 consecutive x of kRows rows of the step lattice (rows y = ry + step*k: the pixels of equal
//                y mod step form an independent sub-image in y) and stages those rows plus two lattice
//                rows above and below, each with a halo of 2*step pixels left and right: every global load
//                is a coalesced 16-B load of consecutive pixels whatever the step, and a pixel outside the
//                image is staged as skip = 1.  !kTiled: the same loop gathering straight from the planes
//                (25 taps x 48 B per pixel) -- the baseline, PT_DENOISE_DIRECT=1.
//   dn_finish    C -> out: remodulates (pass-through pixels: their input), resolves the pixel order
// The variance-guided filter (pt_denoise_guided*) runs on the same planes with kernels of its own: the C planes' .w
// carries v, the variance of the pixel's demodulated mean luminance, so the LDS tile is no larger; two more 4-B planes
// (72 B per pixel) hold a compact copy of v for the prefilter (V: -1 marks a pass-through pixel, v itself is never
// negative) and the prefiltered variance (VB):
//   dg_prepass   dn_prepass, plus v from the caller's variance map, into C0.w and V
//   dg_blur      once per iteration, V -> VB: vbar = the 3x3 binomial mean of v at a spacing of 1 pixel (whatever the
//                step, so it cannot come from the staged lattice rows).  Nine coalesced 4-B loads per pixel; read
//                from the .w of the 16-B planes instead it took 40 us a call at 1920x1080
//   dg_iterate   dn_iterate with the luminance weight 1 / (1 + dl^2 / (sigma_luma^2 vbar_p)) on every tap, and v
//                filtered along: v' = sum(w^2 v_q) / wsum^2, written to C.w and V.  Both gathers, as dn_iterate
//   dn_finish    as above (it never reads .w)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../host/host_internal.h"
#include "pt_hip_util.h"

namespace {

static_assert(sizeof(pt_feature) == 48, "pt_feature is 48 B");

constexpr int kTileX = 64;      // consecutive pixels of a row per block (one wave per row)
constexpr int kRows = 8;        // lattice rows a block filters; 256 threads = 64 x 4, two rows each
constexpr int kStageRows = kRows + 4;
// LDS staging is kept for the steps where it beat the direct gather at 1920x1080 by more than the run-to-run
// spread (steps 1, 2, 4 at 0.62-0.69x; step 8 tied, step 16 lost 5% -- the 55-72 KB tiles leave 2
// blocks per CU); larger steps take the direct gather.  PT_DENOISE_TILED_MAX overrides (up to kTiledLimit).
constexpr int kTiledMaxStep = 4;
constexpr int kTiledLimit = 16;  // what the LDS budget admits: 12 rows x 128 px x 48 B = 72 KB per block

struct DnArgs {
    float4* g0;
    float4* g1;
    const float4* src;
    float4* dst;
    int32_t w, h;
    int32_t step;
    int32_t npow;          // normal_power_log2
    float sigma_color;     // already divided by 2^it; <= 0: off
};

__device__ __forceinline__ uint32_t dn_morton(uint32_t x, uint32_t y)   // camera.h:66-75
{
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        r |= ((x >> b) & 1u) << (2 * b);
        r |= ((y >> b) & 1u) << (2 * b + 1);
    }
    return r;
}

__device__ __forceinline__ bool dn_pass_through(int32_t prim) { return prim < 0 || (prim & PT_FEATURE_EMISSIVE) != 0; }

__global__ __launch_bounds__(256) void dn_prepass(const float* __restrict__ in, const float* __restrict__ feat, float4* __restrict__ g0,
                                                  float4* __restrict__ g1, float4* __restrict__ c0, int w, int h, int morton,
                                                  int demodulate, float sigma_depth)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const size_t s = morton ? (size_t)dn_morton((uint32_t)x, (uint32_t)y) : p;
    const float* f = feat + s * 12;
    const int32_t prim = __float_as_int(f[7]);
    const bool skip = dn_pass_through(prim);
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = in[s * 3 + k];
        const float al = f[k];
        const float a = demodulate ? ((al > 1e-3f) ? al : 1e-3f) : 1.0f;
        c[k] = skip ? v : v / a;
    }
    g0[p] = make_float4(f[8], f[9], f[10], sigma_depth * f[3]);
    g1[p] = make_float4(f[4], f[5], f[6], skip ? 1.0f : 0.0f);
    c0[p] = make_float4(c[0], c[1], c[2], 0.0f);
}

__global__ __launch_bounds__(256) void dn_finish(const float4* __restrict__ c, const float4* __restrict__ g1, const float* __restrict__ feat,
                                                 float* __restrict__ out, int w, int h, int morton, int demodulate)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const size_t s = morton ? (size_t)dn_morton((uint32_t)x, (uint32_t)y) : p;
    const float4 v = c[p];
    const bool skip = g1[p].w != 0.0f;
    const float cc[3] = {v.x, v.y, v.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float al = feat[s * 12 + k];
        const float a = demodulate ? ((al > 1e-3f) ? al : 1e-3f) : 1.0f;
        out[s * 3 + k] = skip ? cc[k] : cc[k] * a;
    }
}

// The weight of tap q of pixel p: the header's arithmetic, in its order.
__device__ __forceinline__ float dn_weight(const float4 P, const float4 N, const float4 Cp, const float4 Pq, const float4 Nq,
                                           const float4 Cq, float hh, int npow, float sc)
{
    float dn = (N.x * Nq.x + N.y * Nq.y) + N.z * Nq.z;
    dn = (dn > 0.0f) ? dn : 0.0f;
    float wn = dn;
    for (int k = 0; k < npow; ++k) wn = wn * wn;
    const float e = (N.x * (Pq.x - P.x) + N.y * (Pq.y - P.y)) + N.z * (Pq.z - P.z);
    const float r = e / P.w;
    const float wz = 1.0f / (1.0f + r * r);
    float w = (hh * wn) * wz;
    if (sc > 0.0f) {
        const float d0 = Cq.x - Cp.x, d1 = Cq.y - Cp.y, d2 = Cq.z - Cp.z;
        const float dc = (d0 * d0 + d1 * d1) + d2 * d2;
        w = w * (1.0f / (1.0f + dc / (sc * sc)));
    }
    return w;
}

// One tap of pixel p.
__device__ __forceinline__ void dn_tap(const float4 P, const float4 N, const float4 Cp, const float4 Pq, const float4 Nq,
                                       const float4 Cq, float hh, int npow, float sc, float (&acc)[3], float& wsum)
{
    const float w = dn_weight(P, N, Cp, Pq, Nq, Cq, hh, npow, sc);
    acc[0] = acc[0] + w * Cq.x;
    acc[1] = acc[1] + w * Cq.y;
    acc[2] = acc[2] + w * Cq.z;
    wsum = wsum + w;
}

__device__ __forceinline__ float dn_h(int k)   // {1/16, 1/4, 3/8, 1/4, 1/16} at k = -2..2
{
    return (k == 0) ? 0.375f : ((k == 1 || k == -1) ? 0.25f : 0.0625f);
}

template <bool kTiled>
__global__ __launch_bounds__(256) void dn_iterate(DnArgs a)
{
    extern __shared__ float4 dn_lds[];
    const int lx = threadIdx.x & 63, lr = threadIdx.x >> 6;
    const int step = a.step;
    const int x = blockIdx.x * kTileX + lx;
    // blockIdx.y = (tile of kRows lattice rows) * step + (row residue ry)
    const int ry = kTiled ? (int)(blockIdx.y % (unsigned)step) : 0;
    const int k0 = kTiled ? (int)(blockIdx.y / (unsigned)step) * kRows : 0;
    const int tw = kTileX + 4 * step;                       // staged pixels per row
    float4* const s0 = dn_lds;                              // G0, G1, C planes of kStageRows x tw
    float4* const s1 = dn_lds + kStageRows * tw;
    float4* const s2 = dn_lds + 2 * kStageRows * tw;
    if (kTiled) {
        const int xl = blockIdx.x * kTileX - 2 * step;      // image x of staged column 0
        for (int e = threadIdx.x; e < kStageRows * tw; e += 256) {   // e = r * tw + cx
            const int r = e / tw, cx = e - r * tw;
            const int yy = ry + (k0 + r - 2) * step, xx = xl + cx;
            float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = make_float4(0.0f, 0.0f, 0.0f, 1.0f), q2 = q0;
            if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
                const size_t g = (size_t)yy * a.w + xx;
                q1 = a.g1[g];
                q0 = a.g0[g];
                q2 = a.src[g];
            }
            s0[e] = q0; s1[e] = q1; s2[e] = q2;
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int half = 0; half < (kTiled ? kRows / 4 : 1); ++half) {
        const int lrow = lr + 4 * half;                     // lattice row of the block this lane filters
        const int y = kTiled ? ry + (k0 + lrow) * step : (int)blockIdx.y * 4 + lr;
        if (x >= a.w || y >= a.h) continue;
        const size_t p = (size_t)y * a.w + x;
        const int cl = lx + 2 * step, rl = lrow + 2;        // this pixel's staged column / row
        const float4 N = kTiled ? s1[rl * tw + cl] : a.g1[p];
        const float4 Cp = kTiled ? s2[rl * tw + cl] : a.src[p];
        if (N.w != 0.0f) {                                  // pass-through: unchanged
            a.dst[p] = Cp;
            continue;
        }
        const float4 P = kTiled ? s0[rl * tw + cl] : a.g0[p];
        float acc[3] = {0.0f, 0.0f, 0.0f};
        float wsum = 0.0f;
        for (int j = -2; j <= 2; ++j) {
            const int yq = y + j * step;
            if (!kTiled && (yq < 0 || yq >= a.h)) continue;
#pragma unroll
            for (int i = -2; i <= 2; ++i) {
                const int xq = x + i * step;
                float4 Nq;
                if (kTiled) {
                    Nq = s1[(rl + j) * tw + cl + i * step];
                } else {
                    if (xq < 0 || xq >= a.w) continue;
                    Nq = a.g1[(size_t)yq * a.w + xq];
                }
                if (Nq.w != 0.0f) continue;                 // pass-through or outside the image
                const float4 Pq = kTiled ? s0[(rl + j) * tw + cl + i * step] : a.g0[(size_t)yq * a.w + xq];
                const float4 Cq = kTiled ? s2[(rl + j) * tw + cl + i * step] : a.src[(size_t)yq * a.w + xq];
                dn_tap(P, N, Cp, Pq, Nq, Cq, dn_h(j) * dn_h(i), a.npow, a.sigma_color, acc, wsum);
            }
        }
        float4 o = Cp;
        if (wsum > 0.0f) {
            o.x = acc[0] / wsum; o.y = acc[1] / wsum; o.z = acc[2] / wsum;
        }
        a.dst[p] = o;
    }
}

// ---------------------------------------------------------------- the variance-guided filter's kernels
struct DgArgs {
    DnArgs d;
    float* vpl;            // V: v of every filtered pixel, -1 for a pass-through one (dg_iterate writes, dg_blur reads)
    float* vbar;           // VB: the prefiltered variance (dg_blur writes it, dg_iterate reads it)
    float sl2;             // sigma_luma * sigma_luma
};

__device__ __forceinline__ float dn_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__global__ __launch_bounds__(256) void dg_prepass(const float* __restrict__ in, const float* __restrict__ feat,
                                                  const float* __restrict__ var, float4* __restrict__ g0, float4* __restrict__ g1,
                                                  float4* __restrict__ c0, float* __restrict__ vpl, int w, int h, int morton,
                                                  int demodulate, float sigma_depth)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const size_t s = morton ? (size_t)dn_morton((uint32_t)x, (uint32_t)y) : p;
    const float* f = feat + s * 12;
    const int32_t prim = __float_as_int(f[7]);
    const bool skip = dn_pass_through(prim);
    float c[3], a[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = in[s * 3 + k];
        const float al = f[k];
        a[k] = demodulate ? ((al > 1e-3f) ? al : 1e-3f) : 1.0f;
        c[k] = skip ? v : v / a[k];
    }
    // the variance of the mean luminance, demodulated by the albedo's luminance; unknown (1e30) when it is NaN,
    // negative, infinite or overflows
    const float A = demodulate ? dn_luma(a[0], a[1], a[2]) : 1.0f;
    const float vp = var[s];
    const float t = vp / (A * A);
    const float v = (vp >= 0.0f && t < 1e30f) ? t : 1e30f;
    g0[p] = make_float4(f[8], f[9], f[10], sigma_depth * f[3]);
    g1[p] = make_float4(f[4], f[5], f[6], skip ? 1.0f : 0.0f);
    c0[p] = make_float4(c[0], c[1], c[2], v);
    vpl[p] = skip ? -1.0f : v;
}

__device__ __forceinline__ float dg_g(int k) { return (k == 0) ? 0.5f : 0.25f; }   // {1/4, 1/2, 1/4} at k = -1..1

// vbar of every filtered pixel from the compact plane of this iteration's input v
__global__ __launch_bounds__(256) void dg_blur(const float* __restrict__ vpl, float* __restrict__ vbar, int w, int h)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    if (vpl[p] < 0.0f) return;                              // pass-through: never read
    float va = 0.0f, vw = 0.0f;
    for (int j = -1; j <= 1; ++j) {
        const int yq = y + j;
        if (yq < 0 || yq >= h) continue;
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int xq = x + i;
            if (xq < 0 || xq >= w) continue;
            const float vq = vpl[(size_t)yq * w + xq];
            if (vq < 0.0f) continue;
            const float g = dg_g(j) * dg_g(i);
            va = va + g * vq;
            vw = vw + g;
        }
    }
    vbar[p] = va / vw;
}

// dn_iterate with the luminance weight; the staging and the lattice are dn_iterate's
template <bool kTiled>
__global__ __launch_bounds__(256) void dg_iterate(DgArgs ga)
{
    extern __shared__ float4 dn_lds[];
    const DnArgs& a = ga.d;
    const int lx = threadIdx.x & 63, lr = threadIdx.x >> 6;
    const int step = a.step;
    const int x = blockIdx.x * kTileX + lx;
    const int ry = kTiled ? (int)(blockIdx.y % (unsigned)step) : 0;
    const int k0 = kTiled ? (int)(blockIdx.y / (unsigned)step) * kRows : 0;
    const int tw = kTileX + 4 * step;
    float4* const s0 = dn_lds;
    float4* const s1 = dn_lds + kStageRows * tw;
    float4* const s2 = dn_lds + 2 * kStageRows * tw;
    if (kTiled) {
        const int xl = blockIdx.x * kTileX - 2 * step;
        for (int e = threadIdx.x; e < kStageRows * tw; e += 256) {
            const int r = e / tw, cx = e - r * tw;
            const int yy = ry + (k0 + r - 2) * step, xx = xl + cx;
            float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = make_float4(0.0f, 0.0f, 0.0f, 1.0f), q2 = q0;
            if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
                const size_t g = (size_t)yy * a.w + xx;
                q1 = a.g1[g];
                q0 = a.g0[g];
                q2 = a.src[g];
            }
            s0[e] = q0; s1[e] = q1; s2[e] = q2;
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int half = 0; half < (kTiled ? kRows / 4 : 1); ++half) {
        const int lrow = lr + 4 * half;
        const int y = kTiled ? ry + (k0 + lrow) * step : (int)blockIdx.y * 4 + lr;
        if (x >= a.w || y >= a.h) continue;
        const size_t p = (size_t)y * a.w + x;
        const int cl = lx + 2 * step, rl = lrow + 2;
        const float4 N = kTiled ? s1[rl * tw + cl] : a.g1[p];
        const float4 Cp = kTiled ? s2[rl * tw + cl] : a.src[p];
        if (N.w != 0.0f) {                                  // pass-through: unchanged, its v too
            a.dst[p] = Cp;
            continue;
        }
        const float4 P = kTiled ? s0[rl * tw + cl] : a.g0[p];
        const float lp = dn_luma(Cp.x, Cp.y, Cp.z);
        const float den = ga.sl2 * ga.vbar[p] + 1e-20f;
        float acc[3] = {0.0f, 0.0f, 0.0f};
        float wsum = 0.0f, vacc = 0.0f;
        for (int j = -2; j <= 2; ++j) {
            const int yq = y + j * step;
            if (!kTiled && (yq < 0 || yq >= a.h)) continue;
#pragma unroll
            for (int i = -2; i <= 2; ++i) {
                const int xq = x + i * step;
                float4 Nq;
                if (kTiled) {
                    Nq = s1[(rl + j) * tw + cl + i * step];
                } else {
                    if (xq < 0 || xq >= a.w) continue;
                    Nq = a.g1[(size_t)yq * a.w + xq];
                }
                if (Nq.w != 0.0f) continue;
                const float4 Pq = kTiled ? s0[(rl + j) * tw + cl + i * step] : a.g0[(size_t)yq * a.w + xq];
                const float4 Cq = kTiled ? s2[(rl + j) * tw + cl + i * step] : a.src[(size_t)yq * a.w + xq];
                float w = dn_weight(P, N, Cp, Pq, Nq, Cq, dn_h(j) * dn_h(i), a.npow, a.sigma_color);
                const float dl = dn_luma(Cq.x, Cq.y, Cq.z) - lp;
                w = w * (1.0f / (1.0f + (dl * dl) / den));
                acc[0] = acc[0] + w * Cq.x;
                acc[1] = acc[1] + w * Cq.y;
                acc[2] = acc[2] + w * Cq.z;
                wsum = wsum + w;
                vacc = vacc + (w * w) * Cq.w;
            }
        }
        float4 o = Cp;
        if (wsum > 0.0f) {
            o.x = acc[0] / wsum; o.y = acc[1] / wsum; o.z = acc[2] / wsum;
            o.w = vacc / (wsum * wsum);
        }
        a.dst[p] = o;
        ga.vpl[p] = o.w;
    }
}

int env_int(const char* name, int dflt)
{
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

bool morton_ok(int w, int h) { return w == h && w > 0 && (w & (w - 1)) == 0; }

int check_params(const char* who, const pt_ctx* c, const pt_denoise_params* dp, int w, int h, int order, const void* in,
                 const void* feat, const void* out)
{
    if (!c || !dp || !in || !feat || !out) return pt::fail(PT_E_INVALID, "%s: null argument", who);
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return pt::fail(PT_E_INVALID, "%s: image size %dx%d out of range (1..65535)", who, w, h);
    if (dp->iterations < 0 || dp->iterations > 8) return pt::fail(PT_E_INVALID, "%s: iterations %d out of range (0..8)", who, dp->iterations);
    if (dp->normal_power_log2 < 0 || dp->normal_power_log2 > 7)
        return pt::fail(PT_E_INVALID, "%s: normal_power_log2 %d out of range (0..7)", who, dp->normal_power_log2);
    if (!std::isfinite(dp->sigma_depth) || !(dp->sigma_depth > 0.0f))
        return pt::fail(PT_E_INVALID, "%s: sigma_depth must be finite and > 0", who);
    if (dp->flags & ~(uint32_t)PT_DENOISE_NO_DEMODULATE) return pt::fail(PT_E_INVALID, "%s: unknown flags 0x%x", who, dp->flags);
    if (order != PT_ORDER_SCANLINE && order != PT_ORDER_MORTON) return pt::fail(PT_E_INVALID, "%s: unknown pixel order %d", who, order);
    if (order == PT_ORDER_MORTON && !morton_ok(w, h))
        return pt::fail(PT_E_INVALID, "%s: Morton pixel order needs a square power-of-two image, not %dx%d", who, w, h);
    if (pt::ctx_in_flight(c) > 0)
        return pt::fail(PT_E_INVALID, "%s: %d asynchronous renders in flight (pt_render_wait first)", who, pt::ctx_in_flight(c));
    return PT_OK;
}

int check_guided(const char* who, const pt_ctx* c, const pt_denoise_guided_params* gp, int w, int h, int order, const void* in,
                 const void* feat, const void* var, const void* out)
{
    if (!gp || !var) return pt::fail(PT_E_INVALID, "%s: null argument", who);
    if (!std::isfinite(gp->sigma_luma) || !(gp->sigma_luma > 0.0f))
        return pt::fail(PT_E_INVALID, "%s: sigma_luma must be finite and > 0", who);
    return check_params(who, c, &gp->base, w, h, order, in, feat, out);
}

// The filter on device buffers, after the checks: the plain one (d_var null: dn_* kernels, 64 B of scratch per
// pixel) or the variance-guided one (dg_* kernels, 72 B).
int filter_device(pt_ctx* c, const pt_denoise_params* dp, int w, int h, int order, const float* d_in, const pt_feature* d_feat,
                  const float* d_var, float sigma_luma, float* d_out, void* stream_v)
{
    HIP_TRY(hipSetDevice(pt::ctx_device(c)));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    const size_t n = (size_t)w * (size_t)h;
    if (dp->iterations == 0) {   // every pixel keeps its input
        if (d_out != d_in) HIP_TRY(hipMemcpyAsync(d_out, d_in, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return PT_OK;
    }
    const bool guided = d_var != nullptr;
    pt::DenoiseScratch* S = pt::ctx_denoise_scratch(c);
    const size_t need = n * 4 * sizeof(float4) + (guided ? 2 * n * sizeof(float) : 0);
    if (S->bytes < need) {
        if (S->mem) (void)hipFree(S->mem);
        S->mem = nullptr;
        S->bytes = 0;
        HIP_TRY(hipMalloc(&S->mem, need));
        S->bytes = need;
    }
    float4* const g0 = static_cast<float4*>(S->mem);
    float4* const g1 = g0 + n;
    float4* const cc[2] = {g0 + 2 * n, g0 + 3 * n};
    float* const vpl = reinterpret_cast<float*>(g0 + 4 * n);
    float* const vbar = vpl + n;
    const int morton = order == PT_ORDER_MORTON, demod = (dp->flags & PT_DENOISE_NO_DEMODULATE) ? 0 : 1;
    const dim3 grid((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4));
    if (guided)
        hipLaunchKernelGGL(dg_prepass, grid, dim3(256), 0, stream, d_in, reinterpret_cast<const float*>(d_feat), d_var, g0, g1, cc[0],
                           vpl, w, h, morton, demod, dp->sigma_depth);
    else
        hipLaunchKernelGGL(dn_prepass, grid, dim3(256), 0, stream, d_in, reinterpret_cast<const float*>(d_feat), g0, g1, cc[0], w, h,
                           morton, demod, dp->sigma_depth);
    HIP_TRY(hipGetLastError());
    // PT_DENOISE_DIRECT=1: every iteration on the direct gather (the baseline); PT_DENOISE_TILED_MAX: the
    // largest step staged through LDS (default kTiledMaxStep)
    const bool direct = env_int("PT_DENOISE_DIRECT", 0) != 0;
    int tiled_max = env_int("PT_DENOISE_TILED_MAX", kTiledMaxStep);
    if (tiled_max > kTiledLimit) tiled_max = kTiledLimit;
    for (int it = 0; it < dp->iterations; ++it) {
        DgArgs ga;
        DnArgs& a = ga.d;
        a.g0 = g0; a.g1 = g1; a.src = cc[it & 1]; a.dst = cc[(it + 1) & 1];
        a.w = w; a.h = h; a.step = 1 << it; a.npow = dp->normal_power_log2;
        a.sigma_color = (dp->sigma_color > 0.0f) ? dp->sigma_color / (float)(1 << it) : 0.0f;
        ga.vpl = vpl;
        ga.vbar = vbar;
        ga.sl2 = sigma_luma * sigma_luma;
        if (guided) {
            hipLaunchKernelGGL(dg_blur, grid, dim3(256), 0, stream, vpl, vbar, w, h);
            HIP_TRY(hipGetLastError());
        }
        if (!direct && a.step <= tiled_max) {
            const size_t lds = (size_t)3 * kStageRows * (size_t)(kTileX + 4 * a.step) * sizeof(float4);
            if (lds > 64 * 1024)   // (beyond the default dynamic-LDS limit; gfx950 has 160 KB per CU)
                HIP_TRY(hipFuncSetAttribute(guided ? reinterpret_cast<const void*>(&dg_iterate<true>)
                                                  : reinterpret_cast<const void*>(&dn_iterate<true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           3 * kStageRows * (kTileX + 4 * kTiledLimit) * (int)sizeof(float4)));
            const unsigned lat_rows = (unsigned)((h + a.step - 1) / a.step);          // rows of one residue class
            const dim3 tg((unsigned)((w + kTileX - 1) / kTileX), ((lat_rows + kRows - 1) / kRows) * (unsigned)a.step);
            if (guided) hipLaunchKernelGGL((dg_iterate<true>), tg, dim3(256), lds, stream, ga);
            else hipLaunchKernelGGL((dn_iterate<true>), tg, dim3(256), lds, stream, a);
        } else {
            if (guided) hipLaunchKernelGGL((dg_iterate<false>), grid, dim3(256), 0, stream, ga);
            else hipLaunchKernelGGL((dn_iterate<false>), grid, dim3(256), 0, stream, a);
        }
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(dn_finish, grid, dim3(256), 0, stream, cc[dp->iterations & 1], g1, reinterpret_cast<const float*>(d_feat), d_out,
                       w, h, morton, demod);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}

// ... on host buffers: copies in, filters in place on the device, copies out
int filter_host(pt_ctx* c, const pt_denoise_params* dp, int w, int h, int order, const float* in, const pt_feature* feat,
                const float* var, float sigma_luma, float* out)
{
    HIP_TRY(hipSetDevice(pt::ctx_device(c)));
    const size_t n = (size_t)w * (size_t)h;
    pt::ScopedDevice<float> d_img, d_var;
    pt::ScopedDevice<pt_feature> d_feat;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_img), n * 3 * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_feat), n * sizeof(pt_feature)));
    HIP_TRY(hipMemcpy(d_img, in, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_feat, feat, n * sizeof(pt_feature), hipMemcpyHostToDevice));
    if (var) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_var), n * sizeof(float)));
        HIP_TRY(hipMemcpy(d_var, var, n * sizeof(float), hipMemcpyHostToDevice));
    }
    if (int rc = filter_device(c, dp, w, h, order, d_img, d_feat, d_var, sigma_luma, d_img, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, d_img, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // namespace

extern "C" {

void pt_denoise_defaults(pt_denoise_params* p)
{
    if (!p) return;
    p->iterations = 5;
    p->normal_power_log2 = 5;
    p->sigma_depth = 0.02f;
    p->sigma_color = 0.0f;
    p->flags = 0;
}

int pt_denoise_device(pt_ctx* c, const pt_denoise_params* dp, int w, int h, int order, const float* d_in,
                      const pt_feature* d_feat, float* d_out, void* stream_v)
{
    pt::clear_error();
    if (int rc = check_params("pt_denoise_device", c, dp, w, h, order, d_in, d_feat, d_out)) return rc;
    return filter_device(c, dp, w, h, order, d_in, d_feat, nullptr, 0.0f, d_out, stream_v);
}

int pt_denoise(pt_ctx* c, const pt_denoise_params* dp, int w, int h, int order, const float* in, const pt_feature* feat,
               float* out)
{
    pt::clear_error();
    if (int rc = check_params("pt_denoise", c, dp, w, h, order, in, feat, out)) return rc;
    return filter_host(c, dp, w, h, order, in, feat, nullptr, 0.0f, out);
}

void pt_denoise_guided_defaults(pt_denoise_guided_params* p)
{
    if (!p) return;
    pt_denoise_defaults(&p->base);
    p->sigma_luma = 2.0f;
}

int pt_denoise_guided_device(pt_ctx* c, const pt_denoise_guided_params* gp, int w, int h, int order, const float* d_in,
                             const pt_feature* d_feat, const float* d_var, float* d_out, void* stream_v)
{
    pt::clear_error();
    if (int rc = check_guided("pt_denoise_guided_device", c, gp, w, h, order, d_in, d_feat, d_var, d_out)) return rc;
    return filter_device(c, &gp->base, w, h, order, d_in, d_feat, d_var, gp->sigma_luma, d_out, stream_v);
}

int pt_denoise_guided(pt_ctx* c, const pt_denoise_guided_params* gp, int w, int h, int order, const float* in,
                      const pt_feature* feat, const float* var, float* out)
{
    pt::clear_error();
    if (int rc = check_guided("pt_denoise_guided", c, gp, w, h, order, in, feat, var, out)) return rc;
    return filter_host(c, &gp->base, w, h, order, in, feat, var, gp->sigma_luma, out);
}

}  // extern "C"
