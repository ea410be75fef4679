// pt_rays.hip -- the classes of a caller's ray buffer (pt_rays_classify_device; the check in front of every
// pt_render_rays*) and of a point buffer (pt_points_classify_device; pt_render_irradiance*): their own gfx950 kernels,
// no render-path code.  The three classes are pt.h's: invalid (a non-finite
// component, or a direction of exactly 0), regular (ray_regular of pt_device.h, the one definition the trace and
// query kernels use) and irregular (every other valid ray).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_device.h"
#include "pt_hip_util.h"

using namespace ptd;

namespace {

constexpr uint32_t kClassifyBlock = 256;   // 4 waves, one ray per lane and pass

// One ray per lane, grid-stride over blocks of 256 rays.  A ray is 24 B, so a lane's own record is three 8-byte words
// at a 24-byte stride: instead, a wave reads its 64 records (1536 B in a row) as three fully coalesced 512-byte
// loads, float2 k * 64 + lane of the row, parks them in LDS and reads its own record back from there.  The class counts
// are taken by ballot and popcount and kept per wave across the passes: at the kernel's end a wave issues one atomic
// add per class it saw, and one atomicMin of the lowest invalid index if it saw an invalid ray.  All four results are
// integers (sums and a minimum), so no answer depends on the order of the waves.
// out: regular, irregular, invalid, first_invalid (the host sets 0, 0, 0, 0xffffffff before the launch).
__global__ __launch_bounds__(kClassifyBlock) void classify_rays(const float2* __restrict__ rays, uint32_t n, float origin_max,
                                                                uint32_t* __restrict__ out)
{
    __shared__ float2 row[kClassifyBlock * 3];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float2* const wrow = row + wave * 192u;
    uint32_t n_reg = 0, n_irr = 0, n_inv = 0, first = 0xffffffffu;   // wave-uniform
    const uint64_t words = (uint64_t)n * 3u;                         // float2 words of the buffer
    for (uint64_t base = (uint64_t)blockIdx.x * kClassifyBlock; base < n; base += (uint64_t)gridDim.x * kClassifyBlock) {
        const uint64_t wbase = base + wave * 64u;   // the wave's first ray (it may lie past the end)
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) {
            const uint64_t j = wbase * 3u + k * 64u + lane;
            if (j < words) wrow[k * 64u + lane] = rays[j];
        }
        __syncthreads();
        const uint64_t r = wbase + lane;
        const bool live = r < n;
        bool invalid = false, regular = false;
        if (live) {
            const float2 a = wrow[3u * lane], b = wrow[3u * lane + 1u], c = wrow[3u * lane + 2u];
            const V3 o = v3(a.x, a.y, b.x), d = v3(b.y, c.x, c.y);
            const bool finite = __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) &&
                                __builtin_isfinite(d.x) && __builtin_isfinite(d.y) && __builtin_isfinite(d.z);
            invalid = !finite || (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
            regular = !invalid && ray_regular(o, d, origin_max);
        }
        const uint64_t m_inv = __ballot(invalid), m_reg = __ballot(regular), m_live = __ballot(live);
        n_inv += (uint32_t)__popcll(m_inv);
        n_reg += (uint32_t)__popcll(m_reg);
        n_irr += (uint32_t)__popcll(m_live & ~m_inv & ~m_reg);
        if (m_inv != 0ull) first = min(first, (uint32_t)wbase + (uint32_t)(__ffsll((long long)m_inv) - 1));
        __syncthreads();   // (the next pass overwrites the rows)
    }
    if (lane == 0u) {
        if (n_reg) atomicAdd(out + 0, n_reg);
        if (n_irr) atomicAdd(out + 1, n_irr);
        if (n_inv) { atomicAdd(out + 2, n_inv); atomicMin(out + 3, first); }
    }
}

// The classes of a point buffer (pt_points_classify_device; the check in front of every pt_render_irradiance*): records
// {p.xyz, n.xyz} read, counted and reported exactly as classify_rays does its rays.  pt.h's classes, all in float32:
// invalid -- a non-finite component, or (n.x*n.x + n.y*n.y) + n.z*n.z outside [1 - 2^-10, 1 + 2^-10]; regular --
// max |p_k| <= origin_max; irregular -- every other valid point.  (The direction a sample hands to the walk is
// normalised in float32 whatever the normal's length within that band, so only the position decides regularity.)
constexpr float kNormalLen2Min = 1.0f - 0x1p-10f, kNormalLen2Max = 1.0f + 0x1p-10f;
__global__ __launch_bounds__(kClassifyBlock) void classify_points(const float2* __restrict__ pts, uint32_t n, float origin_max,
                                                                  uint32_t* __restrict__ out)
{
    __shared__ float2 row[kClassifyBlock * 3];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float2* const wrow = row + wave * 192u;
    uint32_t n_reg = 0, n_irr = 0, n_inv = 0, first = 0xffffffffu;   // wave-uniform
    const uint64_t words = (uint64_t)n * 3u;                         // float2 words of the buffer
    for (uint64_t base = (uint64_t)blockIdx.x * kClassifyBlock; base < n; base += (uint64_t)gridDim.x * kClassifyBlock) {
        const uint64_t wbase = base + wave * 64u;   // the wave's first point (it may lie past the end)
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) {
            const uint64_t j = wbase * 3u + k * 64u + lane;
            if (j < words) wrow[k * 64u + lane] = pts[j];
        }
        __syncthreads();
        const uint64_t r = wbase + lane;
        const bool live = r < n;
        bool invalid = false, regular = false;
        if (live) {
            const float2 a = wrow[3u * lane], b = wrow[3u * lane + 1u], c = wrow[3u * lane + 2u];
            const V3 p = v3(a.x, a.y, b.x), nr = v3(b.y, c.x, c.y);
            const bool finite = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z) &&
                                __builtin_isfinite(nr.x) && __builtin_isfinite(nr.y) && __builtin_isfinite(nr.z);
            const float nn = (nr.x * nr.x + nr.y * nr.y) + nr.z * nr.z;   // (an overflow fails the upper bound)
            invalid = !finite || !(nn >= kNormalLen2Min && nn <= kNormalLen2Max);
            const float m = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(p.x), __builtin_fabsf(p.y)), __builtin_fabsf(p.z));
            regular = !invalid && m <= origin_max;
        }
        const uint64_t m_inv = __ballot(invalid), m_reg = __ballot(regular), m_live = __ballot(live);
        n_inv += (uint32_t)__popcll(m_inv);
        n_reg += (uint32_t)__popcll(m_reg);
        n_irr += (uint32_t)__popcll(m_live & ~m_inv & ~m_reg);
        if (m_inv != 0ull) first = min(first, (uint32_t)wbase + (uint32_t)(__ffsll((long long)m_inv) - 1));
        __syncthreads();   // (the next pass overwrites the rows)
    }
    if (lane == 0u) {
        if (n_reg) atomicAdd(out + 0, n_reg);
        if (n_irr) atomicAdd(out + 1, n_irr);
        if (n_inv) { atomicAdd(out + 2, n_inv); atomicMin(out + 3, first); }
    }
}

}  // namespace

// The classes of d_rays[0..n) (device, 8-byte aligned) into *res, through the four device words d_words; blocking.
// points: the records are points {p, n} (classify_points) instead of rays.
int pt::classify_ray_buffer(const float* d_rays, uint32_t n, float origin_max, int num_cus, uint32_t* d_words, void* stream_v,
                      pt_ray_classes* res, bool points)
{
    res->regular = res->irregular = res->invalid = 0;
    res->first_invalid = 0xffffffffu;
    res->pad = 0;
    if (n == 0) return PT_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    HIP_TRY(hipMemsetAsync(d_words, 0, 12, stream));
    HIP_TRY(hipMemsetAsync(d_words + 3, 0xff, 4, stream));
    uint32_t blocks = (uint32_t)(((uint64_t)n + kClassifyBlock - 1) / kClassifyBlock);
    blocks = std::min(blocks, (uint32_t)std::max(num_cus, 1) * 8u);
    hipLaunchKernelGGL(points ? classify_points : classify_rays, dim3(blocks), dim3(kClassifyBlock), 0, stream,
                       reinterpret_cast<const float2*>(d_rays), n, origin_max, d_words);
    HIP_TRY(hipGetLastError());
    uint32_t h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, d_words, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    res->regular = h[0];
    res->irregular = h[1];
    res->invalid = h[2];
    res->first_invalid = h[3];
    return PT_OK;
}
