// pt_session.hip -- the pack / unpack kernels of a session file (include/pt/pt.h, pt_session_*), for gfx950.
// The progressive state lives in slot-major planes, in the shard's work-slot order: the accumulator's rng (6 x u32)
// and mean (3 x f64), its frozen_at words, the estimator's prev[3] / mu / m2 (5 x f64) and its W_q / b_q words.  The
// file holds per-pixel records in scanline order, one section per kind.  Two kernels move one into the other on the
// device, so that the state crosses PCIe once, already in file layout (pt_session.cpp):
//   session_pack    lanes on consecutive slots: every plane read is a coalesced 4- or 8-B-per-lane row; the slot's
//                   pixel (the slot -> pixel map) says where its records go: section A as three 16-B stores, B one
//                   word, C five 8-B stores (a 40-B record is only 8-B aligned), D one 8-B store.  Slots outside the
//                   image write nothing, and pixels of other shards are never written: the host zeroes the staging
//                   first when the shard does not own the whole image.
//   session_unpack  the inverse gather; a slot outside the image gets what a new accumulator / estimator holds there
//                   (zeros; frozen_at 0, as adaptive_alloc).
// Both count the frozen pixels (unpack also the section-B words that are neither "active" nor <= samples) per wave
// with ballot + popcount, per block through LDS, and flush with one global atomic per block into one of
// kSessionSumCopies copies of the counters at the head of the staging, like pt_noise.hip's sums.  All integer: no
// reduction-order effects.
#include <hip/hip_runtime.h>

#include "../host/host_internal.h"
#include "pt_hip_util.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kBlocksPerCu = 8;   // grid cap, the rest of the slots by grid stride

__device__ __forceinline__ void flush_counts(const pt::SessionPlanes& a, const uint32_t* cnt)
{
    unsigned long long* const sum =
        reinterpret_cast<unsigned long long*>(a.stage) + (blockIdx.x % pt::kSessionSumCopies) * pt::kSessionSumWords;
    if (threadIdx.x < pt::kSessionSumWords && cnt[threadIdx.x]) atomicAdd(&sum[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

__global__ __launch_bounds__(kBlock) void session_pack_planes(pt::SessionPlanes a)
{
    __shared__ uint32_t cnt[pt::kSessionSumWords];
    if (threadIdx.x < pt::kSessionSumWords) cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t n = a.slots;
    uint4* const sec_a = reinterpret_cast<uint4*>(a.stage + a.at.a);
    uint32_t* const sec_b = reinterpret_cast<uint32_t*>(a.stage + a.at.b);
    double* const sec_c = reinterpret_cast<double*>(a.stage + a.at.c);
    uint2* const sec_d = reinterpret_cast<uint2*>(a.stage + a.at.d);
    uint32_t wave_frozen = 0;   // (wave-uniform)
    for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kBlock) {
        const size_t pix = a.slot_pix[q];
        const bool pixel = pix < a.image_pixels;
        bool frozen = false;
        if (pixel) {
            uint32_t r[6];
            unsigned long long m[3];
#pragma unroll
            for (int k = 0; k < 6; ++k) r[k] = a.samples ? a.rng[k * n + q] : 0u;   // (0 samples: all zero, as format 1)
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = a.samples ? (unsigned long long)__double_as_longlong(a.mean[k * n + q]) : 0ull;
            sec_a[pix * 3 + 0] = make_uint4(r[0], r[1], r[2], r[3]);
            sec_a[pix * 3 + 1] = make_uint4(r[4], r[5], (uint32_t)m[0], (uint32_t)(m[0] >> 32));
            sec_a[pix * 3 + 2] = make_uint4((uint32_t)m[1], (uint32_t)(m[1] >> 32), (uint32_t)m[2], (uint32_t)(m[2] >> 32));
            if (a.frozen_at) {
                const uint32_t at = a.frozen_at[q];
                sec_b[pix] = at;
                frozen = at != pt::kSlotActive;
            }
            if (a.nstate) {
#pragma unroll
                for (int k = 0; k < 5; ++k) sec_c[pix * 5 + k] = a.nstate[k * n + q];
            }
            if (a.npix) sec_d[pix] = make_uint2(a.npix[q], a.npix[n + q]);
        }
        wave_frozen += (uint32_t)__popcll(__ballot(frozen));
    }
    if ((threadIdx.x & 63) == 0 && wave_frozen) atomicAdd(&cnt[0], wave_frozen);
    __syncthreads();
    flush_counts(a, cnt);
}

__global__ __launch_bounds__(kBlock) void session_unpack_planes(pt::SessionPlanes a)
{
    __shared__ uint32_t cnt[pt::kSessionSumWords];
    if (threadIdx.x < pt::kSessionSumWords) cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t n = a.slots;
    const uint4* const sec_a = reinterpret_cast<const uint4*>(a.stage + a.at.a);
    const uint32_t* const sec_b = reinterpret_cast<const uint32_t*>(a.stage + a.at.b);
    const double* const sec_c = reinterpret_cast<const double*>(a.stage + a.at.c);
    const uint2* const sec_d = reinterpret_cast<const uint2*>(a.stage + a.at.d);
    uint32_t wave_frozen = 0, wave_bad = 0;   // (wave-uniform)
    for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kBlock) {
        const size_t pix = a.slot_pix[q];
        const bool pixel = pix < a.image_pixels;
        uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0, v2 = v0;
        if (pixel) {
            v0 = sec_a[pix * 3 + 0];
            v1 = sec_a[pix * 3 + 1];
            v2 = sec_a[pix * 3 + 2];
        }
        a.rng[0 * n + q] = v0.x; a.rng[1 * n + q] = v0.y; a.rng[2 * n + q] = v0.z; a.rng[3 * n + q] = v0.w;
        a.rng[4 * n + q] = v1.x; a.rng[5 * n + q] = v1.y;
        a.mean[0 * n + q] = __longlong_as_double((long long)(((unsigned long long)v1.w << 32) | v1.z));
        a.mean[1 * n + q] = __longlong_as_double((long long)(((unsigned long long)v2.y << 32) | v2.x));
        a.mean[2 * n + q] = __longlong_as_double((long long)(((unsigned long long)v2.w << 32) | v2.z));
        bool frozen = false, bad = false;
        if (a.frozen_at) {
            const uint32_t at = pixel ? sec_b[pix] : 0u;
            a.frozen_at[q] = at;
            frozen = pixel && at != pt::kSlotActive;
            bad = frozen && at > a.samples;
        }
        if (a.nstate) {
#pragma unroll
            for (int k = 0; k < 5; ++k) a.nstate[k * n + q] = pixel ? sec_c[pix * 5 + k] : 0.0;
        }
        if (a.npix) {
            const uint2 wb = pixel ? sec_d[pix] : make_uint2(0u, 0u);
            a.npix[q] = wb.x;
            a.npix[n + q] = wb.y;
        }
        wave_frozen += (uint32_t)__popcll(__ballot(frozen));
        wave_bad += (uint32_t)__popcll(__ballot(bad));
    }
    if ((threadIdx.x & 63) == 0) {
        if (wave_frozen) atomicAdd(&cnt[0], wave_frozen);
        if (wave_bad) atomicAdd(&cnt[1], wave_bad);
    }
    __syncthreads();
    flush_counts(a, cnt);
}

unsigned grid_of(const pt_ctx* c, size_t slots)
{
    const size_t blocks = (slots + kBlock - 1) / kBlock;
    const size_t cap = (size_t)pt::ctx_num_cus(c) * kBlocksPerCu;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

int pt::session_pack(pt_ctx* c, const pt::SessionPlanes& pl, void* stream_v)
{
    if (!pl.slots) return PT_OK;
    hipLaunchKernelGGL(session_pack_planes, dim3(grid_of(c, pl.slots)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream_v), pl);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int pt::session_unpack(pt_ctx* c, const pt::SessionPlanes& pl, void* stream_v)
{
    if (!pl.slots) return PT_OK;
    hipLaunchKernelGGL(session_unpack_planes, dim3(grid_of(c, pl.slots)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream_v), pl);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}
